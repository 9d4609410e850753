"""The inputs of the stress error indicator's tests, shared by test_mirror_stress_error.py (CPU) and test_gpu_stress_error.py:
every case of stress_cases.REFERENCE_CASES (imported, unchanged), and two meshes of more than 1,024 cells with an odd remainder
for the second level of the fixed-order sum.  Every reference is computed once and left unchanged.

The two large meshes carry a smooth state (no search for an admissible amplitude over ~10^4 points) and one model each, the
cheaper rule in 3D: 3D Q1 11 x 10 x 10 with model 1 (8 points per cell), 2D Q1 35 x 30 with model 0 (9 points per cell).
"""
import numpy as np

import mirror as Mi
import stress_cases as SC
import stress_error_reference as R
import stress_reference as S

MU, NU, RHO = SC.MU, SC.NU, SC.RHO

# (dim, degree, reps), perturbed, model
REDUCTION_CASES = [((3, 1, (11, 10, 10)), True, S.LINEAR), ((2, 1, (35, 30)), True, S.NEOHOOKE)]
ALL_CASES = SC.REFERENCE_CASES + REDUCTION_CASES

_big, _refs = {}, {}


def _smooth_case(dim, p, reps, perturbed):
    reps = tuple(reps)
    h = 0.1
    hi = tuple(h * r for r in reps)
    rng = np.random.default_rng(100 * dim + 10 * p + sum(reps) + int(perturbed))
    nv = int(np.prod([r + 1 for r in reps]))
    perturb = 0.1 * h * rng.uniform(-1, 1, (nv, dim)) if perturbed else None
    roles = SC.ROLES[:2 * dim]
    m = Mi.Mesh(dim, p, reps, (0.0,) * dim, hi, roles, perturb=perturb)
    X = m.coords
    u = np.zeros((m.nnodes, dim))
    for d in range(dim):  # gradients of a few per cent, and a different field in every cell
        u[:, d] = 0.004 * np.sin(3.0 * X[:, d] + 0.4 * d) * np.cos(2.0 * X[:, (d + 1) % dim] + 0.1) + 0.0005 * rng.standard_normal(m.nnodes)
    u = u.reshape(-1) * ~m.constrained
    return dict(dim=dim, p=p, reps=reps, hi=hi, perturb=perturb, roles=roles, mesh=m, u=u, pts={}, refs={})


def case(dim, p, reps, perturbed):
    if ((dim, p, tuple(reps)), perturbed) in [(m, pt) for m, pt, _ in REDUCTION_CASES]:
        key = (dim, p, tuple(reps), perturbed)
        if key not in _big:
            _big[key] = _smooth_case(dim, p, reps, perturbed)
        return _big[key]
    return SC.case(dim, p, reps, perturbed)


def points(c, model):
    return SC.points(c, model)  # (reads the case's mesh and state alone: the large cases too)


def ref(c, model):
    """the reference's dict (stress_error_reference.stress_error) of a case, computed once"""
    key = (id(c), model)
    if key not in _refs:
        _refs[key] = R.stress_error(c["mesh"], c["u"], MU, NU, model, pts=points(c, model))
    return _refs[key]
