"""The inputs of the nodal stress tests, shared by test_mirror_stress.py (CPU: the conditioning of every case) and
test_gpu_stress_field.py (the device against the reference): meshes, material, roles and states as test_gpu_energy.py.

Meshes: the smallest at which each kernel form can go wrong, box and vertex-perturbed (0.1 h) each -- stress_q3 on 2 x 2 x 2 and
3 x 2 x 3, stress_q2 on 2 x 2 x 2 and 3 x 2 x 2, stress_cells on 2D p = 1..4 (3 x 2), 3D p = 1 (2 x 2 x 2) and 3D p = 4 (1 x 1 x 2);
teams on 3D Q2 and Q3 2 x 2 x 4 and 2D Q2 6 x 2.  State: u = amp randn on the free dofs; amp is halved from 0.02 until the
REFERENCE's smallest det F is >= 0.4.  Every case is built once and left unchanged.
"""
import numpy as np

import mirror as Mi
import stress_reference as S

MU, NU, RHO = 0.7e6, 0.3, 870.0
ROLES = [1, 7, 0, 7, 8, 0]  # x- clamped, x+ / y+ interface, z- clamped in z (3D)

# (dim, degree, reps): by kernel form
Q3_MESHES = [(3, 3, (2, 2, 2)), (3, 3, (3, 2, 3))]
Q2_MESHES = [(3, 2, (2, 2, 2)), (3, 2, (3, 2, 2))]
GENERIC_MESHES = [(2, 1, (3, 2)), (2, 2, (3, 2)), (2, 3, (3, 2)), (2, 4, (3, 2)), (3, 1, (2, 2, 2)), (3, 4, (1, 1, 2))]
TEAM_MESHES = [(3, 2, (2, 2, 4)), (3, 3, (2, 2, 4)), (2, 2, (6, 2))]

# what test_gpu_stress_field.py compares with the reference: (mesh, perturbed, model)
REFERENCE_CASES = ([(m, pt, S.NEOHOOKE) for m in Q3_MESHES + Q2_MESHES + GENERIC_MESHES for pt in (False, True)] +
                   [(m, pt, S.LINEAR) for m in GENERIC_MESHES + [Q2_MESHES[1], Q3_MESHES[1]] for pt in (False, True)])
TEAM_CASES = [(m, True, S.NEOHOOKE) for m in TEAM_MESHES]

_cases = {}


def case(dim, p, reps, perturbed):
    """mesh and admissible state of a case; .ref(model) = (sigma, von_mises, W, min det F) of the reference, computed once"""
    key = (dim, p, tuple(reps), perturbed)
    if key in _cases:
        return _cases[key]
    reps = tuple(reps)
    h = 0.1
    hi = tuple(h * r for r in reps)
    rng = np.random.default_rng(100 * dim + 10 * p + sum(reps) + int(perturbed))
    nv = int(np.prod([r + 1 for r in reps]))
    perturb = 0.1 * h * rng.uniform(-1, 1, (nv, dim)) if perturbed else None
    roles = ROLES[:2 * dim]
    m = Mi.Mesh(dim, p, reps, (0.0,) * dim, hi, roles, perturb=perturb)
    u0 = rng.standard_normal(m.n) * ~m.constrained
    amp = 0.02
    while True:
        with np.errstate(invalid="ignore"):  # (a folded point on the way down: J^(-2/dim) of a negative J)
            pts = S.points(m, amp * u0, MU, NU, S.NEOHOOKE)
        if min(pt[4] for pt in pts) >= 0.4:
            break
        amp *= 0.5
    c = dict(dim=dim, p=p, reps=reps, hi=hi, perturb=perturb, roles=roles, mesh=m, u=amp * u0, pts={S.NEOHOOKE: pts}, refs={})
    _cases[key] = c
    return c


def points(c, model):
    if model not in c["pts"]:
        c["pts"][model] = S.points(c["mesh"], c["u"], MU, NU, model)
    return c["pts"][model]


def ref(c, model):
    if model not in c["refs"]:
        c["refs"][model] = S.nodal_stress(c["mesh"], c["u"], MU, NU, model, pts=points(c, model))
    return c["refs"][model]
