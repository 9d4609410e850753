"""CPU: the linear model of tests/golden/mirror.py (mirror.Linear) that test_gpu_linear_model_reference.py holds the device's
operators, right-hand sides and steps to.

On box meshes it is checked against the C++ oracle (oracle_lib.LinearProblem, which takes no vertex perturbation): K, M, the
stepping matrix and the system matrix entry by entry, the right-hand side and the state of three steps.  On distorted meshes,
where nothing else computes the same operators, it is checked against what the continuum says: K is symmetric and
annihilates the rigid-body modes, the mass matrix sums to rho times the mesh volume (the volume from a Gauss integral of
det J written here), and the body-force vector is M (b, b, ...) because the shape functions sum to one."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402

CL, IF, ZC = O.FACE_CLAMPED, O.FACE_INTERFACE, O.FACE_ZCLAMP
ROLES = [CL, IF, IF, IF, ZC, IF]
# none of them a default; theta away from 0.5 and 1, rho away from 1
MAT = dict(mu=0.7e6, nu=0.3, rho=870.0, delta_t=0.004)
THETA = 0.65
BODY = (0.3, -9.81, 2.0)

# (dim, degree, reps, hi): anisotropic cells
BOXES = [
    (2, 1, (4, 3), (1.3, 0.6)),
    (2, 2, (3, 2), (0.9, 0.5)),
    (2, 3, (3, 2), (1.1, 0.4)),
    (2, 4, (2, 2), (0.7, 0.5)),
    (3, 1, (3, 2, 3), (1.5, 0.7, 1.1)),
    (3, 2, (2, 2, 2), (0.5, 0.35, 0.55)),
    (3, 3, (2, 1, 2), (0.8, 0.3, 0.6)),
]


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _box_pair(dim, p, reps, hi, body):
    P = O.LinearProblem(O.make_desc(dim=dim, degree=p, reps=reps, hi=hi, face_role=ROLES, theta=THETA,
                                    body_force=tuple(body) + (0.0,) * (3 - len(body)), **MAT))
    m = Mi.Mesh(dim, p, reps, (0.0,) * dim, hi, ROLES)
    Ml = Mi.Linear(m, MAT["mu"], MAT["nu"], MAT["rho"], tuple(body)[:dim], MAT["delta_t"], THETA)
    assert np.abs(m.coords - P.coords).max() < 1e-15 and np.array_equal(m.constrained, P.constrained)
    assert np.array_equal(m.interface_nodes, P.interface_nodes)
    return P, m, Ml


@pytest.mark.parametrize("dim,p,reps,hi", BOXES)
def test_linear_matrices_against_the_oracle(dim, p, reps, hi):
    """K, M, M + theta^2 dt^2 K and the matrix after apply_boundary_values, entry by entry, to 1e-12 of the largest entry"""
    P, m, Ml = _box_pair(dim, p, reps, hi, BODY)
    assert 0 < m.constrained.sum() < m.n
    if dim == 3:  # nodes with the z component alone constrained: the z-clamped face
        c = m.constrained.reshape(-1, 3)
        assert (c[:, 2] & ~c[:, 0]).any()
    assert P.step(O.SOLVER_DIRECT, True)[0] == 0  # the oracle forms its system matrix in a step (here one of zero data)
    err = {}
    for which, ref in ((0, Ml.K), (1, Ml.M), (2, Ml.stepping), (3, Ml.system_matrix())):
        err[which] = _relmax(P.matrix(which).toarray(), ref)
    print("Q%d %dD %s: relmax K, M, stepping, system" % (p, dim, reps), err)
    assert all(e < 1e-12 for e in err.values()), err


@pytest.mark.parametrize("body", [BODY, (0.0, 0.0, 0.0)], ids=["body_force", "no_body_force"])
@pytest.mark.parametrize("dim,p,reps,hi", BOXES)
def test_linear_steps_against_the_oracle(dim, p, reps, hi, body):
    """three steps, "Stress" / "Force" / "Stress", random interface data: the right-hand side to 1e-12 of max |rhs|, d and
    v to 1e-9 (both sides solve directly)"""
    P, m, Ml = _box_pair(dim, p, reps, hi, body)
    rng = np.random.default_rng(100 * dim + p)
    ids = m.interface_nodes
    worst = {"rhs": 0.0, "d": 0.0, "v": 0.0}
    for step in range(3):
        consistent = step != 1
        t = MAT["mu"] * 1e-4 * rng.standard_normal((len(ids), dim))
        P.vec(O.L_STRESS)[:] = 0
        Ml.stress[:] = 0
        for c in range(dim):
            P.vec(O.L_STRESS)[ids * dim + c] = t[:, c]
            Ml.stress[ids * dim + c] = t[:, c]
        assert P.step(O.SOLVER_DIRECT, consistent)[0] == 0
        rhs = Ml.step(consistent)
        worst["rhs"] = max(worst["rhs"], _relmax(rhs, P.vec(O.L_RHS)))
        worst["d"] = max(worst["d"], _relmax(Ml.d, P.vec(O.L_D)))
        worst["v"] = max(worst["v"], _relmax(Ml.v, P.vec(O.L_V)))
        assert _relmax(Ml.f_old, P.vec(O.L_STRESS_OLD)) < 1e-12
    print("Q%d %dD %s: worst relmax over three steps" % (p, dim, reps), worst)
    assert worst["rhs"] < 1e-12 and worst["d"] < 1e-9 and worst["v"] < 1e-9, worst


# the distorted meshes: (dim, degree, reps), vertices moved by 0.08 min h of normal noise
DISTORTED = [(3, 3, (2, 1, 2)), (3, 3, (3, 2, 2)), (2, 4, (3, 2)), (3, 2, (2, 2, 2))]
_cache = {}


def _distorted(dim, p, reps):
    key = (dim, p, reps)
    if key not in _cache:
        h = np.array([0.13, 0.1, 0.07])[:dim]
        rng = np.random.default_rng(sum(reps) + p)
        nverts = int(np.prod([r + 1 for r in reps]))
        perturb = 0.08 * h.min() * rng.standard_normal((nverts, dim))
        m = Mi.Mesh(dim, p, reps, (0.0,) * dim, tuple(h * np.array(reps)), ROLES, perturb=perturb)
        _cache[key] = m, Mi.Linear(m, MAT["mu"], MAT["nu"], MAT["rho"], BODY[:dim], MAT["delta_t"], THETA)
    return _cache[key]


def _volume(m):
    """sum over the cells of the integral of det(dX/dxi) of the d-linear map over the unit cell, by the 2-point Gauss rule per
    direction (det J has degree at most 2 in each xi_d, which 2 points integrate exactly).  verts[v]: bit d of v = upper end
    in direction d"""
    dim = m.dim
    g = 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0)  # points of the 2-point rule on [0, 1], weights 1/2 each
    vol = 0.0
    for _, verts, _ in m.cells:
        for q in np.ndindex(*([2] * dim)):
            xi = g[list(q)]
            J = np.zeros((dim, dim))
            for v in range(1 << dim):
                up = [(v >> d) & 1 for d in range(dim)]
                for j in range(dim):  # d phi_v / d xi_j
                    dphi = 1.0 if up[j] else -1.0
                    for d in range(dim):
                        if d != j:
                            dphi *= xi[d] if up[d] else 1.0 - xi[d]
                    J[:, j] += dphi * verts[v]
            vol += np.linalg.det(J) / 2**dim
    return vol


def _rigid_modes(X):
    """translations and infinitesimal rotations of the nodes X[n, dim], as dof vectors"""
    n, dim = X.shape
    modes = []
    for c in range(dim):
        u = np.zeros((n, dim))
        u[:, c] = 1.0
        modes.append(u.reshape(-1))
    for a, b in ((0, 1),) if dim == 2 else ((0, 1), (1, 2), (2, 0)):  # u = w x X
        u = np.zeros((n, dim))
        u[:, a], u[:, b] = -X[:, b], X[:, a]
        modes.append(u.reshape(-1))
    return modes


@pytest.mark.parametrize("dim,p,reps", DISTORTED)
def test_linear_on_distorted_cells(dim, p, reps):
    """no second implementation exists off box meshes, so the mirror is held to what must be true there: K and M symmetric,
    K on translations and infinitesimal rotations below 1e-13 max|K| max|X|, 1^T M 1 / dim = rho times the volume of the
    mesh, body vector = M (b, b, ...); the roles put nodes under a z-only constraint"""
    m, Ml = _distorted(dim, p, reps)
    K, M = Ml.K, Ml.M
    assert np.abs(K - K.T).max() <= 1e-15 * np.abs(K).max()
    assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max()
    if dim == 3:
        c = m.constrained.reshape(-1, 3)
        assert (c[:, 2] & ~c[:, 0]).any()
    scale = np.abs(K).max() * np.abs(m.coords).max()
    modes = _rigid_modes(m.coords)
    assert len(modes) == (3 if dim == 2 else 6)
    worst = max(np.abs(K @ u).max() for u in modes) / scale
    vol = _volume(m)
    box = np.prod(0.0 + np.array([0.13, 0.1, 0.07])[:dim] * np.array(reps))
    assert 0.5 * box < vol < 1.5 * box and vol != box
    one = np.ones(m.n)
    mass = one @ M @ one / dim
    b = np.tile(BODY[:dim], m.nnodes)
    print("Q%d %dD %s distorted: max|K rigid| / (max|K| max|X|) %.1e, mass / (rho vol) - 1 %.1e, body relmax %.1e"
          % (p, dim, reps, worst, mass / (MAT["rho"] * vol) - 1, _relmax(Ml.body_vec, M @ b)))
    assert worst <= 1e-13
    assert abs(mass - MAT["rho"] * vol) <= 1e-13 * MAT["rho"] * vol
    assert _relmax(Ml.body_vec, M @ b) <= 1e-13
