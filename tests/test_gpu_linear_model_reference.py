"""GPU: the linear model (mi_linear_setup / mi_linear_step) against an independent reference off box meshes.

The CPU oracle's linear problem takes no vertex perturbation, so on graded and distorted cells the library was only ever
compared with itself.  Here both operator forms -- assembled ("linear_operator" 0: assemble_linear_cells + the sliced-ELL
product) and matrix-free (1: mf_linear_q3, mf_linear_diag_q3, mf_linear_diag_gather + the slot gathers, 3D Q3) -- are held to
tests/golden/mirror.py's Linear: dense K, M, stepping matrix, body vector, consistent load and step in numpy, itself anchored
to the oracle on boxes and to rigid-body modes, volume and body vector on distorted cells by test_mirror_linear.py.

Operators: y = K x, M x, A x on all rows with x non-zero on constrained dofs, the Jacobi diagonal, the assembled matrices entry
by entry; symmetry, rigid-body modes and total mass without a reference.  Every material differs from the defaults, theta is
neither 0.5 nor 1 and rho is not 1 (c_K = theta^2 dt^2 then differs from dt^2 and dt^2 / 4), one material has nu = 0.
Matrix-free cases: 1, 2, 4, 5, 9, 12 cells (one wave per cell, four waves per workgroup), BOX instances with per-cell 1 / h
(cube, graded) and the trilinear map (distorted), faces that constrain z alone.  "cell_lattice" 0 and 1 are both run on the
graded and distorted cases; a Q3 context builds no cell lattice (the key reads back 0 either way), so the two runs must agree
bit for bit, which is asserted.

Steps: "Stress", "Force", "Stress" with random interface data from non-zero d, v and F_n, scaled so that M v, dt K d, the old
and the new load weigh the same in the first right-hand side.  After each step MI_L_SYSTEM_RHS and MI_L_OLD_STRESS against the
mirror to 1e-12 of max |rhs| -- the device keeps both: the PCG holds its residual in a work vector and the band solver only
reads the right-hand side, so nothing of it is overwritten by the solve -- and d and v to 1e-7 after a solve to 1e-13 max |rhs|;
on the banded route ("solver_type" 1) to 1e-10.  After the comparisons the mirror takes the device's d and v, so that the next
right-hand side is compared from the same state; left to run free, the 1e-13 of the solve shows in the right-hand sides of
steps two and three (up to 3.0e-13 of max |rhs|, seen once), which says nothing about the kernels that form them.

Tolerance of operators and right-hand sides: relmax = max |y - y_ref| / max |y_ref| <= 1e-12 (fp64; the figure of
test_gpu_smoother_operator.py and of the distorted test in test_gpu_linear_matrix_free.py).  Observed worst (MI355X):
  matrix-free operators   K 1.6e-15, M 2.4e-15, A 1.8e-15, diagonal 2.1e-15
  assembled operators     entries of K / M / A 2.2e-15 / 2.7e-15 / 2.1e-15; products 2.2e-15 / 3.0e-15 / 1.6e-15; diagonal 2.1e-15
  properties              asymmetry <= 3.7e-17 of |x| . |B y|; K on rigid-body modes 4.3e-15 (assembled), 5.8e-16 (matrix-free)
                          of the scale, the mirror's own K 3.8e-15; total mass equal to the last digit
  matrix-free steps       rhs 1.4e-14, F_n 6.3e-14 (of max |rhs|); d 4.8e-13, v 3.4e-13
  assembled steps, PCG    rhs 1.2e-14, F_n 5.4e-14; d 2.0e-13, v 2.0e-13 (one and two slabs alike)
  assembled steps, banded rhs 2.9e-15, F_n 5.4e-14; d 9.1e-15, v 1.3e-14
"""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg
from test_gpu_smoother_operator import ROLES_A, ROLES_B, _geometry, _relmax

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

L_D, L_V, L_F_OLD, L_RHS = 0, 2, 4, 9  # MI_L_DISPLACEMENT, MI_L_VELOCITY, MI_L_OLD_STRESS, MI_L_SYSTEM_RHS
TOL = 1e-12
TOL_SOL = 1e-7  # d and v after a PCG solve to 1e-13 max|rhs| (test_steps, test_random_linear_model)
TOL_BAND = 1e-10  # ... after the band solver (test_golden)
BODY = (0.3, -9.81, 2.0)
MATS = {
    "a": dict(mu=0.7e6, nu=0.3, rho=870.0, delta_t=0.004, theta=0.65),
    "b": dict(mu=1.3e6, nu=0.0, rho=2300.0, delta_t=0.011, theta=0.8),
    "c": dict(mu=0.4e6, nu=0.42, rho=310.0, delta_t=0.0025, theta=0.55),
}


# ------------------------------------------------------------------ meshes and references
def _geometry_nd(dim, kind, reps, seed):
    """_geometry of test_gpu_smoother_operator.py, and the same construction in 2D"""
    if dim == 3:
        return _geometry(kind, reps, seed)
    reps = np.array(reps)
    if kind == "cube":
        return (0.0, 0.0), tuple(0.1 * reps), None
    h = np.array([0.13, 0.1])
    rng = np.random.default_rng(seed)
    nv = reps + 1
    vid = np.stack(np.meshgrid(np.arange(nv[0]), np.arange(nv[1]), indexing="ij"), -1).transpose(1, 0, 2).reshape(-1, 2)
    if kind == "graded":
        planes = [0.3 * h[d] * rng.uniform(-1, 1, nv[d]) for d in range(2)]
        return (0.0, 0.0), tuple(h * reps), np.stack([planes[d][vid[:, d]] for d in range(2)], -1)
    assert kind == "distorted"
    return (0.0, 0.0), tuple(h * reps), 0.08 * h.min() * rng.standard_normal((len(vid), 2))


_built = {}  # geometry -> (lo, hi, perturb, Linear of the first role set asked for): K and M do not depend on the roles
_refs = {}  # (geometry, roles) -> Linear over a Mesh of those roles, sharing the matrices


def _reference(geom, roles):
    """the mirror of a case, built once: geom = (dim, degree, kind, reps, material); returns (lo, hi, perturb, Linear)"""
    dim, degree, kind, reps, mat = geom
    key = (geom, tuple(roles))
    if key not in _refs:
        if geom not in _built:
            lo, hi, perturb = _geometry_nd(dim, kind, reps, seed=sum(reps) + degree)
            _built[geom] = (lo, hi, perturb, None)
        lo, hi, perturb, first = _built[geom]
        m = Mi.Mesh(dim, degree, reps, lo, hi, roles, perturb=perturb)
        if first is None:
            k = MATS[mat]
            first = Mi.Linear(m, k["mu"], k["nu"], k["rho"], BODY[:dim], k["delta_t"], k["theta"])
            _built[geom] = (lo, hi, perturb, first)
            _refs[key] = first
        else:
            _refs[key] = copy.copy(first)
            _refs[key].m = m
    return _built[geom][:3] + (_refs[key],)


def _fresh(ref, body=True):
    """the cached reference with a zero state of its own, with or without the body force"""
    L = copy.copy(ref)
    L.d, L.d_old, L.v, L.v_old, L.f_old, L.stress = (np.zeros(ref.m.n) for _ in range(6))
    if not body:
        L.body_on, L.body_vec = False, np.zeros(ref.m.n)
    return L


def _context(geom, roles, operator, body=True, lattice=None, slabs=1, solver_type=None):
    """a context of the case, set up for the linear model, and the reference; mesh, constraints and interface must agree"""
    dim, degree, kind, reps, mat = geom
    lo, hi, perturb, ref = _reference(geom, roles)
    k = MATS[mat]
    bf = tuple(BODY[:dim]) + (0.0,) * (3 - dim) if body else (0.0, 0.0, 0.0)
    G = M.Context(dim=dim, degree=degree, reps=reps, lo=lo, hi=hi, face_role=roles, perturb=perturb, body_force=bf,
                  mu=k["mu"], nu=k["nu"], rho=k["rho"], delta_t=k["delta_t"], slabs=slabs)
    m = ref.m
    assert np.array_equal(G.constrained, m.constrained) and np.abs(G.coords - m.coords).max() < 1e-14
    assert np.array_equal(G.interface()[0], m.interface_nodes)
    assert 0 < m.constrained.sum() < m.n
    if lattice is not None:
        G.set_tuning("cell_lattice", lattice)
    if solver_type is not None:
        G.set_tuning("solver_type", solver_type)
    if operator:
        G.set_tuning("linear_operator", operator)
    G.linear_setup(k["theta"])
    assert G.get_tuning("linear_operator_active") == operator
    return G, ref


def _z_only(m):
    """nodes whose z component alone is constrained (FACE_ZCLAMP off the clamped face)"""
    c = m.constrained.reshape(-1, 3)
    return int((c[:, 2] & ~c[:, 0]).sum())


# ------------------------------------------------------------------ operators
def _check_operators(G, ref, seed):
    """K x, M x, A x and the diagonal against the mirror on all rows; each product twice, the same bits; returns the relmax
    per operator and the products"""
    m = ref.m
    cons = m.constrained
    x = np.random.default_rng(seed).standard_normal(m.n)
    assert np.all(x[cons] != 0)
    err, ys = {}, []
    for which, A in ((0, ref.K), (1, ref.M), (2, ref.system_matrix())):
        y = G.linear_apply(which, x)
        err["KMA"[which]] = _relmax(y, A @ x)
        assert np.array_equal(G.linear_apply(which, x), y)  # fixed summation order
        ys.append(y)
    d = G.linear_diagonal()
    err["diag"] = _relmax(d, np.diag(ref.stepping))
    assert np.array_equal(ys[2][cons], d[cons] * x[cons])  # a constrained row of A is its diagonal entry
    ys.append(d)
    return err, ys


# (geometry, reps, roles, material): the case table of test_gpu_q3_smoother_quadrature.py + nine distorted cells in a row
MF_CASES = [
    ("cube", (1, 1, 1), ROLES_A, "a"),
    ("cube", (2, 1, 1), ROLES_B, "b"),
    ("cube", (2, 2, 1), ROLES_A, "c"),
    ("cube", (3, 2, 2), ROLES_B, "a"),
    ("cube", (5, 1, 1), ROLES_A, "b"),
    ("graded", (2, 3, 2), ROLES_B, "c"),
    ("distorted", (2, 1, 2), ROLES_A, "a"),
    ("distorted", (3, 3, 1), ROLES_B, "b"),
    ("distorted", (9, 1, 1), ROLES_A, "c"),
]


@pytest.mark.parametrize("kind,reps,roles,mat", MF_CASES)
def test_matrix_free_operators_against_the_mirror(kind, reps, roles, mat):
    """mf_linear_q3<BOX> + the gathers and mf_linear_diag_q3<BOX> + mf_linear_diag_gather: K x, M x, A x, diag(A) to 1e-12"""
    geom = (3, 3, kind, reps, mat)
    out = {}
    for lattice in (1,) if kind == "cube" else (1, 0):
        G, ref = _context(geom, roles, 1, lattice=lattice)
        assert _z_only(ref.m) > 0
        err, out[lattice] = _check_operators(G, ref, seed=len(ref.m.cells))
        print("matrix-free %s %s nu %.2f lattice %d: relmax" % (kind, reps, MATS[mat]["nu"], lattice),
              {k: "%.1e" % v for k, v in err.items()})
        assert all(e <= TOL for e in err.values()), err
        G.close()
    if 0 in out:  # no cell lattice exists on a Q3 mesh: the key cannot change what runs
        assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))


# (dim, degree, geometry, reps, material), a few cells each, fewest at the highest degree
ASM_CASES = [
    (2, 1, "distorted", (4, 3), "a"),
    (2, 2, "distorted", (3, 3), "b"),
    (2, 2, "graded", (2, 3), "c"),
    (2, 3, "distorted", (3, 2), "c"),
    (2, 4, "distorted", (2, 2), "a"),
    (2, 4, "graded", (2, 1), "b"),
    (3, 1, "distorted", (3, 3, 4), "b"),
    (3, 1, "graded", (2, 3, 2), "c"),
    (3, 2, "distorted", (2, 2, 2), "a"),
    (3, 3, "distorted", (2, 1, 2), "a"),
    (3, 3, "graded", (1, 2, 1), "b"),
]


@pytest.mark.parametrize("geom", ASM_CASES, ids=lambda g: "%dD-Q%d-%s-%s" % (g[0], g[1], g[2], "x".join(map(str, g[3]))))
def test_assembled_operators_against_the_mirror(geom):
    """assemble_linear_cells with the d-linear map: K, M and the constrained stepping matrix entry by entry (nothing of the
    mirror's outside the exported pattern), then the sliced-ELL products and the diagonal as for the matrix-free form"""
    G, ref = _context(geom, ROLES_A, 0)
    if geom[0] == 3:
        assert _z_only(ref.m) > 0
    err = {}
    for which, A in ((0, ref.K), (1, ref.M), (2, ref.system_matrix())):
        C = G.linear_csr(which)
        rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
        outside = np.ones(A.shape, bool)
        outside[rows, C.indices] = False
        assert outside.sum() == A.size - C.nnz  # no entry exported twice
        assert not A[outside].any()
        err["csr " + "KMA"[which]] = np.abs(C.data - A[rows, C.indices]).max() / np.abs(A).max()
    e2, _ = _check_operators(G, ref, seed=len(ref.m.cells))
    err.update(e2)
    print("assembled %dD Q%d %s %s: relmax" % geom[:4], {k: "%.1e" % v for k, v in err.items()})
    assert all(e <= TOL for e in err.values()), err
    G.close()


def _rigid_modes(X):
    """translations and infinitesimal rotations u = w x X of the nodes X[n, 3], as dof vectors"""
    modes = []
    for c in range(3):
        u = np.zeros_like(X)
        u[:, c] = 1.0
        modes.append(u.reshape(-1))
    for a, b in ((0, 1), (1, 2), (2, 0)):
        u = np.zeros_like(X)
        u[:, a], u[:, b] = -X[:, b], X[:, a]
        modes.append(u.reshape(-1))
    return modes


@pytest.mark.parametrize("operator", [0, 1], ids=["assembled", "matrix_free"])
def test_operator_properties_without_a_reference(operator):
    """one distorted Q3 mesh per operator form: K, M, A symmetric in x . (B y) = y . (B x) to 1e-12 of the product's size;
    K on translations and rotations below 1e-12 max|K x| max|X| / max|x| of a random x (the mirror's own K sets that scale
    and is printed on the same modes); 1^T M 1 / 3 as the mirror's"""
    G, ref = _context((3, 3, "distorted", (2, 1, 2), "a"), ROLES_A, operator)
    m = ref.m
    rng = np.random.default_rng(21)
    x, y = rng.standard_normal(m.n), rng.standard_normal(m.n)
    sym = {}
    for which in range(3):
        By, Bx = G.linear_apply(which, y), G.linear_apply(which, x)
        sym["KMA"[which]] = abs(x @ By - y @ Bx) / (np.abs(x) @ np.abs(By))
    scale = np.abs(ref.K @ x).max() * np.abs(m.coords).max() / np.abs(x).max()
    modes = _rigid_modes(m.coords)
    rigid = max(np.abs(G.linear_apply(0, u)).max() for u in modes) / scale
    rigid_mirror = max(np.abs(ref.K @ u).max() for u in modes) / scale
    one = np.ones(m.n)
    mass, mass_ref = one @ G.linear_apply(1, one) / 3, one @ ref.M @ one / 3
    print("operator form %d: asymmetry %s, K on rigid modes %.1e of the scale (mirror %.1e), mass %.15e (mirror %.15e)"
          % (operator, {k: "%.1e" % v for k, v in sym.items()}, rigid, rigid_mirror, mass, mass_ref))
    assert all(s <= TOL for s in sym.values()), sym
    assert rigid <= TOL
    assert abs(mass - mass_ref) <= TOL * mass_ref
    G.close()


# ------------------------------------------------------------------ right-hand side and steps
def _set_stress(L, t):
    ids, dim = L.m.interface_nodes, L.m.dim
    L.stress[:] = 0
    for c in range(dim):
        L.stress[ids * dim + c] = t[:, c]


def _run_steps(G, ref, body, seed, tol_sol=TOL_SOL, banded=False):
    """three steps on the device and in the mirror from the same non-zero state and interface data; worst errors"""
    L = _fresh(ref, body)
    m, dim, dt, th = L.m, L.m.dim, L.dt, L.theta
    ids, free = m.interface_nodes, ~m.constrained
    assert len(ids) > 0
    rng = np.random.default_rng(seed)
    # the state: M v, dt K d and dt (1 - theta) F_n all of size 1 -- and below the new load times dt theta too
    v0, d0, f0 = rng.standard_normal(m.n) * free, rng.standard_normal(m.n) * free, rng.standard_normal(m.n)
    v0 /= np.abs(L.M @ v0).max()
    d0 /= dt * np.abs(L.K @ d0).max()
    f0 /= dt * (1 - th) * np.abs(f0).max()
    L.v[:], L.d[:], L.f_old[:] = v0, d0, f0
    G.set(L_V, v0)
    G.set(L_D, d0)
    G.set(L_F_OLD, f0)
    worst = {"rhs": 0.0, "f_old": 0.0, "d": 0.0, "v": 0.0}
    for step in range(3):
        consistent = step != 1
        t = rng.standard_normal((len(ids), dim))
        _set_stress(L, t)
        t /= dt * th * np.abs(L.consistent_load() if consistent else L.stress).max()
        _set_stress(L, t)
        G.set_interface_traction(t)
        rhs = L.step(consistent)
        scale = np.abs(rhs).max()
        its, res = G.linear_step(consistent, 1e-13 * scale)
        assert res <= 1e-13 * scale and (its == 1) == banded  # (the band solver reports one iteration)
        e = {"rhs": np.abs(G.get(L_RHS) - rhs).max() / scale, "f_old": np.abs(G.get(L_F_OLD) - L.f_old).max() / scale,
             "d": _relmax(G.get(L_D), L.d), "v": _relmax(G.get(L_V), L.v)}
        print("    step %d %s: %s" % (step, "Stress" if consistent else "Force", {k: "%.1e" % v for k, v in e.items()}))
        assert e["rhs"] <= TOL and e["f_old"] <= TOL and e["d"] <= tol_sol and e["v"] <= tol_sol, (step, e)
        worst = {k: max(worst[k], e[k]) for k in e}
        # the next step starts from the device's d and v on both sides: its right-hand side is then compared from the same
        # state, free of what the solve's tolerance left in v (F_n stays each side's own)
        L.d[:], L.v[:] = G.get(L_D), G.get(L_V)
    return worst


MF_STEP_CASES = [("cube", (2, 2, 1), "c"), ("graded", (2, 3, 2), "c"), ("distorted", (2, 1, 2), "a"), ("distorted", (3, 3, 1), "b")]


@pytest.mark.parametrize("body", [True, False], ids=["body_force", "no_body_force"])
@pytest.mark.parametrize("roles", [ROLES_A, ROLES_B], ids=["roles_a", "roles_b"])
@pytest.mark.parametrize("kind,reps,mat", MF_STEP_CASES)
def test_matrix_free_steps_against_the_mirror(kind, reps, mat, roles, body):
    """mi_linear_step on the matrix-free operators: linear_rhs_prepare / linear_rhs_finish around two mf_linear_q3 products,
    the host-built consistent load, the body vector M (b, b, ...), the PCG on A"""
    G, ref = _context((3, 3, kind, reps, mat), roles, 1, body=body)
    worst = _run_steps(G, ref, body, seed=sum(reps) + int(body))
    print("matrix-free steps %s %s: worst" % (kind, reps), {k: "%.1e" % v for k, v in worst.items()})
    G.close()


# (dim, degree, reps, material, slabs, solver_type): distorted cells
ASM_STEP_CASES = [
    (3, 2, (2, 2, 2), "a", 1, None),
    (2, 3, (3, 2), "c", 1, None),
    (2, 3, (3, 2), "c", 1, 1),  # the banded Cholesky route
    (3, 1, (3, 3, 4), "b", 1, None),
    (3, 1, (3, 3, 4), "b", 2, None),  # (the operator hooks do not work on slabs: steps only)
]


@pytest.mark.parametrize("body", [True, False], ids=["body_force", "no_body_force"])
@pytest.mark.parametrize("dim,degree,reps,mat,slabs,solver_type", ASM_STEP_CASES)
def test_assembled_steps_against_the_mirror(dim, degree, reps, mat, slabs, solver_type, body):
    """mi_linear_step on the assembled operators, in 2D and 3D, on one and two slabs, by PCG and by the band solver"""
    G, ref = _context((dim, degree, "distorted", reps, mat), ROLES_A, 0, body=body, slabs=slabs, solver_type=solver_type)
    assert G.comm_info()[0] == slabs
    banded = solver_type == 1
    worst = _run_steps(G, ref, body, seed=sum(reps) + int(body), tol_sol=TOL_BAND if banded else TOL_SOL, banded=banded)
    print("assembled steps %dD Q%d %s slabs %d solver_type %s: worst" % (dim, degree, reps, slabs, solver_type),
          {k: "%.1e" % v for k, v in worst.items()})
    G.close()
