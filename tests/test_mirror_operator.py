"""CPU: the matrix-free operator of tests/golden/mirror.py (mirror.Operator) that the GPU tests of the smoother's product
(test_gpu_smoother_operator.py) compare against -- checked here against the oracle's assembled matrix, against the
mirror's own dense cell tangent at other quadrature rules, and for its fold rule."""
import os
import sys

import numpy as np

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402

ROLES = [O.FACE_CLAMPED, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_ZCLAMP, O.FACE_INTERFACE]
A1 = 1.0 / (0.25 * 0.005**2)  # alpha_1 of the default Newmark parameters


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _shear(X):
    """a smooth large deformation with shear (F != F^T, J != 1, |F - I| up to about 0.5) that vanishes on x = min x and
    has u_z = 0 on both z faces: no jump where the clamped and z-clamped dofs are masked"""
    L = np.ptp(X, axis=0).max()
    s = (X - X.min(axis=0)) / L
    tz = np.ptp(s[:, 2])
    u = np.zeros_like(X)
    u[:, 0] = s[:, 0] * (0.3 * s[:, 1] + 0.2 * s[:, 2])
    u[:, 1] = s[:, 0] * (0.25 + 0.3 * s[:, 2] ** 2)
    u[:, 2] = s[:, 0] * s[:, 2] * (tz - s[:, 2]) * (0.6 * np.sin(3.0 * s[:, 1]) - 0.5)
    return L * u.reshape(-1)


def _folded(X, ny):
    """u_x = -1.05 x M(eta), M = 4 eta (1 - eta), eta the cell-local y: det F = 1 - 1.05 M < 0 at eta = 0.5 only"""
    eta = (X[:, 1] * ny) % 1.0
    u = np.zeros_like(X)
    u[:, 0] = -1.05 * X[:, 0] * 4.0 * eta * (1.0 - eta)
    return u.reshape(-1)


def test_operator_reproduces_the_oracle_assembled_product():
    """nq = p + 2: the assembled tangent of the oracle (C++) on a distorted, deformed, partly clamped 3D Q2 mesh, constrained
    rows and their |K_e(i,i)| diagonal included, to 1e-12"""
    reps, lo, hi = (3, 2, 2), (0.0, 0.0, 0.0), (0.3, 0.25, 0.15)
    rng = np.random.default_rng(41)
    perturb = 0.008 * rng.standard_normal((int(np.prod([r + 1 for r in reps])), 3))
    P = O.Problem(O.make_desc(dim=3, degree=2, reps=reps, lo=lo, hi=hi, face_role=ROLES), perturb)
    m = Mi.Mesh(3, 2, reps, lo, hi, ROLES, perturb=perturb)
    assert np.abs(m.coords - P.coords).max() < 1e-15 and np.array_equal(m.constrained, P.constrained)
    assert 0 < m.constrained.sum() < m.n
    u = _shear(m.coords) * ~m.constrained
    du = 1e-3 * rng.standard_normal(m.n) * ~m.constrained
    P.vec(O.V_U)[:] = u
    P.vec(O.V_DELTA)[:] = du
    P.update_acceleration()
    P.assemble()
    K = P.csr()
    op = Mi.Operator(m, u + du, alpha1=A1)
    for _ in range(2):
        x = rng.standard_normal(m.n)
        assert _relmax(op(x), K @ x) < 1e-12
    assert _relmax(Mi.Operator(m, u + du, alpha1=A1, nq=3)(x), K @ x) > 1e-6


def test_operator_is_the_sum_of_the_dense_cell_tangents_at_any_rule():
    """y = sum_e K_e(nq) x_e with the mirror's dense cell() at nq = 3 and 4 (no constrained dofs: the plain sum)"""
    reps, lo, hi = (2, 1, 1), (0.0, 0.0, 0.0), (0.2, 0.12, 0.07)
    rng = np.random.default_rng(42)
    perturb = 0.006 * rng.standard_normal((12, 3))
    m = Mi.Mesh(3, 2, reps, lo, hi, [O.FACE_INTERFACE] * 6, perturb=perturb)
    u = _shear(m.coords)
    x = rng.standard_normal(m.n)
    for nq in (3, 4):
        y = np.zeros(m.n)
        for conn, verts, _ in m.cells:
            d = m.dofs(conn)
            Ke, _ = Mi.cell(3, 2, verts, u[d], np.zeros(len(d)), 0.5e6, 0.4, 1000.0, A1, (0, 0, 0), nq=nq)
            y[d] += Ke @ x[d]
        assert _relmax(Mi.Operator(m, u, alpha1=A1, nq=nq)(x), y) < 1e-12


def test_the_two_rules_agree_on_undeformed_boxes_and_differ_on_a_deformed_state():
    """undeformed boxes (non-cubic cells): every integrand is a polynomial the 3-point rule integrates exactly, so the
    27- and 64-point operators agree to rounding; on the sheared state they differ by far more than the 1e-12 the GPU
    tests hold the kernels to -- that comparison can tell the rules apart"""
    reps, lo, hi = (2, 3, 2), (0.0, 0.0, 0.0), (0.2, 0.45, 0.1)
    m = Mi.Mesh(3, 2, reps, lo, hi, ROLES)
    x = np.random.default_rng(43).standard_normal(m.n)
    z = np.zeros(m.n)
    assert _relmax(Mi.Operator(m, z, alpha1=A1, nq=3)(x), Mi.Operator(m, z, alpha1=A1, nq=4)(x)) < 1e-13
    u = _shear(m.coords) * ~m.constrained
    assert _relmax(Mi.Operator(m, u, alpha1=A1, nq=3)(x), Mi.Operator(m, u, alpha1=A1, nq=4)(x)) > 1e-6


def test_fold_to_identity_changes_exactly_the_folded_points():
    """fold_to_identity: the points with det F <= 0 -- and only those -- take the undeformed state (their data are those
    of u = 0, every other point's are those of the plain rule, bit for bit); cell() with the same flag agrees"""
    reps = (1, 3, 1)
    m = Mi.Mesh(3, 2, reps, (0, 0, 0), (0.3, 0.9, 0.2), [O.FACE_INTERFACE] * 6)
    u = _folded(m.coords, reps[1] / 0.9)
    with np.errstate(invalid="ignore"):  # (J^(-2/3) of a negative J)
        plain = Mi.Operator(m, u, alpha1=A1, nq=3)
    fold = Mi.Operator(m, u, alpha1=A1, nq=3, fold_to_identity=True)
    zero = Mi.Operator(m, np.zeros(m.n), alpha1=A1, nq=3)
    f = fold.folded
    assert np.array_equal(f, plain.detF <= 0) and np.array_equal(fold.detF, plain.detF)
    assert 0 < f.sum() < f.size and not plain.folded.any()
    for name in ("g", "tau", "Jc"):
        a, b, c = getattr(fold, name), getattr(plain, name), getattr(zero, name)
        assert np.array_equal(a[~f], b[~f]) and np.array_equal(a[f], c[f])
    x = np.random.default_rng(44).standard_normal(m.n)
    y = np.zeros(m.n)
    for conn, verts, _ in m.cells:
        d = m.dofs(conn)
        Ke, _ = Mi.cell(3, 2, verts, u[d], np.zeros(len(d)), 0.5e6, 0.4, 1000.0, A1, (0, 0, 0), nq=3,
                        fold_to_identity=True)
        y[d] += Ke @ x[d]
    assert _relmax(fold(x), y) < 1e-12
    assert not np.isfinite(plain(x)).all()
    # the default rule does not fold on this state (the assembly's points miss eta = 0.5)
    assert not (Mi.Operator(m, u, alpha1=A1).detF <= 0).any()
