"""CPU: the numpy V-cycle of tests/golden/mg_reference.py, anchored before any GPU test trusts it.

  * the hierarchy shapes of every case of the GPU table against lists written by hand;
  * operator_matrix() against mirror.Operator itself;
  * transfers: prolongation reproduces lattice-linear fields on the free dofs, restriction is its masked transpose, the state
    transfer of a lattice-linear state is that state;
  * with the true lambda_max(D^-1 A) x 1.15 as lmax, B_ref is symmetric to 1e-13 and positive definite and
    rho(I - B_ref A) < 1.  Measured rho: 3D Q2 (3,2,2) 0.286, 3D Q1 (5,4,3) 0.229, 2D Q2 (6,4) 0.230;
  * with an exact coarsest level and many smoother steps on a two-level hierarchy, B_ref A approaches the identity
    (|B A x - x| / |x| = 0.18, 1.3e-3, 2.0e-12 for nu = 2, 8, 30);
  * e_ref, the relmax between the float64 and the long double cycle on a random right-hand side, for every case of the GPU
    table.  Measured worst: 8.98e-16 (case q2_4416_induced); mg_reference.E_REF = 1.0e-15 is what the GPU tolerance rests on;
  * the same for the mid-size cases mg_reference.MID_CASES (level 0 above 10,240 nodes, tests/test_gpu_sell_lds_product.py),
    whose shapes are written by hand too.  Measured: q1_3d 6.22e-16, q2_11 9.04e-16, 2d_q4 8.16e-16 -- within E_REF, so
    these cases take the GPU tolerance of the others.  A case builds its hierarchy in 4 to 30 s and runs the long double
    cycle in under a second;
  * the fp32 opt-ins of the preconditioner (tests/test_gpu_multigrid_fp32.py), on mg_reference.STORAGE_CASES / PRECISION_CASES:
    the storage-32 cycle's own rounding is within E_REF (worst 8.9e-16) and it lies 4.9e-8 .. 1.3e-7 from the storage-64
    cycle; the fp32 emulation of the level-0 products lies at most 5.74e-7 from the fp64 cycle (mg_reference.E32 = 6.0e-7,
    TOL32 = 1e-5); the cycles of the two states that the GPU sequences assemble at lie at least 5.6e-3 apart.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mg_reference as R  # noqa: E402
import mirror as Mi  # noqa: E402

# (degree, reps, dofs, exact) per level, by hand from the rule: p -> 1 on the same cells, then reps -> max(floor, ceil(reps / 2))
# for every reps > floor = min(2, coarsest) until none exceeds coarsest; exact if <= 384 dofs and mg_dense 1
SHAPES = {
    "q2_654": [(2, (6, 5, 4), 3861, 0), (1, (6, 5, 4), 630, 0), (1, (3, 3, 2), 144, 1)],
    "q2_753_mf27": [(2, (7, 5, 3), 3465, 0), (1, (7, 5, 3), 576, 0), (1, (4, 3, 2), 180, 1)],
    "q2_543_mf_fine": [(2, (5, 4, 3), 2079, 0), (1, (5, 4, 3), 360, 0), (1, (3, 2, 2), 108, 1)],
    "q3_532_rule5": [(3, (5, 3, 2), 3360, 0), (1, (5, 3, 2), 216, 0), (1, (3, 2, 2), 108, 1)],
    "q3_532_rule4": [(3, (5, 3, 2), 3360, 0), (1, (5, 3, 2), 216, 0), (1, (3, 2, 2), 108, 1)],
    "q1_987": [(1, (9, 8, 7), 2160, 0), (1, (5, 4, 4), 450, 0), (1, (3, 2, 2), 108, 1)],
    "q2_444_coarsest2": [(2, (4, 4, 4), 2187, 0), (1, (4, 4, 4), 375, 0), (1, (2, 2, 2), 81, 1)],
    "q2_888": [(2, (8, 8, 8), 14739, 0), (1, (8, 8, 8), 2187, 0), (1, (4, 4, 4), 375, 1)],
    "q2_444_polynomial": [(2, (4, 4, 4), 2187, 0), (1, (4, 4, 4), 375, 0), (1, (2, 2, 2), 81, 0), (1, (1, 1, 1), 24, 0)],
    "q2_1231": [(2, (12, 3, 1), 1575, 0), (1, (12, 3, 1), 312, 0), (1, (6, 2, 1), 126, 0), (1, (3, 2, 1), 72, 1)],
    "2d_q2_186": [(2, (18, 6), 962, 0), (1, (18, 6), 266, 0), (1, (9, 3), 80, 0), (1, (5, 2), 36, 0), (1, (3, 2), 24, 1)],
    "2d_q4_64": [(4, (6, 4), 850, 0), (1, (6, 4), 70, 0), (1, (3, 2), 24, 1)],
    "q2_4412_3slabs_z": [(2, (4, 4, 12), 6075, 0), (1, (4, 4, 12), 975, 0), (1, (2, 2, 6), 189, 0), (1, (2, 2, 3), 108, 1)],
    "q2_1244_2slabs_x": [(2, (12, 4, 4), 6075, 0), (1, (12, 4, 4), 975, 0), (1, (6, 2, 2), 189, 0), (1, (3, 2, 2), 108, 1)],
    "q2_4416_induced": [(2, (4, 4, 16), 8019, 0), (1, (4, 4, 16), 1275, 0), (1, (2, 2, 8), 243, 0), (1, (2, 2, 4), 135, 1)],
}


def test_hierarchy_shapes_equal_the_hand_written_lists():
    assert sorted(SHAPES) == sorted(R.CASES)
    for name, c in R.CASES.items():
        h = R.hierarchy(c["dim"], c["p"], c["reps"], c.get("coarsest", 4), c.get("dense", 1))
        assert [(l["degree"], l["reps"], l["n_dofs"], l["exact"]) for l in h] == SHAPES[name], name
        for i, l in enumerate(h):
            last = i + 1 == len(h)
            want = (0, 0.0) if l["exact"] else (12, 60.0) if last else (3 if i == 0 else 2, 20.0)
            assert (l["nu"], l["ratio"]) == want
    # the hierarchy-rebuild test's shapes of case 1
    assert [l["reps"] for l in R.hierarchy(3, 2, (6, 5, 4), 2, 1)] == [(6, 5, 4), (6, 5, 4), (3, 3, 2), (2, 2, 2)]
    assert [(l["exact"], l["nu"]) for l in R.hierarchy(3, 2, (6, 5, 4), 4, 0)] == [(0, 3), (0, 2), (0, 12)]


MID_SHAPES = {
    "q1_3d": [(1, (22, 21, 21), 33396, 0), (1, (11, 11, 11), 5184, 0), (1, (6, 6, 6), 1029, 0), (1, (3, 3, 3), 192, 1)],
    "q2_11": [(2, (11, 11, 11), 36501, 0), (1, (11, 11, 11), 5184, 0), (1, (6, 6, 6), 1029, 0), (1, (3, 3, 3), 192, 1)],
    "2d_q4": [(4, (26, 25), 21210, 0), (1, (26, 25), 1404, 0), (1, (13, 13), 392, 0), (1, (7, 7), 128, 0), (1, (4, 4), 50, 1)],
}


def test_mid_case_shapes_equal_the_hand_written_lists():
    assert sorted(MID_SHAPES) == sorted(R.MID_CASES) and not set(R.MID_CASES) & set(R.CASES)
    for name, c in R.MID_CASES.items():
        h = R.hierarchy(c["dim"], c["p"], c["reps"])
        assert [(l["degree"], l["reps"], l["n_dofs"], l["exact"]) for l in h] == MID_SHAPES[name], name
        assert h[0]["n_dofs"] // c["dim"] > 160 * 64  # more than SELL_SPLIT_MAX_SLICES slices of 64 rows on level 0
        lo, hi, perturb = R.geometry(c["kind"], c["dim"], c["reps"], seed=sum(c["reps"]))
        assert np.allclose(hi, 0.1 * np.array(c["reps"])) and 0.004 < perturb.std() < 0.006  # 5 % of the cell size


SMALL = [(3, 2, (3, 2, 2), R.ROLES_A), (3, 1, (5, 4, 3), R.ROLES_B), (2, 2, (6, 4), R.ROLES_2D)]


def _small(dim, p, reps, roles, **kw):
    hi = tuple(0.1 * r for r in reps)
    m = Mi.Mesh(dim, p, reps, (0.0,) * dim, hi, roles)
    u, du = R.case_state(m, seed=3)
    return m, R.Reference(m, u + du, alpha1=R.A1, **kw)


def test_operator_matrix_is_the_mirror_operator():
    """the level matrices are mirror.Operator: column by column on a small mesh, on random vectors at every rule in use"""
    m = Mi.Mesh(3, 1, (2, 2, 1), (0, 0, 0), (0.2, 0.2, 0.1), R.ROLES_A)
    u, du = R.case_state(m, seed=1)
    op = Mi.Operator(m, u + du, alpha1=R.A1)
    A, B = R.operator_matrix(op), R.operator_matrix_by_unit_vectors(op)
    assert abs(A - B).max() <= 1e-14 * abs(B).max()
    rng = np.random.default_rng(0)
    for dim, p, reps, roles, nq, fold in [(3, 2, (2, 2, 1), R.ROLES_B, 3, True), (3, 2, (2, 1, 2), R.ROLES_A, None, False),
                                          (3, 3, (2, 1, 1), R.ROLES_A, 4, True), (2, 4, (2, 2), R.ROLES_2D, None, False)]:
        m = Mi.Mesh(dim, p, reps, (0.0,) * dim, tuple(0.1 * r for r in reps), roles)
        u, du = R.case_state(m, seed=2)
        op = Mi.Operator(m, u + du, alpha1=R.A1, nq=nq, fold_to_identity=fold)
        x = rng.standard_normal(m.n)
        y = op(x)
        assert np.abs(R.operator_matrix(op) @ x - y).max() <= 1e-13 * np.abs(y).max()


def test_transfers_reproduce_lattice_linear_fields():
    for nf, nc in [((8, 5, 3), (5, 3, 2)), ((16, 10, 7), (6, 4, 3)), ((13, 11, 9), (7, 6, 5)), ((37, 13), (19, 7))]:
        dim = len(nf)
        rng = np.random.default_rng(sum(nf))
        cf, cc = rng.random(int(np.prod(nf)) * dim) < 0.2, rng.random(int(np.prod(nc)) * dim) < 0.2
        t = R.Transfer(dim, nf, nc, cf, cc)

        def linear(nn, coef):  # a field linear in t_d / (n_d - 1), per component
            idx = np.stack(np.unravel_index(np.arange(int(np.prod(nn))), nn[::-1]), -1)[:, ::-1]
            s = idx / (np.array(nn) - 1.0)
            return (coef[0] + s @ coef[1:]).reshape(-1)

        coef = rng.standard_normal((dim + 1, dim))
        ff, fc = linear(nf, coef), linear(nc, coef)
        assert np.abs(t.prolong(fc) - ff * ~cf).max() <= 1e-14 * np.abs(ff).max()
        assert np.abs(t.state(ff) - fc * ~cc).max() <= 1e-14 * np.abs(fc).max()
        # restriction = masked transpose: (R r, x) = (r, P x) for x supported on the free coarse dofs
        r, x = rng.standard_normal(len(ff)), rng.standard_normal(len(fc)) * ~cc
        assert abs(t.restrict(r) @ x - r @ t.prolong(x)) <= 1e-13 * abs(r @ t.prolong(x))
        assert np.all(t.restrict(r)[cc] == 0) and np.all(t.prolong(x)[cf] == 0)
    # non-nested lattices have weights other than 0, 1/2, 1
    assert sorted(set(np.round(R.interp_1d(8, 5)[1], 12))) == [0.0, round(3 / 7, 12), round(4 / 7, 12)]


@pytest.mark.parametrize("dim,p,reps,roles", SMALL)
def test_reference_cycle_is_symmetric_positive_and_contracts(dim, p, reps, roles):
    m, ref = _small(dim, p, reps, roles)
    assert len(ref.shape) >= 2
    lmax = ref.true_lmax()
    free = np.nonzero(~m.constrained)[0]
    B = np.stack([ref.vcycle(np.eye(m.n)[:, j], lmax) for j in free], -1)[free]
    assert np.abs(B - B.T).max() <= 1e-13 * np.abs(B).max()
    B = 0.5 * (B + B.T)
    assert np.linalg.eigvalsh(B)[0] > 0
    A = ref.A[0].toarray()[np.ix_(free, free)]
    rho = np.abs(np.linalg.eigvals(np.eye(len(free)) - B @ A)).max()
    print("rho(I - B_ref A) for dim %d Q%d %s: %.3f" % (dim, p, reps, rho))
    assert rho < 1


def test_two_level_cycle_with_many_smoother_steps_approaches_the_inverse():
    m, ref = _small(3, 1, (4, 3, 2), R.ROLES_A, coarsest=2)
    assert len(ref.shape) == 2 and ref.shape[-1]["exact"]
    lmax = ref.true_lmax()
    free = ~m.constrained
    x = np.random.default_rng(1).standard_normal(m.n) * free
    err = []
    for nu in (2, 8, 30):
        err.append(np.abs(ref.vcycle(ref.A[0] @ x, lmax, nu=nu) - x).max() / np.abs(x).max())
    print("two-level |B A x - x| / |x| for nu = 2, 8, 30:", err)
    assert err[0] > err[1] > err[2] and err[2] < 1e-6


def _e_ref(name):
    m = R.case_mesh(name)[0]
    u, du = R.case_state(m, seed=len(name))
    ref = R.case_reference(name, u + du, m)
    lmax = ref.true_lmax()
    r = np.random.default_rng(5).standard_normal(m.n) * ~m.constrained
    z, zl = ref.vcycle(r, lmax), ref.vcycle(r, lmax, np.longdouble)
    e = float(np.abs(z - zl).max() / np.abs(zl).max())
    print("e_ref %-20s %.2e" % (name, e))
    return e


def test_reference_rounding_on_the_gpu_cases():
    """e_ref per case of the GPU table: float64 against long double cycle, random right-hand side, true lmax x 1.15"""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = 0.0
    for name in R.CASES:
        e = _e_ref(name)
        assert e <= R.E_REF, (name, e)  # (each on its own: a NaN fails)
        worst = max(worst, e)
    print("worst e_ref %.3e" % worst)
    assert worst <= R.E_REF


@pytest.mark.parametrize("name", sorted(R.MID_CASES))
def test_reference_rounding_on_the_mid_cases(name):
    """the same on a mid-size case: within E_REF, so the GPU tolerance of the small cases holds for it"""
    assert np.finfo(np.longdouble).eps < 1e-18
    assert _e_ref(name) <= R.E_REF


# ------------------------------------------------------------------ the fp32 opt-ins of the preconditioner
TOL_GPU = min(1e-10, 10.0 ** math.ceil(math.log10(64 * R.E_REF)))  # TOL of tests/test_gpu_multigrid_reference.py


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _assembled(name, second=False):
    """(mesh, reference with the assembly-rule fine operator, true lmax x 1.15) of a case at its state / at its second state"""
    m = R.case_mesh(name)[0]
    u, du = R.case_state(m, seed=len(name))
    if second:
        du = R.second_increment(m, du)
    ref = R.assembled_reference(name, u + du, m)
    return m, ref, ref.true_lmax()


@pytest.mark.parametrize("name", R.STORAGE_CASES)
def test_storage32_reference_rounding_and_distance(name):
    """"precond_storage" 32 in the reference: fp64 arithmetic on fp32-rounded product matrices (here the mirror's own,
    rounded: no device).  Its rounding, float64 against long double cycle, is within E_REF, so the GPU tolerance stays 1e-13;
    and the key is visible: the storage-32 cycle lies at least 1e3 tolerances from the storage-64 one.
    Measured e_ref / distance: q2_654 4.9e-16 / 6.9e-8, q1_987 4.1e-16 / 4.9e-8, 2d_q4_64 7.4e-16 / 1.3e-7, q3_532_assembled
    6.6e-16 / 7.9e-8, q2_753_mf27 5.9e-16 / 9.3e-8, q2_4412_3slabs_z 8.9e-16 / 1.2e-7, q2_11 8.2e-16 / 1.1e-7."""
    assert np.finfo(np.longdouble).eps < 1e-18
    m, ref, lmax = _assembled(name)
    r = np.random.default_rng(5).standard_normal(m.n) * ~m.constrained
    z32, z32l = ref.vcycle(r, lmax, storage=32), ref.vcycle(r, lmax, np.longdouble, storage=32)
    e = _relmax(z32, z32l)
    d = _relmax(z32, ref.vcycle(r, lmax))
    print("storage 32 %-20s e_ref %.2e  distance to storage 64 %.2e" % (name, e, d))
    assert e <= R.E_REF, (name, e)
    assert d >= 1e3 * TOL_GPU, (name, d)
    # D^-1 and the dense inverse stay fp64: rounding them too gives another cycle
    Ls = ref.levels(np.float64, 32)[0]
    assert Ls[0].Dinv.astype(np.float32).astype(np.float64).tolist() != Ls[0].Dinv.tolist()
    assert np.array_equal(Ls[-1].dense(), ref.levels(np.float64)[0][-1].dense())
    # product_matrices: the same matrices handed in are the same cycle, to the bit
    assert np.array_equal(ref.vcycle(r, lmax, storage=32, product_matrices=[A.copy() for A in ref.A]), z32)
    # the eigenvalue the estimate is bounded by moves with the values
    l = len(ref.shape) - 2
    lam, lam32 = ref.lambda_true(l), ref.lambda_true(l, storage=32)
    print("level %d lambda_true %.12f, storage 32 %.12f" % (l, lam, lam32))
    assert lam32 != lam and abs(lam32 - lam) < 1e-6 * lam


@pytest.mark.parametrize("name", R.PRECISION_CASES)
def test_fp32_emulation_distance_is_within_E32(name):
    """"smoother_precision" 32: the fp64 reference cycle against the cycle whose level-0 products run in the fp32 emulation,
    three right-hand sides, both accumulation orders.  Measured worst: q2_543_mf_fine 4.80e-7, q2_654 5.74e-7,
    q2_4412_3slabs_z 4.84e-7 (all figures 1.4e-7 .. 5.7e-7); mg_reference.E32 is what the GPU tolerance rests on."""
    m, ref, lmax = _assembled(name)
    worst = 0.0
    for what, r in R.cpu_rhs_set(m):
        z = ref.vcycle(r, lmax)
        za, zb = ref.vcycle(r, lmax, product0="f32"), ref.vcycle(r, lmax, product0="f32r")
        assert not np.array_equal(za, zb)  # two orders of one sum: two roundings
        for order, zz in (("stored", za), ("reverse", zb)):
            e = _relmax(zz, z)
            print("fp32 emulation %-18s %-7s %-7s relmax %.2e" % (name, what, order, e))
            assert 1e-10 < e <= R.E32, (name, what, order, e)
            worst = max(worst, e)
    print("worst fp32 emulation distance %-18s %.2e (E32 %.1e, TOL32 %.0e)" % (name, worst, R.E32, R.tol32()))
    assert R.tol32() <= 1e-4 and 16 * R.E32 <= R.tol32() < 160 * R.E32


@pytest.mark.parametrize("name", ["q2_543_mf_fine", "q2_654"])
def test_cycle_of_the_other_tangent_is_far_from_the_tolerance(name):
    """the tests that re-assemble at a changed state tell fresh from stale: the reference cycles at the two states lie at
    least 100 x TOL32 (and so far more than 100 x the storage tolerance) apart.  Measured, smallest of three
    right-hand sides: q2_543_mf_fine 6.4e-3, q2_654 5.6e-3 (the unit vector; 1.2e-2 .. 2.7e-2 on the others)."""
    m, ref, lmax = _assembled(name)
    _, ref2, lmax2 = _assembled(name, second=True)
    for what, r in R.cpu_rhs_set(m):
        d = _relmax(ref2.vcycle(r, lmax2), ref.vcycle(r, lmax))
        d_op = _relmax(ref2.vcycle(r, lmax), ref.vcycle(r, lmax))  # (the same lmax: the operators alone)
        print("second state %-18s %-7s relmax %.2e (same lmax: %.2e)" % (name, what, d, d_op))
        assert d >= 100 * R.tol32() and d_op >= 100 * R.tol32(), (name, what, d, d_op)
