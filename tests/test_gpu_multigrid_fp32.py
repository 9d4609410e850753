"""GPU: the two fp32 opt-ins of the preconditioner, "precond_storage" 32 and "smoother_precision" 32, through the V-cycle
against the numpy reference (tests/golden/mg_reference.py).

Why: a preconditioner that is wrong still converges.  A stale fp32 copy, a level that silently stays on fp64, a fused fp32
Chebyshev epilogue with a wrong coefficient, fp32 point records of the previous tangent: the solve reaches the same solution
within an iteration or two, which is all the earlier tests of these keys asserted.  Here z = M^-1 r (mi_spmv under
"spmv_as_smoother" 2) is compared with the reference cycle of the same opt-in, and the read-backs "precond_storage",
"precond_storage_levels" and "smoother_precision_active" assert that the path each test names is the one that ran.
Protocol, helpers and right-hand sides are those of test_gpu_multigrid_reference.py (imported); the numpy hierarchies are
shared with it, so a case costs no second build.

STORAGE 32 -- which operand reads which array (mi_ctx.cpp / mi_mg.cpp, by reading):
  every product of a cycle (smoother steps, the cycle's residual, the power and Krylov eigenvalue estimates) goes through
  level_spmv -> enqueue_spmv(smoother = true) and reads SellParams::vals32 = d_sell_vals32, the copy that refresh_vals32
  makes of d_vals with float(v) before the first product after an assembly; the arithmetic is fp64;
  D^-1 (extract_dinv_blk) and the coarsest level's dense inverse (launch_dense_inverse_from_sell on sell_params without
  vals32) read d_vals, fp64; so do the CG's own product and residual (smoother = false); the transfers read no matrix.
The reference models exactly that: Reference.vcycle(storage=32, product_matrices=...) multiplies with
astype(float32).astype(float64) of the product matrices and takes D and the dense inverse from the unrounded matrices.  The
product matrices are the DEVICE's own fp64 exports (mi_mg_level_context(l) -> csr, each held to the mirror at 1e-12 in the same
test), not the mirror's: rounding is discontinuous, device and mirror agree to 3e-15 of the largest entry, and one entry of
5e5 that rounds to the other fp32 neighbour moves the cycle by far more than the tolerance.  float(v) and astype(float32) are
both round-to-nearest-even, so both sides round the same bits.
Tolerance: TOL = 1e-13 of the fp64 tests.  The storage-32 reference's own rounding (float64 against long double cycle,
tests/test_mirror_multigrid.py) is 4.1e-16 .. 8.9e-16 on these cases, within E_REF = 1.0e-15, so 64 x E_REF rounded up holds.
lmax is bounded against lambda_max(D^-1 A_32) of the same exports: lmax / lambda = 1.150000 on every first estimate, and the
eigenvalue moves by 1e-9 relative under the rounding, which the upper bound 1.15 (1 + 1e-10) would notice.

  case (mg_reference)            what it forces
  q2_654                         fused steps on sell_spmv_split<F32, CHEB> on every level
  q2_654, "mg_fuse" 0            plain F32 product, then cheb_step_blk
  q1_987                         3D Q1
  2d_q4_64                       2D
  q3_532_assembled               3D Q3, fine level assembled (FP32_CASES)
  q2_753_mf27                    "element_tangents" 2: the matrix-free smoother gives way to the fp32 matrix
  q2_11 (MID_CASES)              level 0 on sell_spmv<F32, CHEB> (12,167 nodes; "spmv_lds_launches" of its level context)
  q2_4412_3slabs_z               three slabs; product matrices of an undecomposed twin, whose level-0 diagonal blocks are
                                 the team's to the bit (asserted; the precondition holds on this mesh)
  sequences on q2_654            the key before "precond" 1; after the first solve; 32 -> 64 -> 32 (the middle state is the
                                 storage-64 reference at TOL); a second solve at a changed state under "mg_lag" 1 (level 0 from
                                 the new exports, the levels below from the old) and under "mg_lag" 0; "mg_coarsest" 2 with
                                 storage 32 left on
  four meshes under 160 slices   the small-launch kernel's plain F32 product row by row against
  3D Q2 (4,3,3), Q1 (5,4,4),     spmv_reference.product(f32=True) of the export, a-priori bound, no margin (part (e) of
  Q4 (2,2,2), 2D Q3 (6,5)        test_gpu_sell_lds_product.py, on the other kernel)
  PCG on q2_654                  cg_solve(0, k), k = 1, 2, 3, and one converged run at the first tau of its V-cycle table
                                 against pcg_reference.pcg with the storage-32 cycle, at tol_x / tol_r, margin condition and
                                 the exact iteration count asserted; x_3 lies > 1e3 tol_x from the fp64-stored run
  linear model                   its hierarchy multiplies with fp64 values by design: mi_linear_apply(3) bitwise unchanged
Every cycle comparison also asserts relmax >= 1e-9 to the storage-64 reference cycle (the key took effect) and that two
applications give the same bits.

PRECISION 32 -- launch_mf_spmv selects mf_spmv<true, true, true, 0, float>: fp32 arithmetic on fp32 point records, level 0
only, 64-point rule, production shape only (3D Q2, box cells, lattice ids, cell-major slots).  numpy cannot reproduce the
kernel's arithmetic, so this path has a tolerance measured on the reference: E32 = 6.0e-7, the worst relmax (5.74e-7) between
the fp64 reference cycle and the cycle whose level-0 products run in an fp32 emulation (values and operand cast to float32,
np.add.at in float32, two accumulation orders), over the three cases and three right-hand sides
(tests/test_mirror_multigrid.py).  TOL32 = 16 x E32 rounded up to a power of ten = 1e-5: the kernel rounds point records and
sums in a sum-factorised order, the emulation rounds matrix entries and sums in row order.  The reference is the fp64 cycle
with the assembly-rule fine operator (the library reports rule 4 on this path); z must lie within TOL32 of it and farther
than 1e-10 (fp32 arithmetic ran); lmax bounds are widened by TOL32 on level 0 only; levels >= 1 keep their parts at 1e-12.
  q2_543_mf_fine                 graded mesh, "fine_level" 1
  q2_654, "element_tangents" 2   assembled fine level, matrix-free smoother
  q2_4412_3slabs_z, the same     the layered launches of "mf_halo_overlap"
  q2_753_mf27 + the key          distorted cells: no float instantiation, "smoother_precision_active" 64, z equals the fp64
                                 reference of the rule that "smoother_quadrature_active" reports, at TOL
  sequences on the graded case   key set after an assembly (active 64 and the reported rule's reference at TOL until the next
                                 assembly, 32 after it); a residual pass in between changes nothing, to the bit; re-assembly at
                                 a changed state (the cycles of the two states lie >= 5.6e-3 apart, asserted on the CPU: stale
                                 records fail); 32 -> 64 without an assembly (the reported rule, TOL) and 32 again (still fp64,
                                 same bits, until the next assembly); "mf_diag_lag" 1 over two tangents (fp32 records of the
                                 second tangent, D and coarse operators of the first)

Measured on an MI355X, worst relmax:
  storage 32, cases: q2_654 1.0e-15 (both forms), q1_987 6.5e-16, 2d_q4_64 1.2e-15, q3_532_assembled 1.1e-15, q2_753_mf27
    1.1e-15, q2_11 1.5e-15, slabs 8.5e-16; sequences 1.0e-15 .. 1.4e-15; distance to the storage-64 cycle 2.5e-8 .. 7.6e-8
  small-launch product, worst |y - y_ref| / bound: 0.020, 0.036, 0.007, 0.051;  PCG: x 2.8e-15, res 6.9e-15 (tolerance 1e-12)
  precision 32, cases: q2_543_mf_fine 2.0e-7, q2_654 2.1e-7, slabs 1.5e-7; sequences 1.4e-7 .. 2.0e-7 (tolerance 1e-5)
Run time: 24 tests in 34 s; q2_11 takes 14.3 s, of which 12 s build the numpy hierarchy it shares with
test_gpu_sell_lds_product.py; every other test takes at most 2.7 s.

The ordering defect -- CONFIRMED AND FIXED.  set_precond_storage forwarded the key to the levels that existed at that moment,
and mg_build_levels created level contexts with the default 64: with the key before "precond" 1 (the order of
_context() for every key of a case) or before a rebuild by a shape key, level 0 multiplied with the fp32 copy and the
levels below with fp64.  On the library without the fix, q2_654 with the key first: "precond_storage_levels" 1 of 3, and
z misses the storage-32 reference by 4.4e-9 (random), 1.9e-8 (the solve's right-hand side) and 1.3e-9 (unit vector) against a
tolerance of 1e-13, while it meets the hybrid "level 0 fp32, levels >= 1 fp64" at 1.9e-15.  mg_setup now hands the fine
context's storage to the levels it has built (array allocated, copy marked stale); the linear model's hierarchy is built by
another caller and stays fp64.

Shown to fail (each change made in a scratch copy of the library, a flag or the choice between two valid arrays, no address
moved; run once, never committed; with the first assertion that fails in each test):
  the fix taken out again                          4: "precond_storage_levels" 1 of 3 (key before "precond", lagged levels,
                                                   PCG), 1 of 4 after "mg_coarsest" 2
  assembly no longer marks the fp32 copy stale     1: the lagged-levels sequence, cycle relmax 3.0e-2 after the second solve
  (refresh_vals32 skipped after a re-assembly)
  vals32 dropped for CHEB launches of              12: cycle relmax 5.7e-8 .. 2.5e-7 on every small case and sequence, 2.3e-9 on
  sell_spmv_split alone (in enqueue_spmv, where    q2_11 (only its levels >= 1 run that kernel), x_1 of the PCG 7.3e-8; q2_654
  the launch is chosen)                            under "mg_fuse" 0 passes, as it must
  mg_set_storage starting at level 2               13: "precond_storage_levels" 2 of 3 in every cycle test
  qrec32_valid left true across                    none at first, a finding: the reset is conservative -- records that were
  set_tuning("smoother_precision", 32)             valid still belong to the current tangent, and a first use of the key finds
                                                   the flag false from the last assembly.  What the reset does keep is the
                                                   documented "takes effect with the next tangent assembly"; the last step of
                                                   the graded sequence (32 -> 64 -> 32: active 64, same bits) was added for
                                                   it and fails under the change: active 32
  mf_spmv<float> taking the fp64 records           not run, and no assertion can exist: assemble_q2sf writes both arrays
                                                   from the same registers, qrec32[i] = float(qrec[i]), whenever
                                                   qrec32_valid holds, so the float kernel would convert the same values to
                                                   the same bits
"""
import functools
import os
import sys
import time

import numpy as np
import pytest

import test_gpu_multigrid_reference as TM
import test_gpu_parity as TP
import test_gpu_sell_lds_product as TS
from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mg_reference as R  # noqa: E402
import pcg_reference as PR  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

TOL = TM.TOL  # storage 32: all arithmetic fp64 on the same fp32 bits -- the fp64 tests' tolerance (mg_reference.STORAGE_CASES)
TOL32 = R.tol32()  # precision 32: 16 x E32 rounded up to a power of ten
_relmax = TM._relmax


# ------------------------------------------------------------------ references and read-backs
@functools.lru_cache(maxsize=None)
def _reference(name, variant=""):
    """the hierarchy with the assembly-rule fine operator at the case's state (shared with the fp64 tests where that is the
    case's own reference); variant "second": at u + second_increment(du), every level; "lagged": level 0 there, levels >= 1
    from u + du; "coarsest2": the shape after "mg_coarsest" 2"""
    m, _, _, _, u, du = TM._inputs(name)
    if variant == "":
        if name in R.MID_CASES:
            return TS._mid_reference(name)
        return TM._reference(name) if R.case(name).get("nq0") is None else R.assembled_reference(name, u + du, m)
    if variant == "coarsest2":
        assert R.case(name).get("nq0") is None
        return TM._reference(name, "coarsest2")
    u2 = u + R.second_increment(m, du)
    return R.assembled_reference(name, u2, m, **(dict(coarse_from=u + du) if variant == "lagged" else {}))


def _second(name):
    m, _, _, _, u, du = TM._inputs(name)
    return R.second_increment(m, du)


def _exports(G):
    """the device's own fp64 level matrices: what its fp32 copies are rounded from"""
    out = []
    for l in range(G.mg_n_levels()):
        V = G.mg_level_context(l)
        out.append(V.csr())
        V.close()
    return out


def _assert_storage(G, bits, team=False):
    """every level of the hierarchy multiplies its cycle products with the copy of `bits`"""
    nl = G.mg_n_levels()
    assert G.get_tuning("precond_storage") == bits
    assert G.get_tuning("precond_storage_levels") == (nl if bits == 32 else 0), (G.get_tuning("precond_storage_levels"), nl)
    if bits == 32:
        assert G.get_tuning("smoother_operator_active") == 0  # the assembled matrix, whatever "element_tangents" says
    if not team:
        for l in range(nl):
            V = G.mg_level_context(l)
            assert V.get_tuning("precond_storage") == bits, (l, V.get_tuning("precond_storage"))
            V.close()


def _hold_storage32(G, name, ref, tag, bounds="first", mats=None, team=False, parts=True, seed=0):
    """read-backs, (b) of the fp64 tests against the mirror, lmax against the eigenvalue of D^-1 A_32, and z = M^-1 r against
    the storage-32 reference on the exports' bits; returns (worst relmax, smallest distance to the storage-64 cycle)"""
    m = TM._inputs(name)[0]
    _assert_storage(G, 32, team)
    if not team:
        if parts:
            TM._check_parts(G, ref)
        mats = _exports(G)
    lam32 = lambda l: ref.lambda_true(l, storage=32, product_matrices=mats)  # noqa: E731
    lmax = TM._check_shape_and_estimates(G, ref, distributed=TM.TEAMS[name] if team else None, bounds=bounds, lambda_true=lam32)
    worst, nearest = 0.0, np.inf
    for what, r in TM._rhs_set(G, m, seed):
        z = TM._minv(G, r)
        z_ref = ref.vcycle(r, lmax, storage=32, product_matrices=mats)
        e, d = _relmax(z, z_ref), _relmax(z, ref.vcycle(r, lmax))
        print("V-cycle storage 32 %s, %s: relmax %.2e (tolerance %.0e), to the storage-64 cycle %.2e" % (tag, what, e, TOL, d))
        assert np.all(np.isfinite(z)) and e <= TOL, (tag, what, e)
        assert d >= 1e-9, (tag, what, d)  # the key took effect
        assert np.array_equal(TM._minv(G, r), z)
        worst, nearest = max(worst, e), min(nearest, d)
    print("CASE storage 32 %-34s worst relmax %.2e, nearest to storage 64 %.2e" % (tag, worst, nearest))
    return worst, nearest


# ------------------------------------------------------------------ storage 32: cases
STORAGE = [("q2_654", ()), ("q2_654", (("mg_fuse", 0),)), ("q1_987", ()), ("2d_q4_64", ()), ("q3_532_assembled", ()),
           ("q2_753_mf27", ()), ("q2_11", ())]


@pytest.mark.parametrize("name,keys", STORAGE, ids=["%s%s" % (n, "".join("-%s%d" % kv for kv in k)) for n, k in STORAGE])
def test_storage32_cycle_matches_the_reference(name, keys):
    t0 = time.time()
    m, _, _, _, u, du = TM._inputs(name)
    G = TM._context(name)
    for k, v in keys:
        G.set_tuning(k, v)
    G.set_tuning("precond_storage", 32)
    TM._solve(G, u, du)
    nl = G.mg_n_levels()
    for l in range(nl):  # the kernels the case is in the table for: level 0 of q2_11 on sell_spmv, everything else split
        V = G.mg_level_context(l)
        lds = (V.get_tuning("spmv_lds_launches"), V.get_tuning("spmv_split_launches"))
        assert lds == ((1, 0) if (name == "q2_11" and l == 0) else (0, 1)), (l, lds)
        V.close()
    if name == "q2_753_mf27":
        assert dict(R.case(name)["keys"])["element_tangents"] == 2  # the matrix-free smoother gives way to the fp32 matrix
    _hold_storage32(G, name, _reference(name), name + "".join(" %s %d" % kv for kv in keys))
    print("CASE storage 32 %s: %.1f s" % (name, time.time() - t0))
    G.close()


def test_storage32_on_slabs():
    """q2_4412_3slabs_z: a team exports no matrix, so the product matrices are those of an undecomposed twin at the same state,
    under the precondition that the team's level-0 diagonal blocks are the twin's bits"""
    name = "q2_4412_3slabs_z"
    m, lo, hi, perturb, u, du = TM._inputs(name)
    c = R.case(name)
    G = TM._context(name)
    assert G.comm_info()[0] == c["slabs"]
    G.set_tuning("precond_storage", 32)
    TM._solve(G, u, du)
    _assert_storage(G, 32, team=True)
    H = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb)
    H.set_tuning("precond", 1)
    H.set_interface_traction(TM.TRACTION[c["dim"]])
    TM._solve(H, u, du)
    assert np.array_equal(G.diagonal_blocks(), H.diagonal_blocks())
    ref = _reference(name)
    TM._check_parts(H, ref)
    mats = _exports(H)
    H.close()
    _hold_storage32(G, name, ref, name, mats=mats, team=True)
    G.close()


# ------------------------------------------------------------------ storage 32: sequences on q2_654
SEQ = "q2_654"


def test_storage32_set_before_the_hierarchy_exists():
    """the key before "precond" 1: the levels are built afterwards and take the fine context's storage"""
    m, _, _, _, u, du = TM._inputs(SEQ)
    G = TM._context(SEQ, extra_keys=[("precond_storage", 32)])
    assert G.get_tuning("precond_storage_levels") == G.mg_n_levels() > 1
    TM._solve(G, u, du)
    _hold_storage32(G, SEQ, _reference(SEQ), "key before precond")
    G.close()


def test_storage32_set_after_a_solve_and_back():
    """the key after the first solve (the estimates are those of the fp64 matrices: no bound), then 32 -> 64 -> 32: the middle
    state is the storage-64 reference, the last one the storage-32 reference again"""
    m, _, _, _, u, du = TM._inputs(SEQ)
    ref = _reference(SEQ)
    G = TM._context(SEQ)
    TM._solve(G, u, du)
    _assert_storage(G, 64)
    G.set_tuning("precond_storage", 32)
    _hold_storage32(G, SEQ, ref, "key after the solve", bounds=None)
    G.set_tuning("precond_storage", 64)
    _assert_storage(G, 64)
    lmax = TM._check_shape_and_estimates(G, ref)
    TM._check_cycle(G, m, ref, lmax, SEQ + " back on 64")
    G.set_tuning("precond_storage", 32)
    _hold_storage32(G, SEQ, ref, "32 again", bounds=None, parts=False)
    G.close()


def test_storage32_copies_follow_the_tangent_and_the_lagged_levels():
    """a second solve at a changed state: under "mg_lag" 1 level 0 multiplies with the copy of the NEW tangent, the levels
    below with the copies of the old operators; under "mg_lag" 0 every level with the new ones.  (The two states lie 5.6e-3
    apart in the cycle, tests/test_mirror_multigrid.py: a stale copy fails.)"""
    m, _, _, _, u, du = TM._inputs(SEQ)
    G = TM._context(SEQ, extra_keys=[("precond_storage", 32)])
    TM._solve(G, u, du)
    n0 = G.get_tuning("count_mg_refresh")
    du2 = _second(SEQ)
    TM._solve(G, u, du2)
    assert G.get_tuning("count_mg_refresh") == n0
    _hold_storage32(G, SEQ, _reference(SEQ, "lagged"), "lagged", bounds=None)
    G.set_tuning("mg_lag", 0)
    TM._solve(G, u, du2)
    assert G.get_tuning("count_mg_refresh") == n0 + 1
    _hold_storage32(G, SEQ, _reference(SEQ, "second"), "mg_lag 0", bounds="refresh")
    G.close()


def test_storage32_survives_a_rebuilt_hierarchy():
    """"mg_coarsest" 2 with storage 32 left on: the rebuilt hierarchy answers 32 on every level"""
    m, _, _, _, u, du = TM._inputs(SEQ)
    G = TM._context(SEQ, extra_keys=[("precond_storage", 32)])
    TM._solve(G, u, du)
    nl = G.mg_n_levels()
    G.set_tuning("mg_coarsest", 2)
    assert G.mg_n_levels() == nl + 1 == G.get_tuning("precond_storage_levels")
    G.set(M.V_NEWTON, np.zeros(G.n))
    rc, _, _ = G.cg_solve(1e-8, 400)
    assert rc == 0
    _hold_storage32(G, SEQ, _reference(SEQ, "coarsest2"), "after mg_coarsest 2")
    G.close()


# ------------------------------------------------------------------ storage 32: the small-launch kernel itself
SMALL = [(3, 2, (4, 3, 3)), (3, 1, (5, 4, 4)), (3, 4, (2, 2, 2)), (2, 3, (6, 5))]


@pytest.mark.parametrize("dim,p,reps", SMALL)
def test_fp32_stored_values_on_the_small_launch_kernel(dim, p, reps):
    """part (e) of test_gpu_sell_lds_product.py on sell_spmv_split: the product of the fp32-rounded export, row by row under the
    a-priori bound of an fp64 dot product, no margin"""
    P, G = TP._pair(dim, p, reps, perturb_amp=0.05, seed=3, roles=TS.ROLES)
    TP._randomise_state(P, G, seed=4)
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    assert G.nnodes <= TS.SPLIT_MAX_ROWS
    assert (G.get_tuning("spmv_lds_launches"), G.get_tuning("spmv_split_launches")) == (0, 1)
    A = G.csr()
    worst = 0.0
    for what, x in TS._inputs(G)[:3]:
        y0 = TS._spmv(G, x)
        G.set_tuning("precond_storage", 32)
        G.set_tuning("spmv_as_smoother", 1)
        y32, ratio = TS._hold(G, A, x, "Q%d %s fp32 %s" % (p, reps, what), f32=True)
        worst = max(worst, ratio)
        assert TS.S.worst_ratio(y32, A, x)[0] > 1.0  # not the fp64 product
        G.set_tuning("spmv_as_smoother", 0)
        assert np.array_equal(TS._spmv(G, x), y0)
        G.set_tuning("precond_storage", 64)
        G.set_tuning("spmv_as_smoother", 1)
        assert np.array_equal(TS._spmv(G, x), y0)
        G.set_tuning("spmv_as_smoother", 0)
    print("CASE small launch dim %d Q%d %s worst %.3f" % (dim, p, reps, worst))
    G.close()


# ------------------------------------------------------------------ storage 32: PCG
def test_pcg_with_the_fp32_stored_preconditioner():
    """truncated runs k = 1, 2, 3 and one converged run against pcg_reference.pcg with the storage-32 reference cycle"""
    name = SEQ
    pr = PR.problem(name)
    m, _, _, _, u, du = TM._inputs(name)
    assert np.array_equal(pr.u, u) and np.array_equal(pr.du, du)
    G = TM._context(name, extra_keys=[("precond_storage", 32)])
    TM._solve(G, u, du)
    _assert_storage(G, 32)
    ref = _reference(name)
    mats = _exports(G)
    lmax = tuple(G.mg_level_describe(l)["lmax"] for l in range(G.mg_n_levels()))
    b, x0 = pr.rhs("smooth"), pr.x0("zero")
    K = PR.K_MAX["vcycle"]
    run = PR.pcg(PR.Matrix(pr.A), PR.vcycle(ref, lmax, storage=32, product_matrices=mats), b, x0, K)
    xs, rn = run[0], run[1]
    assert len(rn) == K + 1
    con = m.constrained

    def solve(tol, max_it):
        G.set(M.V_RHS, b)
        G.set(M.V_NEWTON, x0)
        rc, its, res = G.cg_solve(tol, max_it)
        return rc, its, res, G.get(M.V_NEWTON)

    def check(k, res, x, tag):
        ex, er = _relmax(x, PR.distribute(xs[k], con)), abs(res - rn[k]) / rn[k]
        print("    PCG storage 32 %s k %d: x %.1e (tol %.0e)  res %.1e (tol %.0e)" %
              (tag, k, ex, PR.tol_x("vcycle", k), er, PR.tol_r("vcycle", k)))
        assert np.all(np.isfinite(x)) and np.all(x[con] == 0.0)
        assert ex <= PR.tol_x("vcycle", k), (tag, k, ex)
        assert er <= PR.tol_r("vcycle", k), (tag, k, er)

    for k in (1, 2, 3):
        rc, its, res, x = solve(0.0, k)
        assert rc == M.MI_ENOCONV_LIN and its == k
        check(k, res, x, "truncated")
    # ... and they are not the iterates of the fp64-stored preconditioner
    x64 = PR.pcg(PR.Matrix(pr.A), PR.vcycle(ref, lmax), b, x0, 3)[0][3]
    assert _relmax(x, PR.distribute(x64, con)) > 1e3 * PR.tol_x("vcycle", 3)
    tau, bnorm = PR.TAU[name, "vcycle"][0], np.linalg.norm(b)
    want = PR.first_converged(rn, tau * bnorm)
    assert want is not None and all(PR.margin(rn[k], tau * bnorm, PR.E_R["vcycle"][k]) for k in range(want + 1))
    rc, its, res, x = solve(tau, 400)
    assert rc == 0 and its == want and res <= tau * bnorm, (rc, its, want)
    check(its, res, x, "converged at tau %.1e" % tau)
    G.close()


def test_storage32_leaves_the_linear_models_cycle_alone():
    """the linear model's hierarchy multiplies with fp64 values by design: its V-cycle is the same bits under the key"""
    G = M.Context(dim=3, degree=2, reps=(6, 4, 4))
    G.set_tuning("linear_precond", 1)
    G.linear_setup(0.5)
    assert G.linear_mg_n_levels() > 1
    r = np.random.default_rng(3).standard_normal(G.n) * ~G.constrained
    z = G.linear_apply(3, r)
    G.set_tuning("precond_storage", 32)
    assert np.array_equal(G.linear_apply(3, r), z)
    G.close()


# ------------------------------------------------------------------ precision 32
def _rule_reference(G, name, state=""):
    """the fp64 reference of the rule that the library reports for the next smoother product"""
    m, _, _, _, u, du = TM._inputs(name)
    if G.get_tuning("smoother_quadrature_active") == 4:
        return _reference(name, state)
    c = R.case(name)
    assert (c.get("nq0"), c.get("fold0")) == (3, True)
    if state == "":
        return TM._reference(name)
    return R.case_reference(name, u + R.second_increment(m, du), m)


def _hold_precision32(G, name, ref, tag, bounds="first", team=False, seed=0):
    """read-backs; z against the fp64 reference with the assembly-rule fine operator: within TOL32, and farther than 1e-10 (the
    fp32 arithmetic ran); lmax bounds widened by TOL32 on level 0 alone; levels >= 1 keep (b)"""
    m = TM._inputs(name)[0]
    assert G.get_tuning("smoother_precision") == 32 and G.get_tuning("smoother_precision_active") == 32
    assert G.get_tuning("smoother_quadrature_active") == 4
    assert G.get_tuning("precond_storage_levels") == 0
    lmax = TM._check_shape_and_estimates(G, ref, distributed=TM.TEAMS[name] if team else None, bounds=bounds, slack={0: TOL32})
    if not team:
        TM._check_parts(G, ref, levels=range(1, len(ref.shape)))
    worst = 0.0
    for what, r in TM._rhs_set(G, m, seed):
        z = TM._minv(G, r)
        e = _relmax(z, ref.vcycle(r, lmax))
        print("V-cycle precision 32 %s, %s: relmax %.2e (tolerance %.0e)" % (tag, what, e, TOL32))
        assert np.all(np.isfinite(z)) and 1e-10 < e <= TOL32, (tag, what, e)
        assert np.array_equal(TM._minv(G, r), z)
        worst = max(worst, e)
    print("CASE precision 32 %-34s worst relmax %.2e" % (tag, worst))
    return worst


PRECISION = [("q2_543_mf_fine", ()), ("q2_654", (("element_tangents", 2),)), ("q2_4412_3slabs_z", (("element_tangents", 2),))]


@pytest.mark.parametrize("name,keys", PRECISION, ids=[n for n, _ in PRECISION])
def test_precision32_cycle_is_within_its_tolerance_of_the_reference(name, keys):
    m, _, _, _, u, du = TM._inputs(name)
    team = R.case(name).get("slabs", 1) > 1
    G = TM._context(name, extra_keys=list(keys) + [("smoother_precision", 32)])
    TM._solve(G, u, du)
    if team:
        assert G.comm_info()[0] == R.case(name)["slabs"]  # ("mf_halo_overlap" is on by default: launches over cell layers)
    _hold_precision32(G, name, _reference(name), name, team=team)
    G.close()


def test_precision32_falls_back_to_fp64_off_the_production_shape():
    """distorted cells have no box records: the float instantiation does not exist for them, the key changes nothing"""
    name = "q2_753_mf27"
    m, _, _, _, u, du = TM._inputs(name)
    G = TM._context(name, extra_keys=[("smoother_precision", 32)])
    TM._solve(G, u, du)
    assert G.get_tuning("smoother_precision") == 32 and G.get_tuning("smoother_precision_active") == 64
    ref = _rule_reference(G, name)
    lmax = TM._check_shape_and_estimates(G, ref)
    TM._check_cycle(G, m, ref, lmax, name + " smoother_precision 32, fallback")
    G.close()


GRADED = "q2_543_mf_fine"


def test_precision32_takes_effect_with_the_next_assembly_and_follows_the_state():
    m, _, _, _, u, du = TM._inputs(GRADED)
    G = TM._context(GRADED)
    G.set_tuning("mg_lag", 0)
    TM._solve(G, u, du)
    # the key after an assembly: no fp32 records of this tangent yet
    G.set_tuning("smoother_precision", 32)
    assert G.get_tuning("smoother_precision_active") == 64
    ref = _rule_reference(G, GRADED)
    lmax = TM._check_shape_and_estimates(G, ref)
    TM._check_cycle(G, m, ref, lmax, GRADED + " key set, not assembled")
    # ... they come with the next one
    TM._solve(G, u, du)
    _hold_precision32(G, GRADED, _reference(GRADED), "after the next assembly", bounds="refresh")
    # a residual pass in between writes no records and spoils none
    r = TM._rhs_set(G, m, 0)[0][1]
    z = TM._minv(G, r)
    assert np.isfinite(G.assemble_residual())
    assert G.get_tuning("smoother_precision_active") == 32 and np.array_equal(TM._minv(G, r), z)
    # the changed state: records of the new tangent (the two cycles lie 6.4e-3 apart, tests/test_mirror_multigrid.py)
    TM._solve(G, u, _second(GRADED))
    _hold_precision32(G, GRADED, _reference(GRADED, "second"), "second state", bounds="refresh")
    # 32 -> 64 without a new assembly: the rule the library then reports, in fp64
    G.set_tuning("smoother_precision", 64)
    assert G.get_tuning("smoother_precision_active") == 64
    ref = _rule_reference(G, GRADED, "second")
    lmax = TM._check_shape_and_estimates(G, ref, bounds=None)
    TM._check_cycle(G, m, ref, lmax, GRADED + " back on 64")
    # ... and 32 once more: "takes effect with the next tangent assembly" -- until then the same fp64 cycle, to the bit
    z64 = TM._minv(G, r)
    G.set_tuning("smoother_precision", 32)
    assert G.get_tuning("smoother_precision_active") == 64
    assert np.array_equal(TM._minv(G, r), z64)
    G.close()


def test_precision32_with_lagged_diagonal_blocks():
    """"mf_diag_lag" 1 over two tangents of one step: fp32 records of the second tangent, D of the first (and, under the
    default "mg_lag", the coarse operators of the first)"""
    m, _, _, _, u, du = TM._inputs(GRADED)
    G = TM._context(GRADED, extra_keys=[("smoother_precision", 32), ("mf_diag_lag", 1)])
    TM._solve(G, u, du)
    _hold_precision32(G, GRADED, _reference(GRADED), "mf_diag_lag, first tangent")
    TM._solve(G, u, _second(GRADED))
    first, lag = _reference(GRADED), _reference(GRADED, "lagged")
    ref = R.assembled_reference(GRADED, u + _second(GRADED), m, coarse_from=u + du, fine=lag)
    assert _relmax(lag.D[0], first.D[0]) > 1e-4
    ref.D[0] = first.D[0]
    assert _relmax(G.diagonal_blocks(), first.D[0]) <= 1e-12
    _hold_precision32(G, GRADED, ref, "mf_diag_lag, second tangent", bounds=None)
    G.close()
