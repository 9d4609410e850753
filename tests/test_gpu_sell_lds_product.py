"""GPU: sell_spmv, the sliced-ELL LDS-DMA product that ships, against references, on meshes of more than 160 slices.

Why: mi_ctx.cpp sends every launch of at most SELL_SPLIT_MAX_SLICES = 160 slices (10,240 rows) to sell_spmv_split, another
kernel with plain loads and another summation order, and every small mesh that the suite compares with an independent
reference lies below that size.  The cases here are the smallest of their kind above it; every test asserts through the
read-backs "spmv_lds_launches" / "spmv_split_launches" that it runs the kernel it names, so that a change of the threshold
cannot silently move it back.

  case      dim, p, reps                     nodes   what it forces in sell_slice
  q2_11     3, 2, (11, 11, 11)               12,167  WXT 3 / 5; a chunk of exactly SELL_STAGE_BYTES is staged whole
  q2_thin   3, 2, (1, 1, 600)                10,809  nn0 == wx, wy = 3, padding lanes on a lattice one cell thick
  q1_3d     3, 1, (22, 21, 21)               11,132  the generic instantiation (WXT 0), wx 2 / 3
  q3_7      3, 3, (7, 7, 7)                  10,648  wx 4 staged whole and wx 7 in two halves of 32 rows, in one launch
  q4_3d     3, 4, (5, 5, 6)                  11,025  WXT 5 on Q4 rows (wy up to 9), wx 9 in two halves of 20,736 B
  2d_q1     2, 1, (103, 101)                 10,608  D = 2, wx 2 / 3
  2d_q3     2, 3, (35, 34)                   10,918  D = 2, wx 4 / 7
  2d_q4     2, 4, (26, 25)                   10,605  D = 2, wx 5 / 9
  q1_slabs  3, 1, (104, 104, 4), 2 slabs, z  55,125  boundary launches over 160 slices: slice0 != 0, own range of DOT
No shape had to be enlarged: the read-back reports sell_spmv for every launch of every case.

Every case: cells of 0.1, vertices moved by 5 % of that (seeded), roles clamped + z-clamp + interface and the random state of
test_gpu_parity.py (test_global_assembly_with_constraints_and_traction, _randomise_state), update_acceleration, assemble.

  (a) read-back: "spmv_lds_launches" 1 (q1_slabs: 4, interior and boundary launch of both slabs), "spmv_split_launches" 0.
  (b) G.spmv(x) against spmv_reference.product(A, x), A = G.csr(): |y - y_ref|_i <= bound_i on every row (the a-priori bound of
      an fp64 dot product in any order, tests/golden/spmv_reference.py; no margin) for white noise, a smooth field, a unit
      vector at the mesh corner opposite the clamped face and a vector that lives on the constrained dofs alone (the free rows
      of y are then exactly zero); two calls give the same bits.  q1_slabs exports no matrix (teams do not): A is the export
      of an undecomposed context on the same mesh and state, and the diagonal blocks of the two -- which a team does hand
      out, and which sum over every cell of a node -- are asserted equal to the bit.
  (c) A against the oracle's matrix: same pattern, values to TOL_ASM, so that the reference of (b) does not rest on the
      device's own export alone.  Held: every case but q4_3d.  The oracle's assembly on one thread takes 0.2 - 0.4 s
      (2D), 2.5 s (q1_3d), 2.7 s (q2_thin), 6.0 s (q2_11), 9.5 s (q1_slabs), 14.4 s (q3_7) and 37 s (q4_3d); the test gives it up to
      8 threads (cells in parallel, scattered in cell order: the same bits), with which the slowest held cases, q3_7 and
      q1_slabs, take 0.7 s.  q4_3d is held to its export only.  Measured relmax: 6.1e-14 on q2_thin, <= 8.9e-15 elsewhere.
  (d) launch shapes on q2_11 and q3_7: "sell_icol" 0, "sell_unroll" 4 and "spmv_variant" 1 are other instantiations or kernels,
      each held to the bound; "spmv_grid" 1, 7, 56 and "xcd_remap" 1 at grids 56 and 7 are runtime parameters of one
      instantiation that leave a row's summation order alone: bitwise equal to the default launch.
  (e) fp32 storage on q2_11 and 2d_q4: "precond_storage" 32 with "spmv_as_smoother" 1 against the product of the fp32-rounded
      values under the same bound (all arithmetic of that kernel is fp64); it violates the fp64 bound (the key took effect);
      without either key the context is back on the fp64 bits.
  (f) CHEB, on mg_reference.MID_CASES (q1_3d, q2_11, 2d_q4 with the state of the multigrid tests): z = M^-1 r against
      mg_reference.Reference at the tolerance of test_gpu_multigrid_reference.py for its three right-hand sides, with
      "mg_fuse" 1 (level 0 has fewer than 100,000 nodes, runs sell_spmv by its level context's read-back, assembled rows,
      "spmv_variant" 3: the conditions under which mi_mg.cpp fuses) and with "mg_fuse" 0 (plain product + cheb_step_blk).
      The smoother's D is the block-Jacobi one (cheb_blk 1) in both: the scalar diagonal (cheb_blk 0) is selected by
      MI_MG_BLOCK in the experiments build only and is NOT covered.  Levels >= 1 of these cases stay on sell_spmv_split.
  (g) DOT, on q1_3d and q1_slabs: truncated runs cg_solve(0.0, k), k = 1, 2, 3, "precond" 0, "small_cg" 0, "cg_fused_dot" 1
      and 0, against pcg_reference.pcg on A with the Jacobi preconditioner, at TOL_x(k) / TOL_r(k) of its committed tables;
      one host synchronisation per solve (the three-launch form; the one-launch solver counts none).

Measured on an MI355X, worst |y - y_ref|_i / bound_i (the unit vector gives 0 everywhere: one term per row is exact):
            (b)     (d)                                   (e)                   (b)                   (b)
  q2_11     0.078   0.078 (spmv_variant 1: 0.032)         0.072      q1_3d      0.081      2d_q1      0.235
  q3_7      0.047   0.047 (spmv_variant 1: 0.010)                    q1_slabs   0.108      2d_q3      0.149
  q2_thin   0.072                                                    q4_3d      0.029      2d_q4      0.113 ((e): 0.129)
"sell_icol" 0 and "sell_unroll" 4 give the bits of the default launch on both cases of (d).
Cycles (f), worst relmax: q1_3d 2.7e-15, q2_11 3.0e-15, 2d_q4 1.7e-14 (tolerance 1e-13), the same figures under "mg_fuse" 1
and 0; lmax / lambda_true = 1.149998 .. 1.150000 on every level.  Truncated PCG (g), worst deviation as a part of its tolerance:
q1_3d x 0.0049, res 0.0033; q1_slabs x 0.0044, res 0.0066 (either form of the dot product).
The tests found no error in csrc/.
Run time on the same machine, 28 tests in 38 s: the slowest are (f) on q2_11 with 13.7 s and on q1_3d with 7.3 s, of which 12 s
and 6 s build the numpy hierarchy of the case (36,501 and 33,396 dofs; operator_matrix's einsum over every cell and point,
built once per case and shared by both forms of the smoother step); the device's part of either is under a second.  Every
other test takes at most 2.1 s.  q4_3d is the slowest product test with 1.9 s: its export has 19.1 M entries, which four long
double products and bounds walk; no smaller 3D Q4 mesh has more than 10,240 nodes ((5, 5, 5) has 9,261).

Shown to fail (each change made in a scratch copy of the library, arithmetic or the choice of an in-bounds element only, run
once, never committed; with the first assertion that fails):
  no `lane < rem` tail load in sell_slice (stale LDS)       15 fail: (b) on white noise, ratios 1e14 .. 1e17, in every 3D case; (d);
                                                           (e) q2_11; (f) the first solve of q1_3d and q2_11 does not converge;
                                                           (g) x_1 3.8e-3 off.  The 2D cases pass: their chunks (2,048 B x wx) have
                                                           no tail
  both halves consumed (`ns == 1 ||` and its other arm     3: (b) q3_7 and q4_3d, (d) q3_7 -- the two cases whose chunks exceed
  replaced by true)                                        SELL_STAGE_BYTES; no other comparison with a reference runs such rows
  gy never wrapped in the ICOL walk                        14: (b) every 3D case but q2_thin (wy == nn1 there: the wrap adds 0), (d),
                                                           (e) q2_11, (f) q1_3d and q2_11, (g); no 2D case (one y-run per row)
  remap applied whatever nwg % 8, clamped to nwg - 1       2: (d), bitwise equality at grid 7 with "xcd_remap" 1, both cases.  (A first
                                                           version of (d) overwrote the result vector through the same launch and
                                                           passed: the rows that the launch left out kept the right values of two
                                                           calls before.  Hence _spmv's overwrite on the row-per-wave kernel.)
  own_begin taken as 0 in the DOT epilogue                 none, and none can: build_sell puts the owned rows of a slab into its
                                                           slices and no others, and padding lanes leave at node < 0, so neither
                                                           limit of the own range ever decides in these kernels.  Instead:
  partials[b] for partials[part0 + b] in sell_spmv         1: (g) q1_slabs with "cg_fused_dot" 1, x_1 1.7 off (the boundary launch
                                                           writes over the interior's partials); one slab and "cg_fused_dot" 0 pass
  cheb_c1 taken as 0 in sell_slice's epilogue alone        3: (f) q1_3d and q2_11 under "mg_fuse" 1, relmax 0.17 and 0.12 on the
  (sell_spmv_split keeps it)                               random right-hand side; 2d_q4: the first solve does not converge.  So
                                                           level 0 of these cases does take its fused steps on sell_spmv
"""
import functools
import os
import sys
import time

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_multigrid_reference as TM
import test_gpu_parity as TP
from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mg_reference as R  # noqa: E402
import pcg_reference as PR  # noqa: E402
import spmv_reference as S  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

ROLES = [O.FACE_CLAMPED, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_ZCLAMP, O.FACE_INTERFACE]
CASES = {
    "q2_11": dict(dim=3, p=2, reps=(11, 11, 11), nodes=12167),
    "q2_thin": dict(dim=3, p=2, reps=(1, 1, 600), nodes=10809),
    "q1_3d": dict(dim=3, p=1, reps=(22, 21, 21), nodes=11132),
    "q3_7": dict(dim=3, p=3, reps=(7, 7, 7), nodes=10648),
    "q4_3d": dict(dim=3, p=4, reps=(5, 5, 6), nodes=11025, oracle=False),
    "2d_q1": dict(dim=2, p=1, reps=(103, 101), nodes=10608),
    "2d_q3": dict(dim=2, p=3, reps=(35, 34), nodes=10918),
    "2d_q4": dict(dim=2, p=4, reps=(26, 25), nodes=10605),
    "q1_slabs": dict(dim=3, p=1, reps=(104, 104, 4), nodes=55125, slabs=2, cut_axis=3, lds=4),
}
SPLIT_MAX_ROWS = 160 * 64  # SELL_SPLIT_MAX_SLICES slices of 64 rows (dealii-adapter_amd/csrc/mi_kernels.h)


# ------------------------------------------------------------------ set-up
def _make(name, slabs=None):
    """oracle problem (not assembled) and device context of a case at its state, tangent assembled; slabs: override (1: the
    undecomposed context of a team case)"""
    c = CASES[name]
    kw = {}
    if (c.get("slabs", 1) if slabs is None else slabs) > 1:
        kw = dict(slabs=c["slabs"], cut_axis=c["cut_axis"])
    P, G = TP._pair(c["dim"], c["p"], c["reps"], perturb_amp=0.05, seed=3, roles=ROLES, **kw)
    assert G.nnodes == c["nodes"] > SPLIT_MAX_ROWS and G.comm_info()[0] == kw.get("slabs", 1)
    TP._randomise_state(P, G, seed=4)
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    return P, G


def _assert_lds(G, name):
    """(a)"""
    lds, split = G.get_tuning("spmv_lds_launches"), G.get_tuning("spmv_split_launches")
    assert (lds, split) == (CASES[name].get("lds", 1), 0), (name, lds, split)


@functools.lru_cache(maxsize=None)
def _built(name):
    """(P, G, A) of a case, shared by the tests that leave the context as they found it; A: the matrix the products are held to"""
    P, G = _make(name)
    if CASES[name].get("slabs", 1) == 1:
        return P, G, G.csr()
    # a team exports no matrix: that of the undecomposed context, whose bits the slabs assemble (diagonal blocks: every cell of a node)
    _, G1 = _make(name, slabs=1)
    assert np.array_equal(G.diagonal_blocks(), G1.diagonal_blocks())
    A = G1.csr()
    G1.close()
    return P, G, A


def _inputs(G):
    """white noise, a smooth field, a unit vector at the corner opposite the clamped face, the constrained dofs alone"""
    rng = np.random.default_rng(G.n)
    X, con = G.coords, G.constrained
    s = (X - X.min(0)) / np.ptp(X, axis=0).max()
    smooth = np.stack([np.sin(s @ rng.uniform(0.5, 3.0, G.dim) * np.pi + rng.uniform(0, 6.0)) for _ in range(G.dim)], -1).reshape(-1)
    corner = int(np.argmax(X.sum(1)))
    unit = np.zeros(G.n)
    unit[corner * G.dim] = 1.0
    assert not con[corner * G.dim] and con.any()
    return [("white", rng.standard_normal(G.n)), ("smooth", smooth), ("corner", unit), ("constrained", rng.standard_normal(G.n) * con)]


def _spmv(G, x):
    """G.spmv(x) into a result vector that holds another product: a row that no workgroup computes keeps a wrong value, not
    that of the last call.  The other product runs on the row-per-wave kernel, which no key of the sliced-ELL launch reaches
    (a launch shape that leaves rows out would leave them out of its own overwrite too)"""
    variant = G.get_tuning("spmv_variant")
    G.set_tuning("spmv_variant", 1)
    G.spmv(-3.0 * x[::-1])
    G.set_tuning("spmv_variant", variant)
    return G.spmv(x)


def _hold(G, A, x, tag, f32=False):
    """|y - y_ref|_i <= bound_i on every row, exact zeros where the bound is zero; returns (y, worst ratio)"""
    y = _spmv(G, x)
    ratio, zeros = S.worst_ratio(y, A, x, f32)
    print("    %-40s worst |y - y_ref| / bound %.3f" % (tag, ratio))
    assert np.all(np.isfinite(y)) and zeros and ratio <= 1.0, (tag, ratio, zeros)
    return y, ratio


# ------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_is_within_the_rounding_bound_of_the_reference(name):
    t0 = time.time()
    _, G, A = _built(name)
    _assert_lds(G, name)
    assert A.shape == (G.n, G.n) and np.all(np.diff(A.indptr) > 0)
    free = ~G.constrained
    worst = 0.0
    for what, x in _inputs(G):
        y, ratio = _hold(G, A, x, "%s %s" % (name, what))
        worst = max(worst, ratio)
        assert np.array_equal(G.spmv(x), y)
        if what == "constrained":
            assert np.all(y[free] == 0.0)
    print("CASE %-9s (b) worst %.3f, %.1f s" % (name, worst, time.time() - t0))


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.get("oracle", True)))
def test_exported_matrix_is_the_oracle_matrix(name):
    P, _, A = _built(name)
    t0 = time.time()
    O.lib().orc_set_threads(min(8, len(os.sched_getaffinity(0))))  # (cells in parallel, summed in cell order: the same bits)
    try:
        P.update_acceleration()
        P.assemble()
    finally:
        O.lib().orc_set_threads(1)
    K = P.csr()
    print("CASE %-9s (c) oracle assembly %.1f s" % (name, time.time() - t0))
    assert np.array_equal(K.indptr, A.indptr) and np.array_equal(K.indices, A.indices)
    e = TP._relmax(A.data, K.data)
    print("CASE %-9s (c) matrix relmax %.2e" % (name, e))
    assert e < TP.TOL_ASM


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("name", ["q2_11", "q3_7"])
def test_launch_shapes_and_instantiations(name):
    _, _, A = _built(name)
    _, G = _make(name)
    x = _inputs(G)[0][1]
    y0, worst = _hold(G, A, x, "%s default" % name)
    _assert_lds(G, name)
    for key, value, back in [("sell_icol", 0, 1), ("sell_unroll", 4, 5), ("spmv_variant", 1, 3)]:
        G.set_tuning(key, value)
        assert key == "sell_unroll" or G.get_tuning(key) == value  # (the launch shape has no read-back)
        worst = max(worst, _hold(G, A, x, "%s %s %d" % (name, key, value))[1])
        G.set_tuning(key, back)
        assert np.array_equal(_spmv(G, x), y0)
    for grid, remap in [(1, 0), (7, 0), (56, 0), (56, 1), (7, 1)]:
        G.set_tuning("spmv_grid", grid)
        G.set_tuning("xcd_remap", remap)
        _assert_lds(G, name)
        assert np.array_equal(_spmv(G, x), y0), (grid, remap)
    print("CASE %-9s (d) worst %.3f" % (name, worst))
    G.close()


# ------------------------------------------------------------------ (e)
@pytest.mark.parametrize("name", ["q2_11", "2d_q4"])
def test_fp32_stored_values_against_the_fp32_reference(name):
    _, _, A = _built(name)
    _, G = _make(name)
    _assert_lds(G, name)
    assert G.get_tuning("smoother_operator_active") == 0  # the smoother's form of this level is the assembled matrix
    worst = 0.0
    for what, x in _inputs(G)[:3]:
        y0 = _spmv(G, x)
        G.set_tuning("precond_storage", 32)
        G.set_tuning("spmv_as_smoother", 1)
        y32, ratio = _hold(G, A, x, "%s fp32 %s" % (name, what), f32=True)
        worst = max(worst, ratio)
        assert S.worst_ratio(y32, A, x)[0] > 1.0  # not the fp64 product: the key took effect
        G.set_tuning("spmv_as_smoother", 0)
        assert np.array_equal(_spmv(G, x), y0)
        G.set_tuning("precond_storage", 64)
        G.set_tuning("spmv_as_smoother", 1)
        assert np.array_equal(_spmv(G, x), y0)
        G.set_tuning("spmv_as_smoother", 0)
    print("CASE %-9s (e) worst %.3f" % (name, worst))
    G.close()


# ------------------------------------------------------------------ (f) CHEB
@functools.lru_cache(maxsize=None)
def _mid_reference(name):
    m, _, _, _, u, du = TM._inputs(name)
    return R.case_reference(name, u + du, m)


@pytest.mark.parametrize("name", sorted(R.MID_CASES))
def test_fused_and_unfused_smoother_steps_on_the_lds_kernel(name):
    c = R.MID_CASES[name]
    m, lo, hi, perturb, u, du = TM._inputs(name)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb)
    assert np.array_equal(G.constrained, m.constrained) and np.abs(G.coords - m.coords).max() < 1e-14
    G.set_tuning("precond", 1)
    G.set_interface_traction(TM.TRACTION[c["dim"]])
    TM._solve(G, u, du)
    ref = _mid_reference(name)
    lmax = TM._check_shape_and_estimates(G, ref)
    # level 0 runs sell_spmv and meets the conditions of fuse_level() in mi_mg.cpp under "mg_fuse" 1
    V = G.mg_level_context(0)
    assert (V.get_tuning("spmv_lds_launches"), V.get_tuning("spmv_split_launches")) == (1, 0)
    assert SPLIT_MAX_ROWS < V.nnodes <= 100000
    assert G.get_tuning("spmv_variant") == 3 and G.get_tuning("fine_level") == 0 and G.get_tuning("smoother_operator_active") == 0
    for l in range(1, G.mg_n_levels()):
        L = G.mg_level_context(l)
        assert (L.get_tuning("spmv_lds_launches"), L.get_tuning("spmv_split_launches")) == (0, 1)
    rhs = TM._rhs_set(G, m, 0)
    z_ref = [ref.vcycle(r, lmax) for _, r in rhs]
    worst = 0.0
    for fuse in (1, 0):
        G.set_tuning("mg_fuse", fuse)
        for (what, r), zr in zip(rhs, z_ref):
            z = TM._minv(G, r)
            e = TM._relmax(z, zr)
            print("    V-cycle %s mg_fuse %d, %s: relmax %.2e (tolerance %.0e)" % (name, fuse, what, e, TM.TOL))
            assert np.all(np.isfinite(z)) and e <= TM.TOL, (name, fuse, what, e)
            assert np.array_equal(TM._minv(G, r), z)
            worst = max(worst, e)
    print("CASE %-9s (f) worst relmax %.2e" % (name, worst))
    G.close()


# ------------------------------------------------------------------ (g) DOT
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["q1_3d", "q1_slabs"])
def test_truncated_jacobi_pcg_with_the_fused_dot_product(name, fused):
    _, _, A = _built(name)
    _, G = _make(name)
    for key, value in [("precond", 0), ("small_cg", 0), ("cg_fused_dot", fused)]:
        G.set_tuning(key, value)
    _assert_lds(G, name)
    free = ~G.constrained
    xin = dict(_inputs(G))
    worst = [0.0, 0.0]
    for what in ("smooth", "white"):
        b = 1e2 * xin[what] / np.abs(xin[what]).max() * free
        x0 = np.zeros(G.n)
        xs, rn, _, _ = PR.pcg(PR.Matrix(A), PR.jacobi(A), b, x0, 3)
        assert len(rn) == 4
        for k in (1, 2, 3):
            G.set(M.V_RHS, b)
            G.set(M.V_NEWTON, x0)
            s0 = G.get_tuning("count_cg_host_sync")
            rc, its, res = G.cg_solve(0.0, k)
            polls = G.get_tuning("count_cg_host_sync") - s0
            x = G.get(M.V_NEWTON)
            assert rc == M.MI_ENOCONV_LIN and its == k, (what, k, rc, its)
            assert polls == 1, (k, polls)  # three launches per iteration, polled once per batch of 16
            assert np.all(np.isfinite(x)) and np.all(x[~free] == 0.0)
            ex = TM._relmax(x, PR.distribute(xs[k], ~free))
            er = abs(res - rn[k]) / rn[k]
            print("    %s %s fused %d k %d: x %.1e (tol %.0e)  res %.1e (tol %.0e)" %
                  (name, what, fused, k, ex, PR.tol_x("jacobi", k), er, PR.tol_r("jacobi", k)))
            assert ex <= PR.tol_x("jacobi", k), (what, k, ex)
            assert er <= PR.tol_r("jacobi", k), (what, k, er)
            worst = [max(worst[0], ex / PR.tol_x("jacobi", k)), max(worst[1], er / PR.tol_r("jacobi", k))]
    print("CASE %-9s (g) fused %d worst of the tolerance: x %.3g res %.3g" % (name, fused, worst[0], worst[1]))
    G.close()
