"""GPU: the iterations of mi_cg_solve and mi_linear_step (cg_run, dealii-adapter_amd/csrc/mi_ctx.cpp) against an independent
numpy PCG (tests/golden/pcg_reference.py), iterate by iterate.

Why: every operand of the linear solve is pinned to a reference (operators, smoother products, the V-cycle, the linear
model's matrices); the Krylov iteration that combines them was held to "converges to the direct solve" and "about as many
iterations as the oracle".  A beta from the wrong ping-pong slot, a missing term in the single-reduction denominator, a final
check that reports it - 1, an x updated once more after the flag went up: all of these converge to the same solution and move
the count by one or two -- and the count is a product number (bench.py divides by it, the warm start and "mg_refresh_every"
read it).

Per case: context, shape keys, state of mg_reference.case_state, update_acceleration, assemble; with the V-cycle one cg_solve
that builds the hierarchy, then lmax per level from mi_mg_level_describe (the one scalar per level that the reference takes
from the device, as in test_gpu_multigrid_reference.py).  No re-assembly afterwards.  Then, with V_RHS and V_NEWTON set by
the test (zero on constrained dofs):
  (a) truncated runs cg_solve(0.0, k): MI_ENOCONV_LIN, its == k, res = ||r_k|| to TOL_r(k), V_NEWTON = x_k to TOL_x(k) with
      exact zeros on constrained dofs.  k: 1, 2, 3, 5, 8 with the V-cycle; 1, 2, 3, 15, 16, 17, 32, 33 for the three-launch
      Jacobi form (both sides of both polls); 1, 2, 17, 33 for the one-launch solver.  Inputs: the smooth right-hand side from
      x0 = 0 and from a random x0 (r0 = b - A x0 through team_spmv), white noise and the assembly's own residual from x0 = 0.
  (b) converged runs at the tolerances of pcg_reference.TAU (Jacobi: converging inside a batch, on its % 16 == 0 and on
      its % 16 == 1): rc == 0, its EQUAL to the reference's count, res to TOL_r(its) and <= tau ||b||, x to TOL_x(its); for the
      reference's run with the device's lmax the margin condition of test_mirror_pcg.py is asserted again.
      The same counts are then asked of the other inputs -- random x0, rough right-hand side, the assembly's residual -- at
      tolerances taken from the reference's run of that input (geometric_tau, margin asserted at run time).  max_it == its
      converges, max_it == its - 1 gives MI_ENOCONV_LIN with its - 1; a start that satisfies the rule gives its == 0, x
      unchanged to the bit and res = ||b - A x0|| within the rounding bound of that residual.
  (c) every form of the table below runs (a) and (b) against the same cached reference runs, and what can be read back about
      the form is asserted: host synchronisations per solve (none for the one-launch solver, one per batch of 16 for the
      three-launch form, one per iteration with the V-cycle), "cg_single_reduction_active", comm_info, and the scalar
      all-reduces of five iterations on teams: 11 (Jacobi), 15 (standard recurrence), 10 (single reduction).
  (d) predicted start and speculation ("cg_warm_start" 2 / 3, V-cycle, one slab and three): eight solves after
      mi_newton_begin_step each, whose right-hand sides and tolerances make the solve converge later than the expected count,
      on it, and before expected - 2 (the flag must silence the iterations in the queue); "cg_speculate_margin" 1; two
      histories; a truncated run inside the speculated window.  its, res and x against the reference started from alpha h,
      equal to the bit to the same sequence under "cg_speculate" 0, with fewer host synchronisations.
  (e) mi_linear_step: three steps on an assembled 2D Q3 and a matrix-free 3D Q3 distorted mesh (those of
      test_gpu_linear_model_reference.py, whose set-up helpers are used); its and res per step against the reference on the
      mirror's stepping matrix and right-hand side from the previous velocity, absolute tolerance.  The assembled mesh is small
      enough for the one-launch solver, which is what runs there; the matrix-free mesh takes the three-launch path.

  form                                    keys                                              cases
  Jacobi, three launches                  precond 0, small_cg 0, cg_fused_dot 1 | 0,        2d_q2_186, q2_432_distorted
                                          spmv_variant 3 | 1
  Jacobi, one launch                      precond 0, small_cg 1                             2d_q2_small, q2_small (under
                                          SMALL_CG_MAX_MATRIX_BYTES by pcg_reference.sell_matrix_bytes); 2d_q2_above, q2_above
                                          (the next sizes: three launches, asserted by the synchronisation count)
  Jacobi on the matrix-free product       fine_level 1, precond 0                           q2_543_mf_fine, q3_532_rule5
  V-cycle, standard recurrence            precond 1, cg_single_reduction 0                  q2_654, q2_543_mf_fine,
  V-cycle, single reduction               precond 1, cg_single_reduction 1                  q3_532_rule5, 2d_q2_186
  teams: Jacobi / standard / single       slabs, cut_axis; cg_single_reduction 0 | -1       q2_4412_3slabs_z, q2_1244_2slabs_x,
                                                                                            q2_4416_induced

Tolerances: TOL_x(k) = min(1e-6, 64 E_x(k) rounded up to a power of ten), TOL_r(k) likewise, from the committed tables of the
reference's own float64 rounding against long double (pcg_reference.E_X / E_R, measured by tests/test_mirror_pcg.py); 64 is the
V-cycle test's margin for the device's other summation orders.  With the V-cycle: TOL_x 1e-13 at k = 1, then 1e-12; TOL_r
1e-12 up to k = 6, 1e-11 up to k = 9, 1e-10 after; Jacobi: 1e-13 at k = 1 to 1e-7 (x) and 1e-6 (res) at k = 33, where the reference itself
has lost seven digits.  The assembly's residual, the starts of (d) and the steps of (e) are held to the same tables, which were
measured on the smooth and the white-noise right-hand side and the random start.  One
departure, (d) only: after a predicted start TOL_r is multiplied by |b| / |r0| (and still capped at 1e-6), because r0 = b -
A (alpha h) is then what cancellation leaves of b and every rounding relative to |b| -- of h, which the two sides share to
TOL_x only, of alpha, of the product -- is that much larger relative to |r0| and to every residual after it.  Measured: the
solve that starts from a right-hand side 1e-4 away from the previous one (|b| / |r0| = 2.5e3) ends 1.5e-11 from the
reference's residual on one slab and 8.2e-12 on three, x 3e-15; all other runs of (d) stay below 2e-13.

Measured on an MI355X, worst deviation per form (x: relmax of the iterate, res: relative to ||r_k||; in brackets as a part of the
tolerance of its k):
  Jacobi, three launches          x 7.4e-12 (0.04)   res 7.2e-09 (0.02)      V-cycle, standard          x 6.0e-15 (0.03)   res 4.7e-14 (0.05)
  Jacobi, one launch              x 2.7e-10 (0.06)   res 2.0e-07 (0.2)       V-cycle, single reduction  x 6.0e-15 (0.03)   res 4.8e-14 (0.05)
  ... the next size above         x 2.1e-10 (0.07)   res 6.0e-09 (0.01)      teams, standard            x 5.6e-15 (0.05)   res 4.9e-14 (0.04)
  Jacobi, matrix-free product     x 3.6e-13 (0.03)   res 3.8e-12 (0.007)     teams, single reduction    x 5.6e-15 (0.05)   res 5.1e-14 (0.03)
  teams, Jacobi                   x 6.4e-12 (0.04)   res 1.6e-10 (0.009)     speculated, one slab       x 3.1e-15 (0.03)   res 1.5e-11 (0.003)
  linear model, assembled         v 5.9e-15 (0.006)  res 6.8e-15 (0.007)     speculated, three slabs    x 3.7e-15 (0.004)  res 8.2e-12 (0.002)
  linear model, matrix-free       v 1.3e-14 (0.01)   res 4.7e-15 (0.005)
The Jacobi figures are those of k = 32, 33; up to k = 17 every form stays below 1e-14.  Every converged run, 12 per Jacobi and
8 per V-cycle context and 21 of (d), reports the reference's count; the residual of a start that satisfies the rule lies within
1e-14 of ||b - A x0|| (bound 5e-11).  (d) on q2_654 and on three slabs alike: counts 8, 10, 10, 7, 7, 10, 10 and the truncated 3
where the previous solve let 0, 8, 10, 10, 7, 7, 10, 10 be expected; host synchronisations 8, 4, 2, 1, 2, 4, 1, 1 against 8, 10, 10, 7, 7,
10, 10, 3 without speculation; on q2_543_mf_fine the early solve ends after one iteration with seven more in the queue.
The tests found no error in csrc/.  Run time on the same machine: the slowest test here takes 4.1 s (teams, standard recurrence,
q2_4416_induced), (d) 1.5 s on q2_654 and 2.6 s on three slabs; the slowest test of
test_gpu_multigrid_reference.py takes 5.1 s there (q2_888).

Shown to fail (each change made in a scratch copy of the library, arithmetic only, run once, never committed; 36 tests, with the
first assertion that fails):
  beta = rz / sc[it & 1] in cg_update_p                      25 fail: the truncated run of k = 2 breaks down (p.Ap <= 0) instead of
                                                             reporting its == 2 (every form on cg_update_p; not the one-launch solver,
                                                             the single-reduction form on one slab or the assembled linear model)
  denom = zw in cg_update_single                             8: x_2 of the truncated run, 6e-5 .. 6e-3 off (single form, one slab and teams)
  cg_final_check writes it - 1                               32: its == 0 from cg_solve(0.0, 1); in (d) 7 iterations reported for 8
                                                             (all but the one-launch solver and the linear model)
  no flags[0] guard in cg_update_xr                          25: x of the run converged at tau = 0.51 .. 0.69, 0.26 .. 0.74 off, "x unchanged"
                                                             of the start that satisfies the rule, v of the linear model 0.28 off: the
                                                             Jacobi batches and the polled V-cycle loop enqueue an update behind the
                                                             test as well, not (d) alone
  |b|^2 of the previous solve on a team, single form        4: the solve that builds the hierarchy does not converge (tolerance 0 from the
                                                             never-reduced total), in the three team cases and in (d) on slabs
  launch_scale_start skipped                                 3: (d) alone, the solve after the first one: 11 iterations for 10, 10 for 9,
                                                             and on q2_654 res 3.6e-11 off at the same count
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pcg_reference as P  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

TRACTION = {3: (0.0, -1e3, 200.0), 2: (0.0, -1e3)}
EPS = np.finfo(float).eps
WORST = {}  # form -> [worst x deviation / tolerance ..., as printed at the end of every test]


# ------------------------------------------------------------------ set-up
def _context(name, precond, keys=()):
    c, pr = P.MESHES[name], P.problem(name)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=pr.lo, hi=pr.hi, face_role=c["roles"], perturb=pr.perturb,
                  slabs=c.get("slabs", 1), cut_axis=c.get("cut_axis", 0))
    assert np.array_equal(G.constrained, pr.m.constrained) and np.abs(G.coords - pr.m.coords).max() < 1e-14
    assert G.comm_info()[0] == c.get("slabs", 1)
    for k, v in list(c.get("keys", [])):
        if precond or k in ("fine_level", "element_tangents"):  # (the other shape keys are the hierarchy's)
            G.set_tuning(k, v)
    G.set_tuning("precond", precond)
    for k, v in keys:
        G.set_tuning(k, v)
    G.set_interface_traction(TRACTION[c["dim"]])
    return G, pr


def _assemble(G, pr, precond):
    """state, tangent and, with the V-cycle, the hierarchy; returns (the assembly's residual on the free dofs, lmax or None)"""
    G.set(M.V_U, pr.u)
    G.set(M.V_DELTA, pr.du)
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    b_res = G.get(M.V_RHS) * pr.free
    if not precond:
        assert G.get_tuning("precond") == 0
        return b_res, None
    G.set(M.V_NEWTON, np.zeros(G.n))
    rc, _, _ = G.cg_solve(1e-8, 400)
    assert rc == 0
    shape = pr.ref.shape
    assert G.mg_n_levels() == len(shape)
    lmax = []
    for l, sh in enumerate(shape):
        d = G.mg_level_describe(l)
        assert (d["degree"], d["reps"], d["n_dofs"], d["exact_solve"]) == (sh["degree"], sh["reps"], sh["n_dofs"], sh["exact"])
        lmax.append(d["lmax"])
    return b_res, tuple(lmax)


def _solve(G, b, x0, tol, max_it):
    """one mi_cg_solve from the test's own right-hand side and start; (rc, its, res, x, host synchronisations, all-reduces)"""
    G.set(M.V_RHS, b)
    G.set(M.V_NEWTON, x0)
    s0, a0 = G.get_tuning("count_cg_host_sync"), G.get_tuning("count_scalar_allreduce_cg")
    rc, its, res = G.cg_solve(tol, max_it)
    return (rc, its, res, G.get(M.V_NEWTON), G.get_tuning("count_cg_host_sync") - s0,
            G.get_tuning("count_scalar_allreduce_cg") - a0)


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _tol_r(pre, k, kappa=1.0):
    """kappa = |b| / |r0| of a predicted start (1 otherwise): r0 = b - A (alpha h) is what cancellation leaves of b, so the
    rounding of h, of alpha and of the product, which is relative to |b|, is kappa times as large relative to |r0| and to
    every residual after it"""
    return min(1e-6, P.tol_r(pre, k) * max(1.0, kappa))


def _record(form, pre, k, ex, er, kappa=1.0):
    w = WORST.setdefault(form, [0.0, 0.0, 0.0, 0.0])
    w[0], w[1] = max(w[0], ex), max(w[1], er)
    w[2], w[3] = max(w[2], ex / P.tol_x(pre, k)), max(w[3], er / _tol_r(pre, k, kappa))


def _report(form):
    w = WORST.get(form)
    if w:
        print("FORM %-34s worst x %.1e  res %.1e  (of the tolerance: x %.2g  res %.2g)" % (form, w[0], w[1], w[2], w[3]))


def _check_iterate(form, tag, pr, pre, k, res, x, ref, kappa=1.0):
    """res and x of a run that stopped at iteration k against the reference run `ref` = (xs, rn, ...)"""
    xs, rn = ref[0], ref[1]
    assert np.all(np.isfinite(x)) and np.all(x[pr.m.constrained] == 0.0), tag
    want = P.distribute(xs[k], pr.m.constrained)
    ex = _relmax(x, want) if np.abs(want).max() > 0 else float(np.abs(x).max())
    er = abs(res - rn[k]) / rn[k]
    print("    %-46s k %2d  x %.1e (tol %.0e)  res %.1e (tol %.0e)" % (tag, k, ex, P.tol_x(pre, k), er, _tol_r(pre, k, kappa)))
    assert ex <= P.tol_x(pre, k), (tag, k, ex)
    assert er <= _tol_r(pre, k, kappa), (tag, k, er, res, rn[k])
    _record(form, pre, k, ex, er, kappa)


def _polls(pre, small, its, max_it):
    """host synchronisations of one solve: none in the one-launch solver; the three-launch Jacobi form polls after every
    batch of CG_BATCH enqueued iterations and learns of convergence at iteration i from the update of i + 1 or from the final
    check of the batch that ends with i; with the V-cycle every iteration is polled"""
    if small:
        return 0
    if pre == "vcycle":
        return max(1, its)
    return max(1, -(-min(its, max_it) // P.CG_BATCH))


def _inputs(pr, b_res):
    out = [(what, start, pr.rhs(what), pr.x0(start)) for what, start in P.INPUTS]
    return out + [("residual", "zero", b_res, pr.x0("zero"))]


def _run_reference(pr, pre, what, start, b, x0, lmax):
    key = (what, start) if what != "residual" else (what, hash(b.tobytes()))
    return pr.run(pre, b, x0, P.K_MAX[pre], lmax, key=key)


def _protocol(G, pr, pre, lmax, b_res, klist, form, small=False):
    """(a), (b) and the counters of (c) on one context"""
    name = pr.name
    # (a)
    for what, start, b, x0 in _inputs(pr, b_res):
        ref = _run_reference(pr, pre, what, start, b, x0, lmax)
        assert len(ref[1]) == P.K_MAX[pre] + 1
        for k in klist:
            rc, its, res, x, polls, _ = _solve(G, b, x0, 0.0, k)
            assert rc == M.MI_ENOCONV_LIN and its == k, (what, start, k, rc, its)
            _check_iterate(form, "%s %s/%s truncated" % (name, what, start), pr, pre, k, res, x, ref)
            assert polls == _polls(pre, small, k, k), (k, polls)
    # (b)
    b, x0 = pr.rhs("smooth"), pr.x0("zero")
    ref = _run_reference(pr, pre, "smooth", "zero", b, x0, lmax)
    xs, rn = ref[0], ref[1]
    bnorm = np.linalg.norm(b)
    counts = []
    for tau in P.TAU[name, pre]:
        want = P.first_converged(rn, tau * bnorm)
        assert want is not None and all(P.margin(rn[k], tau * bnorm, P.E_R[pre][k]) for k in range(want + 1))
        rc, its, res, x, polls, _ = _solve(G, b, x0, tau, 400)
        print("    %s tau %.1e: its %d (reference %d), res / (tau |b|) %.3f" % (name, tau, its, want, res / (tau * bnorm)))
        assert rc == 0 and its == want, (tau, rc, its, want)
        assert res <= tau * bnorm
        _check_iterate(form, "%s converged at tau %.1e" % (name, tau), pr, pre, its, res, x, ref)
        assert polls == _polls(pre, small, its, 400), (its, polls)
        counts.append(want)
    assert tuple(counts) == P.TAU_AT[pre]  # (the iteration counts the tolerances were chosen for)
    # ... and on the other inputs, the assembly's own residual and the random start among them: the tolerance that the
    # reference's run meets first at each of the same counts (pcg_reference.geometric_tau), with the margin condition
    for what, start, b2, x2 in _inputs(pr, b_res)[1:]:
        ref2 = _run_reference(pr, pre, what, start, b2, x2, lmax)
        rn2, bn2 = ref2[1], np.linalg.norm(b2)
        for want in P.TAU_AT[pre]:
            tau = P.geometric_tau(rn2, bn2, want, rounded=False)
            assert P.first_converged(rn2, tau * bn2) == want
            assert all(P.margin(rn2[k], tau * bn2, P.E_R[pre][k]) for k in range(want + 1))
            rc, its, res, x, polls, _ = _solve(G, b2, x2, tau, 400)
            assert rc == 0 and its == want, (what, start, tau, rc, its, want)
            assert res <= tau * bn2
            _check_iterate(form, "%s %s/%s converged at tau %.1e" % (name, what, start, tau), pr, pre, its, res, x, ref2)
            assert polls == _polls(pre, small, its, 400), (its, polls)
    tau, want = P.TAU[name, pre][-1], counts[-1]
    rc, its, res, x, _, _ = _solve(G, b, x0, tau, want)
    assert rc == 0 and its == want
    _check_iterate(form, "%s max_it == its" % name, pr, pre, its, res, x, ref)
    rc, its, res, x, _, _ = _solve(G, b, x0, tau, want - 1)
    assert rc == M.MI_ENOCONV_LIN and its == want - 1
    _check_iterate(form, "%s max_it == its - 1" % name, pr, pre, its, res, x, ref)
    # a start that satisfies the rule already: the tightest tolerance's solution under the loosest tolerance
    tau = P.TAU[name, pre][0]
    start = P.distribute(xs[counts[-1]], pr.m.constrained)
    r0 = b - pr.A @ start
    assert np.linalg.norm(r0) < 0.9 * tau * bnorm
    rc, its, res, x, polls, _ = _solve(G, b, start, tau, 400)
    assert rc == 0 and its == 0 and np.array_equal(x, start)
    # |fl(b - A x) - (b - A x)| <= (m + 1) eps (|A| |x| + |b|) entry by entry, m the longest row
    m = int(np.diff(pr.A.indptr).max())
    bound = (m + 1) * EPS * np.linalg.norm(abs(pr.A) @ np.abs(start) + np.abs(b)) / np.linalg.norm(r0)
    print("    %s its == 0: res %.1e of |r0| (bound %.1e)" % (name, abs(res - np.linalg.norm(r0)) / np.linalg.norm(r0), bound))
    assert abs(res - np.linalg.norm(r0)) <= bound * np.linalg.norm(r0)
    assert polls == _polls(pre, small, 0, 400)
    _report(form)


# ------------------------------------------------------------------ (a) - (c), one slab
@pytest.mark.parametrize("fused,variant", [(1, 3), (0, 3), (1, 1), (0, 1)])
@pytest.mark.parametrize("name", ["2d_q2_186", "q2_432_distorted"])
def test_jacobi_three_launches(name, fused, variant):
    """cg_update_p, the product with the fused p.q partials or dot_partials, cg_update_xr, cg_final_check at the batch end"""
    G, pr = _context(name, 0, [("small_cg", 0), ("cg_fused_dot", fused), ("spmv_variant", variant)])
    assert G.get_tuning("spmv_variant") == variant and G.get_tuning("precond") == 0
    b_res, _ = _assemble(G, pr, 0)
    _protocol(G, pr, "jacobi", None, b_res, P.K_JACOBI, "Jacobi three launches")
    G.close()


@pytest.mark.parametrize("name", sorted(P.SMALL) + sorted(P.SMALL.values()))
def test_jacobi_one_launch_and_the_next_size_above(name):
    """cg_small<2 | 3> under SMALL_CG_MAX_MATRIX_BYTES (no host synchronisation is counted for a solve); the next size takes the
    three-launch path under the same key and matches the same way"""
    c = P.MESHES[name]
    small = name in P.SMALL
    assert (P.sell_matrix_bytes(c["dim"], c["p"], c["reps"]) <= P.SMALL_CG_MAX_MATRIX_BYTES) == small
    G, pr = _context(name, 0, [("small_cg", 1)])
    b_res, _ = _assemble(G, pr, 0)
    _protocol(G, pr, "jacobi", None, b_res, P.K_SMALL, "Jacobi one launch" if small else "Jacobi, next size above", small=small)
    G.close()


@pytest.mark.parametrize("name", ["q2_543_mf_fine", "q3_532_rule5"])
def test_jacobi_on_the_matrix_free_product(name):
    """ "fine_level" 1: q = K p by mf_spmv / mf_spmv_q3 with the gathers' p.q partials, the diagonal from the point records"""
    G, pr = _context(name, 0)
    b_res, _ = _assemble(G, pr, 0)
    _protocol(G, pr, "jacobi", None, b_res, P.K_JACOBI, "Jacobi, matrix-free product")
    G.close()


@pytest.mark.parametrize("single", [0, 1], ids=["standard", "single_reduction"])
@pytest.mark.parametrize("name", ["q2_654", "q2_543_mf_fine", "q3_532_rule5", "2d_q2_186"])
def test_vcycle_pcg_on_one_slab(name, single):
    """mg_apply + dot_partials + cg_update_p / cg_update_xr, or cg_update_single with s = w + beta s standing for A p"""
    G, pr = _context(name, 1, [("cg_single_reduction", single)])
    assert G.get_tuning("cg_single_reduction_active") == single
    b_res, lmax = _assemble(G, pr, 1)
    _protocol(G, pr, "vcycle", lmax, b_res, P.K_VCYCLE, "V-cycle %s" % ("single reduction" if single else "standard"))
    G.close()


# ------------------------------------------------------------------ (c) teams
TEAMS = ["q2_4412_3slabs_z", "q2_1244_2slabs_x", "q2_4416_induced"]


@pytest.mark.parametrize("form", ["jacobi", "standard", "single"])
@pytest.mark.parametrize("name", TEAMS)
def test_pcg_on_teams(name, form):
    """totals through reduce_to_totals + team_allreduce; in the single form |b|^2 arrives with the first iteration's reduction.
    The reference is numpy throughout and knows nothing of slabs."""
    pre = "jacobi" if form == "jacobi" else "vcycle"
    keys = [] if form == "jacobi" else [("cg_single_reduction", 0 if form == "standard" else -1)]
    G, pr = _context(name, int(pre == "vcycle"), keys)
    c = P.MESHES[name]
    assert G.comm_info()[0] == c["slabs"] > 1 and G.get_tuning("cut_axis") == c["cut_axis"]
    if pre == "vcycle":
        assert G.get_tuning("cg_single_reduction_active") == int(form == "single")
    b_res, lmax = _assemble(G, pr, int(pre == "vcycle"))
    _protocol(G, pr, pre, lmax, b_res, P.K_JACOBI if pre == "jacobi" else P.K_VCYCLE, "teams, %s" % form)
    # scalar all-reduces of a truncated run of k iterations, from cg_run: Jacobi one for the initial totals, then p.Ap and
    # {||r||^2, r.z} per iteration; standard recurrence r.z (after each V-cycle), p.Ap and ||r||^2 per iteration; single
    # reduction THE reduction and the polled check per iteration
    k = 5
    n = _solve(G, pr.rhs("smooth"), pr.x0("zero"), 0.0, k)[5]
    print("    scalar all-reduces of %d iterations, %s: %d" % (k, form, n))
    assert n == dict(jacobi=2 * k + 1, standard=3 * k, single=2 * k)[form]
    G.close()


# ------------------------------------------------------------------ (d) predicted start and speculation
def _sequence(pr, taus):
    """(tag, b, tau, max_it, keys set before the solve): see the module docstring"""
    bs, br = pr.rhs("smooth"), pr.rhs("rough")
    b3 = -0.7 * bs + 0.05 * br
    b4 = b3 + 1e-4 * np.abs(bs).max() * np.random.default_rng(3).standard_normal(pr.m.n) * pr.free
    t0, t1 = taus
    return [("first", bs, t0, 400, []), ("later", br, t1, 400, []), ("on it", b3, t1, 400, []), ("early", b4, t1, 400, []),
            ("again", bs, t0, 400, []), ("margin 1", br, t1, 400, [("cg_speculate_margin", 1)]),
            ("two histories", b3, t1, 400, [("cg_warm_start", 3)]), ("truncated", bs, 0.0, 3, [])]


SPECULATED = {"q2_654": (1e-8, 1e-10), "q2_543_mf_fine": (1e-3, 1e-4), "q2_4412_3slabs_z": (1e-8, 1e-10)}


@pytest.mark.parametrize("name", sorted(SPECULATED))
def test_predicted_start_and_speculation(name):
    """every solve follows mi_newton_begin_step, so all but the first start from alpha h (scale_start) and enqueue
    expected - margin iterations without a poll; q2_543_mf_fine forms A h matrix-free from the point records"""
    runs = {}
    lmax = None
    for speculate in (1, 0):
        G, pr = _context(name, 1, [("cg_speculate", speculate)])
        b_res, lm = _assemble(G, pr, 1)
        assert lmax is None or lm == lmax
        lmax = lm
        G.set_tuning("cg_warm_start", 2)
        out = []
        for tag, b, tau, max_it, keys in _sequence(pr, SPECULATED[name]):
            for k, v in keys:
                G.set_tuning(k, v)
            G.newton_begin_step()
            G.set(M.V_RHS, b)
            s0 = G.get_tuning("count_cg_host_sync")
            rc, its, res = G.cg_solve(tau, max_it)
            out.append((rc, its, res, G.get(M.V_NEWTON), G.get_tuning("count_cg_host_sync") - s0))
        runs[speculate] = out
        G.close()
    A = P.Matrix(pr.A)
    form = "speculated, %s" % ("one slab" if P.MESHES[name].get("slabs", 1) == 1 else "team")
    hist, expect, warm, margin, seen = [], 0, 2, 2, set()
    for i, (tag, b, tau, max_it, keys) in enumerate(_sequence(pr, SPECULATED[name])):
        warm = dict(keys).get("cg_warm_start", warm)
        margin = dict(keys).get("cg_speculate_margin", margin)
        if not hist:
            x0 = np.zeros(pr.m.n)
        else:
            x0 = P.predicted_start(A, b, hist[0], hist[1] if warm == 3 and len(hist) > 1 else None)
        ref = pr.run("vcycle", b, x0, P.K_MAX["vcycle"], lmax)
        rn, bnorm = ref[1], np.linalg.norm(b)
        want = min(max_it, P.first_converged(rn, tau * bnorm)) if tau > 0 else max_it
        assert tau == 0 or all(P.margin(rn[k], tau * bnorm, P.E_R["vcycle"][k]) for k in range(want + 1))
        window = min(max_it - 1, expect - margin)  # iterations enqueued without a test
        rc, its, res, x, polls = runs[1][i]
        print("    %s %-13s its %d (reference %d, expected %d, unpolled %d), polls %d against %d, |b| / |r0| %.1e" %
              (name, tag, its, want, expect, max(window, 0), polls, runs[0][i][4], bnorm / rn[0]))
        assert rc == (0 if tau > 0 else M.MI_ENOCONV_LIN) and its == want, (tag, rc, its, want)
        _check_iterate(form, "%s %s" % (name, tag), pr, "vcycle", its, res, x, ref, kappa=bnorm / rn[0])
        # the same bits without speculation (include/mi_elasticity.h, "cg_speculate")
        rc0, its0, res0, x0_, polls0 = runs[0][i]
        assert (rc0, its0, res0) == (rc, its, res) and np.array_equal(x0_, x), tag
        # iterations 1 .. window are enqueued without a test; a solve that ends inside the window is noticed at the first poll
        assert polls0 == max(1, its) and polls == max(1, its - max(window, 0)), (tag, polls, polls0, window)
        if window >= 1:
            assert polls < polls0 or polls0 == 1, (tag, polls, polls0)
            seen.add("early" if want < window else "later" if want > expect else "on it" if expect - want <= 1 else "other")
        if tag == "truncated":
            assert window == max_it - 1 >= 1 and polls == 1  # (inside the window: only its last iteration is polled)
        if rc == 0:  # (a solve that did not converge predicts nothing)
            hist = [P.distribute(ref[0][want], pr.m.constrained)] + hist[:1]
            expect = want
        else:
            expect = 0
    _report(form)
    assert {"later", "on it", "early"} <= seen, seen


# ------------------------------------------------------------------ (e) the linear model
@pytest.mark.parametrize("geom,operator", [((2, 3, "distorted", (3, 2), "c"), 0), ((3, 3, "distorted", (2, 1, 2), "a"), 1)],
                         ids=["assembled_2d_q3", "matrix_free_3d_q3"])
def test_linear_model_steps_count_the_reference_iterations(geom, operator):
    """mi_linear_step: Jacobi-PCG on the stepping matrix from the previous velocity to an absolute tolerance.  The tolerance of
    a step is chosen from the reference's run (between ||r_12|| and the smallest residual before it), so that the count is 12
    with a margin; the mirror takes the device's d and v after each step, as in test_gpu_linear_model_reference.py."""
    import test_gpu_linear_model_reference as TL
    G, ref = TL._context(geom, TL.ROLES_A, operator, body=True)
    L = TL._fresh(ref, True)
    m, dim, dt, th = L.m, L.m.dim, L.dt, L.theta
    ids, free = m.interface_nodes, ~m.constrained
    rng = np.random.default_rng(7)
    v0, d0 = rng.standard_normal(m.n) * free, rng.standard_normal(m.n) * free
    v0 /= np.abs(L.M @ v0).max()
    d0 /= dt * np.abs(L.K @ d0).max()
    L.v[:], L.d[:] = v0, d0
    G.set(TL.L_V, v0)
    G.set(TL.L_D, d0)
    A = sp.csr_matrix(L.system_matrix())
    form = "linear model, %s" % ("matrix-free" if operator else "assembled")
    for step in range(3):
        t = rng.standard_normal((len(ids), dim))
        TL._set_stress(L, t)
        t /= dt * th * np.abs(L.consistent_load()).max()
        TL._set_stress(L, t)
        G.set_interface_traction(t)
        start = L.v.copy()
        rhs = L.step(True)
        xs, rn, _, _ = P.pcg(P.Matrix(A), P.jacobi(A), rhs, start, P.K_MAX["jacobi"])
        want = 12
        tol = float("%.1e" % np.sqrt(rn[want] * rn[:want].min()))
        assert P.first_converged(rn, tol) == want and all(P.margin(rn[k], tol, P.E_R["jacobi"][k]) for k in range(want + 1))
        its, res = G.linear_step(True, tol)
        er = abs(res - rn[want]) / rn[want]
        ev = _relmax(G.get(TL.L_V), P.distribute(xs[want], m.constrained))
        print("    step %d: its %d (reference %d), res %.1e, v %.1e" % (step, its, want, er, ev))
        assert its == want and res <= tol
        assert er <= P.tol_r("jacobi", want) and ev <= P.tol_x("jacobi", want)
        _record(form, "jacobi", want, ev, er)
        L.d[:], L.v[:] = G.get(TL.L_D), G.get(TL.L_V)
    _report(form)
    G.close()
