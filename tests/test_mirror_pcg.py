"""CPU: the numpy PCG of tests/golden/pcg_reference.py, anchored and measured before any GPU test trusts it.

  * pcg() against scipy.sparse.linalg.cg with a callback, iterate by iterate through 10 iterations, on one Jacobi case and
    one V-cycle case (relmax <= 1e-10; measured 0 on both: the same operations in the same order), and its recursive residual against b - A x_k;
  * first_converged(), predicted_start() and sell_nblk64() on inputs small enough to check by hand;
  * the reference's own rounding: float64 against long double on every case, input and iteration the GPU test uses.  The
    committed tables pcg_reference.E_X / E_R are the running maximum over k of what is measured here, rounded up in the second
    digit: the test asserts measurement <= table <= 1.12 x that envelope;
  * the conditions of the GPU test for the reference alone: every tau of pcg_reference.TAU converges at the iteration it was
    chosen for (Jacobi: inside a batch, on its % 16 == 0 and on its % 16 == 1), and no ||r_k|| / (tau ||b||), k <= its, lies
    within the margin [1 / (1 + g), 1 + g], g = max(1e-6, 1e3 E_r(k)): the iteration count is one number;
  * the one-launch cases lie under SMALL_CG_MAX_MATRIX_BYTES and their neighbours above it.

Measured (running maximum over k): V-cycle PCG E_x <= 1.9e-15 and E_r <= 2.0e-13 for k <= 14 (1.6e-14 at k = 7); Jacobi-PCG
E_x 3.3e-15 at k = 17 and 1.5e-10 at k = 33, E_r 1.2e-13 at k = 17 and 2.7e-07 at k = 33 (white noise on the two 3D meshes of a
few hundred dofs, on which 33 iterations are a tenth of the Krylov space, loses orthogonality first).  V-cycle runs take 1.15
lambda_true for the device's lmax.  Not measured here: the assembly's own residual (the mirror's assembly is a dense Python
loop, minutes on the larger cases), the predicted starts of (d) and the linear model's steps of (e); the GPU test holds them
to the tolerances of these tables.
"""
import inspect
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pcg_reference as P  # noqa: E402


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name,pre", [("2d_q2_186", "jacobi"), ("q2_543_mf_fine", "vcycle")])
def test_iterates_are_those_of_scipy(name, pre):
    pr = P.problem(name)
    lmax = pr.lmax_cpu() if pre == "vcycle" else None
    b, x0, K = pr.rhs("smooth"), pr.x0("random"), 10
    xs, rn, alpha, beta = pr.run(pre, b, x0, K, lmax)
    assert len(xs) == K + 1 and len(alpha) == len(beta) == K and np.all(alpha > 0) and np.all(beta > 0)
    Minv = pr.preconditioner(pre, lmax)
    seen = []
    no_stop = {"rtol": 0.0, "atol": 0.0} if "rtol" in inspect.signature(spla.cg).parameters else {"tol": 0.0, "atol": 0.0}
    spla.cg(pr.A, b, x0=x0.copy(), maxiter=K, M=spla.LinearOperator(pr.A.shape, matvec=Minv, dtype=float),
            callback=lambda x: seen.append(x.copy()), **no_stop)
    assert len(seen) == K
    worst = max(_relmax(xs[k + 1], seen[k]) for k in range(K))
    print("%s %s: worst relmax of 10 iterates against scipy %.1e" % (name, pre, worst))
    assert worst <= 1e-10
    assert np.array_equal(xs[0], x0)
    for k in range(K + 1):  # the recursive residual is the true one while it is far above the rounding of b - A x
        assert abs(rn[k] - np.linalg.norm(b - pr.A @ xs[k])) <= 1e-10 * np.linalg.norm(b)
        assert not xs[k][pr.m.constrained].any()


def test_small_things_by_hand():
    assert P.first_converged([3.0, 5.0, 1.0, 0.5, 0.7], 1.0) == 2  # (<=, and the first, not the last)
    assert P.first_converged([3.0, 5.0], 1.0) is None and P.first_converged([0.5, 5.0], 1.0) == 0
    A = np.diag([2.0, 4.0])
    h, b = np.array([1.0, 1.0]), np.array([3.0, 3.0])
    assert np.allclose(P.predicted_start(lambda x: A @ x, b, h), h)  # h.b / h.Ah = 6 / 6
    assert np.allclose(P.predicted_start(lambda x: A @ x, b, h, h0=np.array([1.0, 2.0])), [1.5, 0.0])  # 2 h1 - h0 = (1, 0): 3 / 2 of it
    assert np.all(P.predicted_start(lambda x: -A @ x, b, h) == 0)
    assert not P.margin(1.0 + 5e-7, 1.0, 0.0) and P.margin(1.0 + 2e-6, 1.0, 0.0) and not P.margin(1.0 + 2e-6, 1.0, 1e-8)
    # one Q1 cell in 2D: four rows of length 4 and x-width 2, one class, one slice of length 4
    assert P.sell_nblk64(2, 1, (1, 1)) == 4
    # 2 x 1 Q1 cells: the four end nodes couple 4 nodes, the two middle ones 6 (x-width 3): slices of length 4 and 6
    assert P.sell_nblk64(2, 1, (2, 1)) == 10
    for small, above in P.SMALL.items():
        a, b = P.MESHES[small], P.MESHES[above]
        assert P.sell_matrix_bytes(a["dim"], a["p"], a["reps"]) <= P.SMALL_CG_MAX_MATRIX_BYTES
        assert P.sell_matrix_bytes(b["dim"], b["p"], b["reps"]) > P.SMALL_CG_MAX_MATRIX_BYTES


@pytest.mark.parametrize("pre", ["jacobi", "vcycle"])
def test_reference_rounding_is_the_committed_table(pre):
    assert np.finfo(np.longdouble).eps < 1e-18
    K = P.K_MAX[pre]
    assert len(P.E_X[pre]) == len(P.E_R[pre]) == K + 1
    assert K >= max(P.K_JACOBI + P.K_SMALL if pre == "jacobi" else P.K_VCYCLE)
    ex, er = np.zeros(K + 1), np.zeros(K + 1)
    for name in P.CASES_OF[pre]:
        for what, start in P.INPUTS:
            a, b = P.measure_rounding(name, pre, what, start)
            assert np.all(a <= P.E_X[pre]) and np.all(b <= P.E_R[pre]), (name, what, start, a.max(), b.max())  # (a NaN fails)
            ex, er = np.maximum(ex, a), np.maximum(er, b)
    print("E_X %s:" % pre, ", ".join("%.1e" % v for v in ex))
    print("E_R %s:" % pre, ", ".join("%.1e" % v for v in er))
    # the tables are the running maximum of this measurement, rounded up in the second digit (floor 1e-16), not more
    ex, er = np.maximum.accumulate(ex), np.maximum.accumulate(er)
    assert np.all(np.array(P.E_X[pre]) <= np.maximum(1.12 * ex, 1e-16))
    assert np.all(np.array(P.E_R[pre]) <= np.maximum(1.12 * er, 1e-16))


@pytest.mark.parametrize("pre", ["jacobi", "vcycle"])
def test_every_tau_gives_one_iteration_count(pre):
    assert sorted(n for n, q in P.TAU if q == pre) == sorted(P.CASES_OF[pre])
    for name in P.CASES_OF[pre]:
        pr = P.problem(name)
        lmax = pr.lmax_cpu() if pre == "vcycle" else None
        b = pr.rhs("smooth")
        rn = pr.run(pre, b, pr.x0("zero"), P.K_MAX[pre], lmax, key=("smooth", "zero"))[1]
        counts = []
        for tau in P.TAU[name, pre]:
            tol = tau * np.linalg.norm(b)
            its = P.first_converged(rn, tol)
            assert its is not None and its >= 2
            for k in range(its + 1):
                assert P.margin(rn[k], tol, P.E_R[pre][k]), (name, pre, tau, k, rn[k] / tol)
            counts.append(its)
            assert abs(tau / P.geometric_tau(rn, np.linalg.norm(b), its) - 1) <= 0.06  # (how it was chosen, to two digits)
        print("%s %s: tau %s converge at %s" % (name, pre, P.TAU[name, pre], counts))
        assert tuple(counts) == P.TAU_AT[pre]
    if pre == "jacobi":  # inside a batch, at its end, and one past it
        a, b, c = P.TAU_AT[pre]
        assert 1 < a % P.CG_BATCH and b % P.CG_BATCH == 0 and c % P.CG_BATCH == 1
