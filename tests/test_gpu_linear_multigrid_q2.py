"""GPU: the linear model's multigrid-preconditioned CG ("linear_precond" 1) on a matrix-free Q2 fine level ("linear_operator" 2:
mf_linear_q2, D from mf_linear_diag_q2<., true> + mf_diag_gather) against the numpy reference of
tests/golden/linear_mg_reference.py: the checks that tests/test_gpu_linear_multigrid.py runs on its matrix-free forms, at that
file's tolerances (E_LIN was measured on q2_644 itself).

  q2_644    the reference's own case: graded boxes, 3 levels
  q2_212d   the smallest two-level case: 2 x 1 x 2 distorted cells (the general-geometry kernels), 4 cells = 2 full pairs

  1  the hierarchy: shape, lmax bounds, level 0's product and every D, the coarser levels' matrices through the borrowed level
     contexts, the block hook repeatable across two set-ups;
  2  one V-cycle, linear_apply(3, r), against ref.vcycle(r, lmax of the device) for three right-hand sides, same bits twice;
  3  three steps whose tolerance is chosen from the reference's own multigrid-PCG so that the count is 6 with a margin; count,
     residual and velocity against the reference's r_6 and x_6.
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import linear_mg_reference as LR  # noqa: E402
import mg_reference as R  # noqa: E402
import mirror as Mi  # noqa: E402
import pcg_reference as P  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

TOL = 10.0 ** math.ceil(math.log10(64 * LR.E_LIN))  # tests/test_gpu_linear_multigrid.py
TOL_OP = 1e-12
SMALL = dict(dim=3, p=2, reps=(2, 1, 2), kind="distorted", roles=R.ROLES_A)
NAMES = ["q2_644", "q2_212d"]
_small = {}


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _case(name):
    """the case's description, geometry and LinearReference (built once per process)"""
    if name == "q2_644":
        return LR.CASES[name], LR.case_geometry(name), LR.reference(name)
    c = SMALL
    geom = R.geometry(c["kind"], c["dim"], c["reps"], seed=sum(c["reps"]))
    if "ref" not in _small:
        lo, hi, perturb = geom
        _small["ref"] = LR.LinearReference(Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, c["roles"], perturb=perturb), body=LR.BODY)
    return c, geom, _small["ref"]


def _context(name, body=False):
    c, (lo, hi, perturb), ref = _case(name)
    G = M.Context(dim=3, degree=2, reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb,
                  body_force=tuple(LR.BODY) if body else (0.0, 0.0, 0.0), delta_t=LR.DT)
    G.set_tuning("linear_operator", 2)
    G.set_tuning("linear_precond", 1)
    G.linear_setup(LR.THETA)
    assert G.get_tuning("linear_operator_active") == 2 and G.get_tuning("linear_precond_active") == 1
    return G, ref


def _device_lmax(G, ref):
    return [G.linear_mg_level_describe(l)["lmax"] for l in range(len(ref.shape))]


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", NAMES)
def test_hierarchy_against_the_reference(name):
    G, ref = _context(name)
    m = ref.meshes[0]
    assert np.array_equal(G.constrained, m.constrained) and np.abs(G.coords - m.coords).max() < 1e-14
    assert G.linear_mg_n_levels() == len(ref.shape) >= 2
    err = {}
    for l, sh in enumerate(ref.shape):
        d = G.linear_mg_level_describe(l)
        print("level %d: %s" % (l, d))
        assert (d["degree"], d["reps"], d["n_dofs"]) == (sh["degree"], sh["reps"], sh["n_dofs"])
        assert (d["exact_solve"], d["smoother_degree"], d["interval_ratio"]) == (sh["exact"], sh["nu"], sh["ratio"])
        assert d["distributed"] == 0
        if sh["exact"]:
            assert d["lmax"] == 0.0
        else:
            lam = ref.lambda_true(l)
            print("level %d: lmax / lambda_true = %.6f" % (l, d["lmax"] / lam))
            assert lam <= d["lmax"] <= 1.15 * lam * (1 + 1e-10), (l, lam, d["lmax"])
        V = G if l == 0 else G.linear_mg_level_context(l)
        assert V.n == ref.A[l].shape[0] and np.array_equal(V.constrained, ref.meshes[l].constrained)
        if l == 0:  # no matrix: its product
            x = np.random.default_rng(l).standard_normal(G.n)
            err["A0 x"] = _relmax(G.linear_apply(2, x), ref.A[0] @ x)
        else:
            err["A%d" % l] = abs(V.linear_csr(2) - ref.A[l]).max() / abs(ref.A[l]).max()
        err["D%d" % l] = _relmax(V.linear_diagonal_blocks(), ref.D[l])
    print("%s: relmax" % name, {k: "%.1e" % v for k, v in err.items()})
    assert all(e <= TOL_OP for e in err.values()), err
    D0 = G.linear_diagonal_blocks()
    G.linear_setup(LR.THETA)
    assert np.array_equal(G.linear_diagonal_blocks(), D0)
    G.close()


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", NAMES)
def test_cycle_against_the_reference(name):
    import test_gpu_linear_model_reference as TL
    G, ref = _context(name)
    m = ref.meshes[0]
    lmax = _device_lmax(G, ref)
    free = ~m.constrained
    rng = np.random.default_rng(len(name))
    unit = np.zeros(m.n)
    unit[np.nonzero(free)[0][-1]] = 1.0
    G.set(TL.L_V, rng.standard_normal(m.n) * free)
    G.set_interface_traction(1e3 * rng.standard_normal((len(m.interface_nodes), m.dim)))
    G.linear_step(True, 1e-6)
    rhs = G.get(TL.L_RHS)
    assert np.abs(rhs).max() > 0 and not rhs[~free].any()
    worst = 0.0
    for tag, r in (("random", rng.standard_normal(m.n) * free), ("unit", unit), ("step", rhs)):
        z = G.linear_apply(3, r)
        assert np.all(np.isfinite(z)) and np.array_equal(G.linear_apply(3, r), z)
        e = _relmax(z, ref.vcycle(r, lmax))
        print("%s %-6s relmax %.2e" % (name, tag, e))
        worst = max(worst, e)
    assert worst <= TOL, worst
    G.close()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", NAMES)
def test_steps_count_the_reference_iterations(name):
    import test_gpu_linear_model_reference as TL
    G, ref = _context(name, body=True)
    lmax = _device_lmax(G, ref)
    L = TL._fresh(ref.linear, True)
    m, dim, dt, th = L.m, L.m.dim, L.dt, L.theta
    ids, free = m.interface_nodes, ~m.constrained
    rng = np.random.default_rng(7)
    v0, d0 = rng.standard_normal(m.n) * free, rng.standard_normal(m.n) * free
    v0 /= np.abs(L.M @ v0).max()
    d0 /= dt * np.abs(L.K @ d0).max()
    L.v[:], L.d[:] = v0, d0
    G.set(TL.L_V, v0)
    G.set(TL.L_D, d0)
    A = ref.A[0]
    want, K = 6, 14
    for step in range(3):
        t = rng.standard_normal((len(ids), dim))
        TL._set_stress(L, t)
        t /= dt * th * np.abs(L.consistent_load()).max()
        TL._set_stress(L, t)
        G.set_interface_traction(t)
        start = L.v.copy()
        rhs = L.step(True)
        xs, rn, _, _ = P.pcg(P.Matrix(A), P.vcycle(ref, lmax), rhs, start, K)
        xl, rl, _, _ = P.pcg(P.Matrix(A, np.longdouble), P.vcycle(ref, lmax, np.longdouble), rhs, start, K, np.longdouble)
        e_r = float(abs(rn[want] - rl[want]) / rl[want])
        e_x = float(np.abs(xs[want] - xl[want]).max() / np.abs(xl[want]).max())
        tol = float("%.1e" % np.sqrt(rn[want] * rn[:want].min()))
        assert P.first_converged(rn, tol) == want and all(P.margin(rn[k], tol, e_r) for k in range(want + 1))
        its, res = G.linear_step(True, tol)
        er = abs(res - rn[want]) / rn[want]
        ev = _relmax(G.get(TL.L_V), P.distribute(xs[want], m.constrained))
        print("    step %d: its %d (reference %d), res %.1e (reference's rounding %.1e), v %.1e (%.1e)" %
              (step, its, want, er, e_r, ev, e_x))
        assert its == want and res <= tol
        assert er <= max(64 * e_r, 1e-13) and ev <= max(64 * e_x, 1e-13)
        L.d[:], L.v[:] = G.get(TL.L_D), G.get(TL.L_V)
    G.close()
