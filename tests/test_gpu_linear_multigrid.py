"""GPU: the linear model's multigrid-preconditioned CG (tuning key "linear_precond" 1) against the numpy reference of
tests/golden/linear_mg_reference.py, in both forms of "linear_operator".

  1  the key: default, read-backs, back to 0, refused on a team, the default path's bits;
  2  the hierarchy per case and form: shape, lmax bounds (first estimates: lambda_true <= lmax <= 1.15 lambda_true (1 + 1e-10)),
     level matrices and diagonal blocks through the borrowed level contexts to 1e-12 (the matrix-free fine level: its product),
     the block hook repeatable across two set-ups;
  3  the cycle: linear_apply(3, r) against ref.vcycle(r, lmax of the device) to TOL for three right-hand sides, same bits twice;
  4  the iteration: three steps whose tolerance is chosen from the reference's own multigrid-PCG so that the count is 6 with a
     margin; count, residual and velocity against the reference's r_6 and x_6;
  5  steps against the mirror's direct solves to 1e-7, with fewer iterations than a Jacobi context on the same inputs;
  6  co-existence with the tangent's hierarchy: a nonlinear solve gives the same bits before and after linear steps.

TOL (3): 64 x the worst rounding of the reference itself (float64 against long double cycle, linear_mg_reference.E_LIN = 5.0e-15
over a measured 3.19e-15, tests/test_mirror_linear_multigrid.py on these very cases), rounded up to the next power of ten: 1e-12.
(4): 64 x the float64-against-long-double difference of the reference's own PCG at iteration 6, computed in the test, and not
below 1e-13.
"""
import functools
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

TOL = 10.0 ** math.ceil(math.log10(64 * LR.E_LIN))
TOL_OP = 1e-12  # matrices, products and diagonal blocks (test_gpu_linear_model_reference.py)
FORMS = [(name, op) for name, c in LR.CASES.items() for op in ((0, 1) if c["dim"] == 3 and c["p"] == 3 else (0,))]
IDS = ["%s-%s" % (n, "matrix_free" if o else "assembled") for n, o in FORMS]


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _context(name, operator, precond=1, body=False, setup=True, **kw):
    c = LR.CASES[name]
    lo, hi, perturb = LR.case_geometry(name)
    bf = tuple(LR.BODY[:c["dim"]]) + (0.0,) * (3 - c["dim"]) if body else (0.0, 0.0, 0.0)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb,
                  body_force=bf, delta_t=LR.DT, **kw)
    if operator:
        G.set_tuning("linear_operator", 1)
    if precond:
        G.set_tuning("linear_precond", 1)
    if setup:
        G.linear_setup(LR.THETA)
        assert G.get_tuning("linear_operator_active") == operator and G.get_tuning("linear_precond_active") == precond
    return G


@functools.lru_cache(maxsize=None)
def _lambda_true(name, level):
    return LR.reference(name).lambda_true(level)


def _device_lmax(G, ref):
    return [G.linear_mg_level_describe(l)["lmax"] for l in range(len(ref.shape))]


# ------------------------------------------------------------------ 1
def _three_steps(G, seed=3):
    import test_gpu_linear_model_reference as TL
    rng = np.random.default_rng(seed)
    k = len(G.interface()[0])
    free = ~G.constrained
    G.set(TL.L_V, rng.standard_normal(G.n) * free)
    out = [G.linear_diagonal()]
    for step in range(3):
        G.set_interface_traction(1e3 * rng.standard_normal((k, G.dim)))
        its, res = G.linear_step(step != 1, 1e-9)
        out += [np.array([its, res]), G.get(TL.L_D), G.get(TL.L_V)]
    return out


def test_key_semantics():
    name = "q3_212"
    G = _context(name, 1, precond=0, setup=False)
    assert G.get_tuning("linear_precond") == 0 and G.get_tuning("linear_precond_active") == 0
    G.set_tuning("linear_precond", 1)
    assert G.get_tuning("linear_precond") == 1 and G.get_tuning("linear_precond_active") == 0  # read by the next set-up
    assert G.linear_mg_n_levels() == 0
    G.linear_setup(LR.THETA)
    assert G.get_tuning("linear_precond_active") == 1 and G.linear_mg_n_levels() == 2
    r = np.random.default_rng(0).standard_normal(G.n) * ~G.constrained
    assert np.all(np.isfinite(G.linear_apply(3, r)))
    n_refresh = G.get_tuning("count_mg_refresh")
    its_mg, _ = G.linear_step(True, 1e-9)
    assert G.get_tuning("count_mg_refresh") == n_refresh
    G.set_tuning("linear_precond", 0)
    assert G.get_tuning("linear_precond_active") == 1  # until the next set-up
    G.linear_setup(LR.THETA)
    assert G.get_tuning("linear_precond_active") == 0 and G.linear_mg_n_levels() == 0
    with pytest.raises(M.MiError) as e:
        G.linear_apply(3, r)
    assert e.value.code == M.MI_EINVAL
    with pytest.raises(M.MiError) as e:
        G.linear_mg_level_describe(0)
    assert e.value.code == M.MI_EINVAL
    # the default path: a context that went through 1 and back gives the bits of one that never heard of the key
    fresh = _context(name, 1, precond=0)
    for a, b in zip(_three_steps(G), _three_steps(fresh)):
        assert np.array_equal(a, b)
    G.close()
    fresh.close()
    # refused on a team before anything changes; the team then sets up and steps with Jacobi
    S = _context("q1_987", 0, precond=0, setup=False, slabs=2)
    with pytest.raises(M.MiError) as e:
        S.set_tuning("linear_precond", 1)
    assert e.value.code == M.MI_EINVAL and "linear_precond" in str(e.value)
    assert S.get_tuning("linear_precond") == 0
    S.linear_setup(LR.THETA)
    assert S.get_tuning("linear_precond_active") == 0 and S.linear_mg_n_levels() == 0
    one = _context("q1_987", 0, precond=0)
    k = len(S.interface()[0])
    t = np.random.default_rng(1).standard_normal((k, 3))
    for C in (S, one):
        C.set_interface_traction(t)
    its_s, its_1 = S.linear_step(True, 1e-9)[0], one.linear_step(True, 1e-9)[0]
    assert its_s > 1 and abs(its_s - its_1) <= 1  # Jacobi, as on one slab
    S.close()
    one.close()


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("name,operator", FORMS, ids=IDS)
def test_hierarchy_against_the_reference(name, operator):
    ref = LR.reference(name)
    G = _context(name, operator)
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
            lam = _lambda_true(name, l)
            print("level %d: lmax / lambda_true = %.6f" % (l, d["lmax"] / lam))
            assert lam <= d["lmax"] <= 1.15 * lam * (1 + 1e-10), (l, lam, d["lmax"])
        V = G if l == 0 else G.linear_mg_level_context(l)
        assert V.n == ref.A[l].shape[0] and np.array_equal(V.constrained, ref.meshes[l].constrained)
        if l == 0 and operator:  # no matrix: its product
            x = np.random.default_rng(l).standard_normal(G.n)
            err["A0 x"] = _relmax(G.linear_apply(2, x), ref.A[0] @ x)
        else:
            err["A%d" % l] = abs(V.linear_csr(2) - ref.A[l]).max() / abs(ref.A[l]).max()
        err["D%d" % l] = _relmax(V.linear_diagonal_blocks(), ref.D[l])
    print("%s form %d: relmax" % (name, operator), {k: "%.1e" % v for k, v in err.items()})
    assert all(e <= TOL_OP for e in err.values()), err
    D0 = G.linear_diagonal_blocks()
    G.linear_setup(LR.THETA)
    assert np.array_equal(G.linear_diagonal_blocks(), D0)
    G.close()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name,operator", FORMS, ids=IDS)
def test_cycle_against_the_reference(name, operator):
    import test_gpu_linear_model_reference as TL
    ref = LR.reference(name)
    G = _context(name, operator)
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
        print("%s form %d %-6s relmax %.2e" % (name, operator, tag, e))
        worst = max(worst, e)
    assert worst <= TOL, worst
    G.close()


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("name,operator", [("q3_212", 1), ("2d_q2_186", 0)], ids=["q3_212-matrix_free", "2d_q2_186-assembled"])
def test_steps_count_the_reference_iterations(name, operator):
    import test_gpu_linear_model_reference as TL
    ref = LR.reference(name)
    G = _context(name, operator, body=True)
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


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("name,operator,body", [("q3_532", 1, True), ("q2_644", 0, False)],
                         ids=["q3_532-matrix_free-body_force", "q2_644-assembled"])
def test_steps_against_the_mirror_with_fewer_iterations(name, operator, body):
    """_run_steps of test_gpu_linear_model_reference.py with a Jacobi context beside the preconditioned one: the same state and
    interface data on both, d and v of the preconditioned one against the mirror's direct solves"""
    import test_gpu_linear_model_reference as TL
    ref = LR.reference(name)
    G, J = _context(name, operator, body=body), _context(name, operator, precond=0, body=body)
    L = TL._fresh(ref.linear, body)
    m, dim, dt, th = L.m, L.m.dim, L.dt, L.theta
    ids, free = m.interface_nodes, ~m.constrained
    rng = np.random.default_rng(sum(m.reps) + int(body))
    v0, d0, f0 = rng.standard_normal(m.n) * free, rng.standard_normal(m.n) * free, rng.standard_normal(m.n)
    v0 /= np.abs(L.M @ v0).max()
    d0 /= dt * np.abs(L.K @ d0).max()
    f0 /= dt * (1 - th) * np.abs(f0).max()
    L.v[:], L.d[:], L.f_old[:] = v0, d0, f0
    for C in (G, J):
        C.set(TL.L_V, v0)
        C.set(TL.L_D, d0)
        C.set(TL.L_F_OLD, f0)
    for step in range(3):
        consistent = step != 1
        t = rng.standard_normal((len(ids), dim))
        TL._set_stress(L, t)
        t /= dt * th * np.abs(L.consistent_load() if consistent else L.stress).max()
        TL._set_stress(L, t)
        rhs = L.step(consistent)
        scale = np.abs(rhs).max()
        out = []
        for C in (G, J):
            C.set_interface_traction(t)
            out.append(C.linear_step(consistent, 1e-13 * scale))
        (its, res), (its_j, res_j) = out
        e = {"rhs": np.abs(G.get(TL.L_RHS) - rhs).max() / scale, "d": _relmax(G.get(TL.L_D), L.d), "v": _relmax(G.get(TL.L_V), L.v)}
        print("    step %d: its %d (Jacobi %d), %s" % (step, its, its_j, {k: "%.1e" % v for k, v in e.items()}))
        assert res <= 1e-13 * scale and res_j <= 1e-13 * scale
        assert e["rhs"] <= TL.TOL and e["d"] <= TL.TOL_SOL and e["v"] <= TL.TOL_SOL, (step, e)
        assert 1 < its < its_j
        L.d[:], L.v[:] = G.get(TL.L_D), G.get(TL.L_V)
        J.set(TL.L_D, L.d)
        J.set(TL.L_V, L.v)
    G.close()
    J.close()


# ------------------------------------------------------------------ 6
def test_linear_steps_leave_the_tangent_hierarchy_alone():
    """3D Q2 with "precond" 1: a nonlinear assemble + solve, a linear set-up with the key at 1 and two steps, the linear model
    back at the key's 0, then the same assemble + solve from the same state.  Both solves start from a hierarchy whose estimates
    are made from scratch ("mg_coarsest" set again rebuilds it), so x and the count must have the bits of the first run -- and
    of a second context that runs the two solves without the linear model in between."""
    import test_gpu_linear_model_reference as TL
    reps, hi = (5, 4, 3), (0.5, 0.4, 0.3)
    m = Mi.Mesh(3, 2, reps, (0.0, 0.0, 0.0), hi, R.ROLES_A)
    u, du = R.case_state(m, seed=4)

    def nonlinear(C):
        C.set_tuning("mg_coarsest", 4)
        for v in range(10):  # (the linear model's vectors are the context's: every one is set again)
            C.set(v, np.zeros(C.n))
        C.set_interface_traction((0.0, -1e3, 200.0))
        C.newton_begin_step()
        C.set(M.V_U, u)
        C.set(M.V_DELTA, du)
        C.update_acceleration()
        assert np.isfinite(C.assemble())
        C.set(M.V_NEWTON, np.zeros(C.n))
        rc, its, res = C.cg_solve(1e-8, 400)
        assert rc == 0
        return its, res, C.get(M.V_NEWTON)

    G, H = (M.Context(dim=3, degree=2, reps=reps, hi=hi, face_role=R.ROLES_A, delta_t=LR.DT) for _ in range(2))
    for C in (G, H):
        C.set_tuning("precond", 1)
    first, first_h = nonlinear(G), nonlinear(H)
    assert first[0] > 1 and G.mg_n_levels() == 3
    n_refresh = G.get_tuning("count_mg_refresh")
    G.set_tuning("linear_precond", 1)
    G.linear_setup(LR.THETA)
    assert G.get_tuning("linear_precond_active") == 1 and G.linear_mg_n_levels() == 3 and G.mg_n_levels() == 3
    rng = np.random.default_rng(2)
    G.set(TL.L_V, rng.standard_normal(G.n) * ~G.constrained)
    for _ in range(2):
        its, _ = G.linear_step(True, 1e-8)
        assert its > 1
    assert G.get_tuning("count_mg_refresh") == n_refresh
    G.set_tuning("linear_precond", 0)
    G.linear_setup(LR.THETA)
    second, second_h = nonlinear(G), nonlinear(H)
    for a, b in ((first, second), (first_h, second_h), (second, second_h)):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    G.close()
    H.close()
