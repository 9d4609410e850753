"""GPU: "smoother_quadrature_q3" 4 -- the multigrid smoother's fine-level operator A' of a 3D Q3 matrix-free level on the
element's full-order rule, 4 x 4 x 4 Gauss points (mf_records_q3s, mf_spmv_q3s), beside the assembly's 125-point rule.

The smoother only preconditions: a wrong A' changes iteration counts, not results, so no oracle test can see it.  The
product (mi_spmv under "spmv_as_smoother" 1) is therefore held to tests/golden/mirror.py's Operator at the rule the library
REPORTS ("smoother_quadrature_q3_active"), and on a deformed state it must lie far from the other rule's reference -- a
report that does not match the kernel that ran fails.  The 4-point reference applies the fold rule of the records kernel
(a point with det F <= 0 takes the undeformed state); the folded state is folded at the 4-point rule and valid at all 125
points of the assembly's.

Everything else the key must leave alone, bit for bit: residual, right-hand side, diagonal blocks, the CG's product.

Tolerance of the products, relmax = max |y - y_ref| / max |y_ref|: 1e-12 (fp64; the tolerance of
test_gpu_smoother_operator.py).  Observed worst (MI355X): 1.8e-14 for the 64-point rule; 4.6e-13 for the 125-point
rule on the folded state (det F = 0.04 at one of its points), 9.1e-15 on the others.
"""
import math
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg
from test_gpu_parity import _pair as _oracle_pair
from test_gpu_smoother_operator import A1, APART, ROLES_A, ROLES_B, _geometry, _relmax, _shear, _smoother_product
from test_host_gpu import _check_rows, _prm, _run_case, _scenario_desc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

KEY, ACTIVE = "smoother_quadrature_q3", "smoother_quadrature_q3_active"
TOL = 1e-12
TOL_SOL = 1e-8


def _pair(kind, reps, roles, seed, degree=3):
    lo, hi, perturb = _geometry(kind, reps, seed)
    G = M.Context(dim=3, degree=degree, reps=reps, lo=lo, hi=hi, face_role=roles, perturb=perturb)
    m = Mi.Mesh(3, degree, reps, lo, hi, roles, perturb=perturb)
    assert np.array_equal(G.constrained, m.constrained) and np.abs(G.coords - m.coords).max() < 1e-14
    return G, m


def _folded(m):
    """u_x = -7.04 (x - x_min) g(eta), g = eta (1 - eta)^2 in every cell's own eta along y (a cubic: Q3 holds it exactly):
    det F = 1 - 7.04 g is -0.04 at the 4-point rule's eta = 0.330 and +0.04 at the 5-point rule's nearest point 0.231"""
    X, p = m.coords, 3
    jy = (np.arange(m.nnodes) // m.nn[0]) % m.nn[1]
    yline = X[np.arange(m.nn[1]) * m.nn[0], 1]  # y of the node planes
    j0 = np.minimum(jy // p, (m.nn[1] - 1) // p - 1) * p  # the plane the node's cell starts at (the last plane: eta = 1)
    eta = (X[:, 1] - yline[j0]) / (yline[j0 + p] - yline[j0])
    u = np.zeros((m.nnodes, 3))
    u[:, 0] = -7.04 * (X[:, 0] - X[:, 0].min()) * eta * (1.0 - eta) ** 2
    return u.reshape(-1)


def _states(m, kind, rng):
    """(name, u, du, deformed): V_U and V_DELTA both non-zero, since the records read u + du"""
    free = ~m.constrained
    w = 1e-3 * rng.standard_normal(m.n) * free
    yield "undeformed", w, -w, False  # u + du = 0 exactly
    s = _shear(m.coords) * free
    yield "shear", 0.6 * s, s - 0.6 * s, True
    r = 0.03 * 0.07 * rng.standard_normal(m.n) * free
    yield "random", 0.6 * r, r - 0.6 * r, True
    if kind != "distorted":
        f = _folded(m) * free
        yield "folded", 0.5 * f, f - 0.5 * f, True


def _references(m, ut, x):
    """the two rules' products of x at the state ut, and whether the 4-point rule met a folded point / min det F at 125"""
    op5 = Mi.Operator(m, ut, alpha1=A1, nq=5)
    op4 = Mi.Operator(m, ut, alpha1=A1, nq=4, fold_to_identity=True, cdiag=op5.cdiag)
    return {4: op4(x), 5: op5(x)}, bool(op4.folded.any()), float(op5.detF.min())


def _set_state(G, u, du):
    G.set(M.V_U, u)
    G.set(M.V_DELTA, du)
    G.update_acceleration()
    rn = G.assemble()
    assert np.isfinite(rn)
    return rn


def _check(G, ref, x, deformed, expect):
    """the smoother's product of the assembled state against the reference at the reported rule; relmax"""
    q = G.get_tuning(ACTIVE)
    assert q == expect
    y = _smoother_product(G, x)
    err = _relmax(y, ref[q])
    print("    rule %d: relmax %.2e" % (q, err))
    assert err <= TOL, (q, err)
    if deformed:
        assert _relmax(y, ref[9 - q]) > APART
    return err


# (geometry, reps, roles).  mf_spmv_q3s runs four waves = four cells per workgroup: 1, 2, 4 (one full workgroup), 5 and 9
# (a multiple + 1: the last workgroup has one wave with a cell), 12 cells.  cube / graded: BOX instances (per-cell 1/h);
# distorted: the trilinear map
CASES = [
    ("cube", (1, 1, 1), ROLES_A),
    ("cube", (2, 1, 1), ROLES_B),
    ("cube", (2, 2, 1), ROLES_A),
    ("cube", (3, 2, 2), ROLES_B),
    ("cube", (5, 1, 1), ROLES_A),
    ("graded", (2, 3, 2), ROLES_B),
    ("distorted", (2, 1, 2), ROLES_A),
    ("distorted", (3, 3, 1), ROLES_B),
]


@pytest.mark.parametrize("kind,reps,roles", CASES)
def test_q3_smoother_product_matches_the_reference_at_the_reported_rule(kind, reps, roles):
    """key 4 and key 5 on the same mesh and states: each product to 1e-12 of the mirror at the rule the library reports,
    and more than 1e-6 from the other rule on every deformed state; the folded state folds at 4 points and not at 5"""
    ctx = {}
    for key in (4, 5):
        ctx[key], m = _pair(kind, reps, roles, seed=sum(reps))
        ctx[key].set_tuning("fine_level", 1)
        assert ctx[key].get_tuning(ACTIVE) == 5  # no 64-point records before an assembly
        ctx[key].set_tuning(KEY, key)
        assert ctx[key].get_tuning(KEY) == key
    rng = np.random.default_rng(len(m.cells))
    worst = {4: 0.0, 5: 0.0}
    for name, u, du, deformed in _states(m, kind, rng):
        x = rng.standard_normal(m.n)
        ref, folded, detmin5 = _references(m, u + du, x)
        assert detmin5 > 0 and (folded or name != "folded")  # valid at all 125 points; the folded state folds at the 64
        if deformed:
            assert _relmax(ref[4], ref[5]) > 10 * APART
        for key, G in ctx.items():
            _set_state(G, u, du)
            worst[key] = max(worst[key], _check(G, ref, x, deformed, key))
    print("Q3 smoother product %s %s: worst relmax %.2e (64 points), %.2e (125 points)" % (kind, reps, worst[4], worst[5]))
    for G in ctx.values():
        G.close()


def test_q3_smoother_quadrature_touches_the_preconditioner_only():
    """key 4 against key 5 on the same distorted block and random state: the residual norm, the right-hand side, the diagonal
    blocks, the plain product and the residual-only pass are the same bits; the residual-only pass leaves A' alone"""
    reps, G = (3, 2, 2), {}
    for key in (4, 5):
        G[key], m = _pair("distorted", reps, ROLES_A, seed=11)
        G[key].set_tuning("fine_level", 1)
        G[key].set_tuning(KEY, key)
    rng = np.random.default_rng(12)
    r = 0.03 * 0.07 * rng.standard_normal(m.n) * ~m.constrained
    x = rng.standard_normal(m.n)
    out = {}
    for key, g in G.items():
        g.set_interface_traction((0.0, -1e3, 200.0))
        rn = _set_state(g, 0.6 * r, r - 0.6 * r)
        assert g.get_tuning(ACTIVE) == key
        rhs, D, y = g.get(M.V_RHS), g.diagonal_blocks(), g.spmv(x)
        ys = _smoother_product(g, x)
        rn2 = g.assemble_residual()
        assert np.array_equal(_smoother_product(g, x), ys) and g.get_tuning(ACTIVE) == key
        out[key] = (rn, rhs, D, y, rn2, g.get(M.V_RHS))
    for a, b in zip(out[4], out[5]):
        assert np.array_equal(a, b)
    for g in G.values():
        g.close()


def test_q3_smoother_quadrature_switching():
    """5 -> 4 -> 5 -> 4 between assemblies, the key before the level, the level off again, refused values, a Q2 context"""
    reps = (2, 1, 2)
    G, m = _pair("distorted", reps, ROLES_B, seed=3)
    rng = np.random.default_rng(4)
    s = _shear(m.coords) * ~m.constrained
    x = rng.standard_normal(m.n)
    ref, _, _ = _references(m, s, x)
    G.set_tuning("fine_level", 1)
    assert G.get_tuning(KEY) == 5
    for key in (5, 4, 5, 4):
        G.set_tuning(KEY, key)
        assert G.get_tuning(ACTIVE) == 5  # a change invalidates the 64-point records: the next product is a 125-point one
        _set_state(G, 0.6 * s, s - 0.6 * s)
        _check(G, ref, x, True, key)
    for bad in (3, 6):
        with pytest.raises(M.MiError):
            G.set_tuning(KEY, bad)
        assert G.get_tuning(KEY) == 4 and G.get_tuning(ACTIVE) == 4
    # the level off: the assembled level runs, nothing reports a Q3 rule; on again: the remembered key returns
    G.set_tuning("fine_level", 0)
    assert G.get_tuning(ACTIVE) == 0 and G.get_tuning(KEY) == 4
    _set_state(G, 0.6 * s, s - 0.6 * s)
    assert G.csr().nnz > 0 and np.all(np.isfinite(_smoother_product(G, x)))
    G.set_tuning("fine_level", 1)
    _set_state(G, 0.6 * s, s - 0.6 * s)
    _check(G, ref, x, True, 4)
    G.close()
    # the key BEFORE the level
    G, _ = _pair("distorted", reps, ROLES_B, seed=3)
    G.set_tuning(KEY, 4)
    assert G.get_tuning(ACTIVE) == 0
    G.set_tuning("fine_level", 1)
    _set_state(G, 0.6 * s, s - 0.6 * s)
    _check(G, ref, x, True, 4)
    G.close()
    # a Q2 context: accepted, no effect
    G, m2 = _pair("distorted", reps, ROLES_B, seed=3, degree=2)
    G.set_tuning("fine_level", 1)
    s2 = _shear(m2.coords) * ~m2.constrained
    _set_state(G, 0.6 * s2, s2 - 0.6 * s2)
    x2 = rng.standard_normal(m2.n)
    q2, y, ys = G.get_tuning("smoother_quadrature_active"), G.spmv(x2), _smoother_product(G, x2)
    G.set_tuning(KEY, 4)
    assert G.get_tuning(ACTIVE) == 0 and G.get_tuning(KEY) == 4 and G.get_tuning("smoother_quadrature_active") == q2
    assert np.array_equal(G.spmv(x2), y) and np.array_equal(_smoother_product(G, x2), ys)
    G.close()


@pytest.mark.parametrize("perturb_amp", [0.0, 0.05])
def test_q3_vcycle_on_the_64_point_smoother_is_spd(perturb_amp):
    """the construction of test_q3_matrix_free_multigrid_against_the_oracle with key 4: two Newmark steps against the
    oracle's CG + SSOR, then the V-cycle as an operator: symmetric to 1e-10 relative, positive"""
    roles = [O.FACE_CLAMPED, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_ZCLAMP, O.FACE_INTERFACE]
    P, G = _oracle_pair(3, 3, (4, 3, 3), perturb_amp=perturb_amp, seed=61, roles=roles)
    G.set_tuning("precond", 1)
    G.set_tuning("fine_level", 1)
    G.set_tuning(KEY, 4)
    for s in range(2):
        t = (0.0, -2e3 * (s + 1), 500.0)
        P.set_interface_traction(t)
        G.set_interface_traction(t)
        rc, info = G.newmark_step(tol_lin=1e-12, max_it_mult=2.0)
        rc_o, info_o = P.newmark_step(O.SOLVER_CG_SSOR, tol_lin=1e-12, max_it_mult=2.0)
        assert rc == 0 and rc_o == 0 and info.converged == 1
        assert _relmax(G.get(M.V_U), P.vec(O.V_U)) < TOL_SOL
    assert G.get_tuning(ACTIVE) == 4
    free = ~G.constrained

    def minv(r):
        G.set_tuning("spmv_as_smoother", 2)
        z = G.spmv(r)
        G.set_tuning("spmv_as_smoother", 0)
        return z

    rng = np.random.default_rng(5)
    r1, r2 = rng.standard_normal(G.n) * free, rng.standard_normal(G.n) * free
    z1, z2 = minv(r1), minv(r2)
    print("V-cycle asymmetry %.2e" % (abs(r2 @ z1 - r1 @ z2) / abs(r2 @ z1)))
    assert abs(r2 @ z1 - r1 @ z2) <= 1e-10 * abs(r2 @ z1) and r1 @ z1 > 0 and r2 @ z2 > 0
    G.close()


def _steps(key, lag):
    """_steps of test_gpu_q3_matrix_free.py on the matrix-free level, with the smoother's rule set"""
    G = M.Context(dim=3, degree=3, reps=(24, 12, 5), hi=(2.4, 1.2, 0.5))
    assert G.n > 75000 and G.get_tuning("precond") == 1  # (multigrid: the default above 75 k dofs)
    G.set_tuning("cg_warm_start", 2)
    G.set_tuning("fine_level", 1)
    G.set_tuning("mf_diag_lag", lag)
    G.set_tuning(KEY, key)
    out = []
    for s in range(3):
        G.set_interface_traction((0.0, -1e3 * (s + 1), 0.0))
        rc, info = G.newmark_step(tol_lin=1e-10, max_it_mult=2.0)
        assert rc == 0 and info.converged == 1 and G.get_tuning(ACTIVE) == key
        out.append((info.newton_iterations, list(info.lin_its)[:info.newton_iterations], G.get(M.V_U), G.get(M.V_V),
                    G.get(M.V_A)))
    G.close()
    return out


@pytest.mark.parametrize("lag", [0, 1])
def test_q3_newmark_steps_64_point_smoother_against_125(lag):
    """three Newmark steps of the 24 x 12 x 5-cell Q3 block (129,648 dofs, multigrid, the executable's warm start) with key 4
    and key 5: the same Newton iterations, u, v and a to 1e-8, and the CG iterations summed over the steps with key 4 at
    most 1.10 x those with key 5, rounded up (the kernel's expected gain is about 15 % of a step).
    Observed CG iterations per solve (MI355X), lag 0 and lag 1, key 4 and key 5 alike: 17 16 17 / 17 15 17 17 / 17 16 17 16 --
    identical, as they were for Q2's 27-point rule."""
    s4, s5 = _steps(4, lag), _steps(5, lag)
    print("lag %d CG iterations per solve: key 4 %s, key 5 %s" % (lag, [l for _, l, *_ in s4], [l for _, l, *_ in s5]))
    for (n4, _, u4, v4, a4), (n5, _, u5, v5, a5) in zip(s4, s5):
        assert n4 == n5
        assert _relmax(u4, u5) < TOL_SOL and _relmax(v4, v5) < TOL_SOL and _relmax(a4, a5) < TOL_SOL
    its4, its5 = sum(sum(l) for _, l, *_ in s4), sum(sum(l) for _, l, *_ in s5)
    assert its4 <= math.ceil(1.10 * its5), (its4, its5)


def test_q3_executable_64_point_smoother(tmp_path):
    """MI_FINE_LEVEL=1 MI_SMOOTHER_QUADRATURE_Q3=4 take effect on the shipped Q3 case: no "ignored" line, the oracle's
    interface displacements"""
    name = "fsi3_neo_3d_q3"
    stdout, rows = _run_case(name, "elasticity3d", tmp_path, env={"MI_FINE_LEVEL": "1", "MI_SMOOTHER_QUADRATURE_Q3": "4"})
    assert "ignored" not in stdout
    get = _prm(name)
    P = O.Problem(_scenario_desc(get, 3))
    ids = P.interface_nodes
    dt, exp = float(get("Time step size")), []
    for k in range(2):
        P.set_interface_traction((0.0, -40.0, 0.0))
        rc, _ = P.newmark_step(O.SOLVER_CG_SSOR, tol_lin=1e-12, max_it_mult=2.0)
        assert rc == 0
        exp.append(((k + 1) * dt, P.vec(O.V_U).reshape(-1, 3)[ids].copy()))
    _check_rows(rows, exp, 3)
