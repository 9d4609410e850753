"""The Q3 matrix-free level's assembly in one sum-factorised launch (tuning "point_pass_q3" 1): mf_point_pass_q3 forms the
residual of every cell -- and, in a tangent pass, the point records -- in the shape of mf_spmv_q3, residual_gather sums the
cells' slots into system_rhs.  Against the CPU oracle, against the default form (the generic element kernel's residual pass
+ mf_records_q3) on the same state, at the stress-free state, through mi_assemble_residual, on a folded mesh, through the
key's semantics, Newmark steps and the executable.  The meshes are the smallest at which the kernel can go wrong: one cell,
2 x 2 x 2 (a node shared by eight cells), 3 x 2 x 3 (anisotropic: an axis mix-up shows), each of boxes and of distorted cells."""
import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg
from test_gpu_parity import _diag_blocks_of
from test_gpu_q3_matrix_free import ROLES, TOL_ASM, TOL_SOL, _pair, _randomise_state, _relmax
from test_host_gpu import _check_rows, _prm, _run_case, _scenario_desc

M = load_pkg()
pytestmark = pytest.mark.gpu

MESHES = [(1, 1, 1), (2, 2, 2), (3, 2, 3)]
BODY = (1.5, -9.81, 2.0)


def _level(reps, perturb_amp, key=1, seed=61, body_force=BODY):
    """oracle problem + a Q3 matrix-free context with "point_pass_q3" = key (None: the key is never set)"""
    P, G = _pair(3, 3, reps, perturb_amp=perturb_amp, seed=seed, roles=ROLES, body_force=body_force)
    G.set_tuning("fine_level", 1)
    if key is not None:
        G.set_tuning("point_pass_q3", key)
        assert G.get_tuning("point_pass_q3_active") == key
    return P, G


def _state(P, G, seed):
    """a random state with a non-zero interface traction, the acceleration updated on both sides"""
    _randomise_state(P, G, seed=seed)
    P.update_acceleration()
    G.update_acceleration()


@pytest.mark.parametrize("perturb_amp", [0.0, 0.05])
@pytest.mark.parametrize("reps", MESHES)
def test_point_pass_residual_against_the_oracle(reps, perturb_amp):
    """system_rhs and the residual norm of the one-launch pass against the oracle's assembly, two random states per mesh;
    constrained dofs get no residual at all [REF nonlinear_elasticity.cc:769-773, 984-995]"""
    P, G = _level(reps, perturb_amp)
    for rnd in range(2):
        _state(P, G, seed=62 + rnd)
        P.assemble()
        rn = G.assemble()
        rhs = G.get(M.V_RHS)
        print("reps", reps, "perturb", perturb_amp, "rhs", _relmax(rhs, P.vec(O.V_RHS)), "norm",
              abs(rn - P.residual_norm()) / P.residual_norm())
        assert _relmax(rhs, P.vec(O.V_RHS)) < TOL_ASM
        assert abs(rn - P.residual_norm()) / P.residual_norm() < 1e-12
        assert np.all(rhs[P.constrained] == 0.0)
    G.close()


@pytest.mark.parametrize("perturb_amp", [0.0, 0.05])
@pytest.mark.parametrize("reps", MESHES)
def test_point_pass_against_the_default_form_on_the_same_state(reps, perturb_amp):
    """the residual, the operator and the diagonal blocks of a tangent pass against the context that runs the generic
    residual pass and mf_records_q3: the records come from the same stages"""
    P0, G0 = _level(reps, perturb_amp, key=0)
    P1, G1 = _level(reps, perturb_amp, key=1)
    _state(P0, G0, seed=64)
    _state(P1, G1, seed=64)
    rn0, rn1 = G0.assemble(), G1.assemble()
    assert abs(rn1 - rn0) / rn0 < 1e-12
    assert _relmax(G1.get(M.V_RHS), G0.get(M.V_RHS)) < TOL_ASM
    x = np.random.default_rng(65).standard_normal(G0.n)
    y0, y1 = G0.spmv(x), G1.spmv(x)
    D0, D1 = G0.diagonal_blocks(), G1.diagonal_blocks()
    print("reps", reps, "perturb", perturb_amp, "rhs", _relmax(G1.get(M.V_RHS), G0.get(M.V_RHS)), "spmv", _relmax(y1, y0),
          "bitwise", np.array_equal(y1, y0), "blocks", _relmax(D1, D0), "bitwise", np.array_equal(D1, D0))
    assert _relmax(y1, y0) < 1e-13
    assert _relmax(D1, D0) < TOL_ASM
    G0.close()
    G1.close()


@pytest.mark.parametrize("perturb_amp", [0.0, 0.05])
@pytest.mark.parametrize("reps", MESHES)
def test_point_pass_stress_free_state_is_exactly_zero(reps, perturb_amp):
    """u = du = 0, no acceleration, no body force, no traction: tau itself goes into the gradient rows (not the tangent's
    split of it), so every entry of system_rhs is an exact zero"""
    P, G = _level(reps, perturb_amp, body_force=(0.0, 0.0, 0.0))
    G.set_interface_traction((0.0, 0.0, 0.0))
    G.update_acceleration()
    assert np.all(G.get(M.V_A) == 0.0)
    assert G.assemble() == 0.0
    assert np.all(G.get(M.V_RHS) == 0.0)
    assert G.assemble_residual() == 0.0 and np.all(G.get(M.V_RHS) == 0.0)
    G.close()


@pytest.mark.parametrize("perturb_amp", [0.0, 0.05])
@pytest.mark.parametrize("reps", MESHES)
def test_point_pass_assemble_residual(reps, perturb_amp):
    """mi_assemble_residual runs the kernel without its record stores: the bits of mi_assemble's residual on the same state,
    the tangent's products unchanged after a residual at another state, and a fixed summation order"""
    P, G = _level(reps, perturb_amp)
    _state(P, G, seed=66)
    rn = G.assemble()
    rhs = G.get(M.V_RHS)
    x = np.random.default_rng(67).standard_normal(G.n)
    y = G.spmv(x)
    assert G.assemble_residual() == rn and np.array_equal(G.get(M.V_RHS), rhs)
    _state(P, G, seed=68)  # another state: the residual moves, the records stay
    rn2 = G.assemble_residual()
    assert rn2 != rn and not np.array_equal(G.get(M.V_RHS), rhs)
    assert np.array_equal(G.spmv(x), y)
    assert G.assemble() == rn2  # ... and two assemblies of one state give identical bits
    rhs2, y2 = G.get(M.V_RHS), G.spmv(x)
    assert not np.array_equal(y2, y)
    assert G.assemble() == rn2 and np.array_equal(G.get(M.V_RHS), rhs2) and np.array_equal(G.spmv(x), y2)
    G.close()


def test_point_pass_reports_an_inverted_element():
    """the state of test_inverted_element_is_reported: det F <= 0 at the points of the rule is a status code of both
    passes, and the context assembles again afterwards [REF nonlinear_elasticity.cc:935]"""
    G = M.Context(dim=3, degree=3, reps=(3, 3, 2))
    G.set_tuning("fine_level", 1)
    G.set_tuning("point_pass_q3", 1)
    G.set_interface_traction((0.0, 0.0, 0.0))
    G.update_acceleration()
    assert np.isfinite(G.assemble())  # a regular state assembles
    u = np.zeros((G.nnodes, 3))
    u[:, 0] = -2.5 * G.coords[:, 0]  # F_xx = 1 - 2.5 < 0 everywhere
    G.set(M.V_U, (u * (~G.constrained.reshape(-1, 3))).ravel())
    with pytest.raises(M.MiError, match="inverted element"):
        G.assemble()
    with pytest.raises(M.MiError, match="inverted element"):
        G.assemble_residual()
    G.set(M.V_U, np.zeros(G.n))  # the context survives
    assert np.isfinite(G.assemble()) and np.isfinite(G.assemble_residual())
    assert G.get_tuning("point_pass_q3_active") == 1
    G.close()


def test_point_pass_key_default_values_and_both_orders():
    """default 0; active only while the Q3 level exists, whichever of the two keys was set first; 2 and -1 refused; "fine_level"
    0 brings the assembled level back"""
    P, G = _pair(3, 3, (2, 2, 2), perturb_amp=0.05, seed=71, roles=ROLES, body_force=BODY)
    assert G.get_tuning("point_pass_q3") == 0 and G.get_tuning("point_pass_q3_active") == 0
    for bad in (2, -1):
        with pytest.raises(M.MiError):
            G.set_tuning("point_pass_q3", bad)
        assert G.get_tuning("point_pass_q3") == 0
    G.set_tuning("point_pass_q3", 1)  # the key first, the level second
    assert G.get_tuning("point_pass_q3") == 1 and G.get_tuning("point_pass_q3_active") == 0
    G.set_tuning("fine_level", 1)
    assert G.get_tuning("point_pass_q3_active") == 1
    _state(P, G, seed=72)
    P.assemble()
    G.assemble()
    assert _relmax(G.get(M.V_RHS), P.vec(O.V_RHS)) < TOL_ASM
    P2, G2 = _pair(3, 3, (2, 2, 2), perturb_amp=0.05, seed=71, roles=ROLES, body_force=BODY)
    G2.set_tuning("fine_level", 1)  # the level first, the key second
    assert G2.get_tuning("point_pass_q3_active") == 0
    G2.set_tuning("point_pass_q3", 1)
    assert G2.get_tuning("point_pass_q3_active") == 1
    _state(P2, G2, seed=72)
    G2.assemble()
    assert np.array_equal(G2.get(M.V_RHS), G.get(M.V_RHS))
    for bad in (2, -1):
        with pytest.raises(M.MiError):
            G2.set_tuning("point_pass_q3", bad)
        assert G2.get_tuning("point_pass_q3") == 1 and G2.get_tuning("point_pass_q3_active") == 1
    G2.close()
    # ... and back to the assembled level: the key stays, nothing runs it
    G.set_tuning("fine_level", 0)
    assert G.get_tuning("point_pass_q3") == 1 and G.get_tuning("point_pass_q3_active") == 0
    G.assemble()
    assert _relmax(G.csr().data, P.csr().data) < TOL_ASM
    assert _relmax(G.get(M.V_RHS), P.vec(O.V_RHS)) < TOL_ASM
    G.close()


@pytest.mark.parametrize("case", ["q2_3d_matrix_free", "q2_2d", "q3_key_1_then_0"])
def test_point_pass_key_without_effect_gives_the_default_bits(case):
    """on a 3D Q2 matrix-free level and on a 2D context the key is accepted and nothing runs it; on a Q3 level 1 then 0 is the
    default again: residual and norm are the bits of a context that never saw the key"""
    kw = dict(q2_3d_matrix_free=dict(dim=3, degree=2, reps=(3, 2, 2)), q2_2d=dict(dim=2, degree=2, reps=(4, 3)),
              q3_key_1_then_0=dict(dim=3, degree=3, reps=(2, 2, 2)))[case]
    dim = kw["dim"]
    roles = ROLES if dim == 3 else None
    out = []
    for touched in (False, True):
        P, G = _pair(kw["dim"], kw["degree"], kw["reps"], perturb_amp=0.05, seed=73, roles=roles, body_force=BODY[:dim] + (0.0,) * (3 - dim))
        if dim == 3:
            G.set_tuning("fine_level", 1)
        if touched:
            G.set_tuning("point_pass_q3", 1)
            assert G.get_tuning("point_pass_q3") == 1
            assert G.get_tuning("point_pass_q3_active") == (1 if case == "q3_key_1_then_0" else 0)
            if case == "q3_key_1_then_0":
                G.set_tuning("point_pass_q3", 0)
                assert G.get_tuning("point_pass_q3_active") == 0
        _state(P, G, seed=74)
        rn = G.assemble()
        x = np.random.default_rng(75).standard_normal(G.n)
        out.append((rn, G.get(M.V_RHS), G.spmv(x), G.assemble_residual()))
        G.close()
    assert out[0][0] == out[1][0] and out[0][3] == out[1][3]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def _steps(key, lag, points):
    """three Newmark steps of the 24 x 12 x 5 block of test_gpu_q3_matrix_free._steps on the matrix-free level"""
    G = M.Context(dim=3, degree=3, reps=(24, 12, 5), hi=(2.4, 1.2, 0.5))
    assert G.n > 75000 and G.get_tuning("precond") == 1  # (multigrid: the default above 75 k dofs)
    G.set_tuning("cg_warm_start", 2)
    G.set_tuning("fine_level", 1)
    G.set_tuning("mf_diag_lag", lag)
    G.set_tuning("smoother_quadrature_q3", points)
    G.set_tuning("point_pass_q3", key)
    out = []
    for s in range(3):
        G.set_interface_traction((0.0, -1e3 * (s + 1), 0.0))
        rc, info = G.newmark_step(tol_lin=1e-10, max_it_mult=2.0)
        assert rc == 0 and info.converged == 1
        assert G.get_tuning("point_pass_q3_active") == key
        out.append((info.newton_iterations, list(info.lin_its)[:info.newton_iterations], G.get(M.V_U), G.get(M.V_V),
                    G.get(M.V_A)))
    G.close()
    return out


@pytest.mark.parametrize("lag,points", [(0, 5), (1, 5), (1, 4)])
def test_point_pass_newmark_steps_against_the_default_form(lag, points):
    """three Newmark steps (multigrid, the executable's warm start) with both forms of the assembly: the same Newton
    iterations, CG iterations per solve within one, u, v and a to 1e-8"""
    ref, new = _steps(0, lag, points), _steps(1, lag, points)
    for (n0, l0, u0, v0, a0), (n1, l1, u1, v1, a1) in zip(ref, new):
        assert n0 == n1
        assert all(abs(i - j) <= 1 for i, j in zip(l0, l1)), (l0, l1)
        assert _relmax(u1, u0) < TOL_SOL and _relmax(v1, v0) < TOL_SOL and _relmax(a1, a0) < TOL_SOL


def test_point_pass_executable(tmp_path):
    """MI_POINT_PASS_Q3=1 beside MI_FINE_LEVEL=1 takes effect on the shipped Q3 case: no "ignored" line, the oracle's interface
    displacements"""
    name = "fsi3_neo_3d_q3"
    stdout, rows = _run_case(name, "elasticity3d", tmp_path, env={"MI_FINE_LEVEL": "1", "MI_POINT_PASS_Q3": "1"})
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
