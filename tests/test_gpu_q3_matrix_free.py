"""The matrix-free fine level ("fine_level" 1) on 3D Q3 meshes, the reference's default element degree: point records at the
125 points of qf_cell(5) (mf_records_q3), every product of the level on the sum-factorised Q3 product (mf_spmv_q3), the
nodes' diagonal blocks from the records (mf_diag_q3), the residual from the generic element kernel's residual pass.
Against the CPU oracle's assembled system, against the assembled fine level on the same state, through Newmark steps, the
multigrid preconditioner and the executable; and what the level still refuses."""
import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg
from test_gpu_parity import _diag_blocks_of, _pair, _randomise_state, _relmax
from test_host_gpu import _check_rows, _prm, _run_case, _scenario_desc

M = load_pkg()
pytestmark = pytest.mark.gpu

TOL_ASM = 1e-12
TOL_SOL = 1e-8
ROLES = [O.FACE_CLAMPED, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_INTERFACE, O.FACE_ZCLAMP, O.FACE_INTERFACE]


@pytest.mark.parametrize("perturb_amp", [0.0, 0.05])
def test_q3_matrix_free_fine_level_against_the_oracle(perturb_amp):
    """residual, operator (constrained rows / columns and their diagonal rule included) and diagonal blocks of the Q3
    level against the oracle's assembled system [REF nonlinear_elasticity.cc:760-774, 1011-1023]; box and distorted
    cells; the converged update of a Jacobi-PCG on that operator; and back to the assembled level"""
    P, G = _pair(3, 3, (3, 2, 3), perturb_amp=perturb_amp, seed=41, roles=ROLES, body_force=(0.0, -9.81, 2.0))
    G.set_tuning("fine_level", 1)
    assert G.get_tuning("fine_level") == 1
    with pytest.raises(M.MiError):  # no tangent yet
        G.spmv(np.ones(G.n))
    rng = np.random.default_rng(43)
    for rnd in range(2):
        _randomise_state(P, G, seed=42 + rnd)
        P.update_acceleration()
        P.assemble()
        G.update_acceleration()
        rn = G.assemble()
        K = P.csr()
        assert abs(rn - P.residual_norm()) / P.residual_norm() < 1e-12
        assert _relmax(G.get(M.V_RHS), P.vec(O.V_RHS)) < TOL_ASM
        D_o, D_g = _diag_blocks_of(K, 3), G.diagonal_blocks()
        assert _relmax(D_g, D_o) < TOL_ASM
        cons = P.constrained.reshape(-1, 3)
        for c in range(3):  # constrained dofs: row / column dropped up to the kept diagonal, exactly
            assert np.all(D_g[cons[:, c], c, (c + 1) % 3] == 0) and np.all(D_g[cons[:, c], (c + 2) % 3, c] == 0)
            assert np.all(D_g[cons[:, c], (c + 1) % 3, c] == 0) and np.all(D_g[cons[:, c], c, (c + 2) % 3] == 0)
        x = rng.standard_normal(G.n)
        y = G.spmv(x)
        assert _relmax(y, K @ x) < 1e-12
        assert np.array_equal(G.spmv(x), y)  # fixed summation order
        assert G.assemble_residual() == rn and _relmax(G.get(M.V_RHS), P.vec(O.V_RHS)) < TOL_ASM
        assert np.array_equal(G.spmv(x), y)  # the residual-only pass left the tangent's records alone
    with pytest.raises(M.MiError):
        G.csr()
    G.set_tuning("precond", 0)
    rc, its, res = G.cg_solve(1e-12, 4 * G.n)
    rc_o, its_o, _ = P.solve_linear(O.SOLVER_CG_JACOBI, tol_lin=1e-12, max_it_mult=4.0)
    assert rc == 0 and rc_o == 0
    assert _relmax(G.get(M.V_NEWTON), P.vec(O.V_NEWTON)) < TOL_SOL
    # ... and back: the assembled level returns with the next assembly
    G.set_tuning("fine_level", 0)
    G.assemble()
    assert _relmax(G.csr().data, K.data) < TOL_ASM
    assert _relmax(G.spmv(x), K @ x) < 1e-13
    assert _relmax(G.diagonal_blocks(), D_o) < TOL_ASM
    G.close()


def test_q3_matrix_free_residual_is_bitwise_the_assembled_one():
    """the level's residual pass is the generic element kernel's residual-only pass: system_rhs and the residual norm
    are the assembled level's bits"""
    G = {}
    for fl in (0, 1):
        P, G[fl] = _pair(3, 3, (3, 3, 2), perturb_amp=0.05, seed=51, roles=ROLES, body_force=(1.0, -9.81, 0.0))
        G[fl].set_tuning("fine_level", fl)
        _randomise_state(P, G[fl], seed=52)
        G[fl].update_acceleration()
    rn0, rn1 = G[0].assemble(), G[1].assemble()
    assert rn0 == rn1
    assert np.array_equal(G[0].get(M.V_RHS), G[1].get(M.V_RHS))
    assert G[0].assemble_residual() == G[1].assemble_residual()
    for g in G.values():
        g.close()


def _steps(fine_level, lag):
    G = M.Context(dim=3, degree=3, reps=(24, 12, 5), hi=(2.4, 1.2, 0.5))
    assert G.n > 75000 and G.get_tuning("precond") == 1  # (multigrid: the default above 75 k dofs)
    G.set_tuning("cg_warm_start", 2)
    if fine_level:
        G.set_tuning("fine_level", 1)
        G.set_tuning("mf_diag_lag", lag)
    out = []
    for s in range(3):
        G.set_interface_traction((0.0, -1e3 * (s + 1), 0.0))
        rc, info = G.newmark_step(tol_lin=1e-10, max_it_mult=2.0)
        assert rc == 0 and info.converged == 1
        out.append((info.newton_iterations, list(info.lin_its)[:info.newton_iterations], G.get(M.V_U), G.get(M.V_V),
                    G.get(M.V_A)))
    G.close()
    return out


@pytest.fixture(scope="module")
def assembled_steps():
    return _steps(0, 0)


@pytest.mark.parametrize("lag", [0, 1])
def test_q3_newmark_steps_matrix_free_against_assembled(assembled_steps, lag):
    """three Newmark steps of a 24 x 12 x 5-cell Q3 block (multigrid, the executable's warm start) on both fine levels:
    the same Newton iterations, CG iterations per solve within one (lag 0), u, v and a to 1e-8"""
    mf = _steps(1, lag)
    for (n0, l0, u0, v0, a0), (n1, l1, u1, v1, a1) in zip(assembled_steps, mf):
        assert n0 == n1
        if lag == 0:
            assert all(abs(i - j) <= 1 for i, j in zip(l0, l1)), (l0, l1)
        assert _relmax(u1, u0) < TOL_SOL and _relmax(v1, v0) < TOL_SOL and _relmax(a1, a0) < TOL_SOL


def test_q3_matrix_free_multigrid_against_the_oracle():
    """a small Q3 block with the multigrid preconditioner forced: two Newmark steps against the oracle's CG + SSOR; the
    V-cycle on the matrix-free level is a symmetric positive definite operator"""
    P, G = _pair(3, 3, (4, 3, 3), roles=ROLES)
    G.set_tuning("precond", 1)
    G.set_tuning("fine_level", 1)
    for s in range(2):
        t = (0.0, -2e3 * (s + 1), 500.0)
        P.set_interface_traction(t)
        G.set_interface_traction(t)
        rc, info = G.newmark_step(tol_lin=1e-12, max_it_mult=2.0)
        rc_o, info_o = P.newmark_step(O.SOLVER_CG_SSOR, tol_lin=1e-12, max_it_mult=2.0)
        assert rc == 0 and rc_o == 0 and info.converged == 1
        assert _relmax(G.get(M.V_U), P.vec(O.V_U)) < TOL_SOL
    free = ~G.constrained

    def minv(r):
        G.set_tuning("spmv_as_smoother", 2)
        z = G.spmv(r)
        G.set_tuning("spmv_as_smoother", 0)
        return z

    rng = np.random.default_rng(5)
    r1, r2 = rng.standard_normal(G.n) * free, rng.standard_normal(G.n) * free
    z1, z2 = minv(r1), minv(r2)
    assert abs(r2 @ z1 - r1 @ z2) <= 1e-10 * abs(r2 @ z1) and r1 @ z1 > 0 and r2 @ z2 > 0
    G.close()


def test_q3_executable_matrix_free_fine_level(tmp_path):
    """MI_FINE_LEVEL=1 takes effect on the shipped Q3 case: no "ignored" line, the oracle's interface displacements"""
    name = "fsi3_neo_3d_q3"
    stdout, rows = _run_case(name, "elasticity3d", tmp_path, env={"MI_FINE_LEVEL": "1"})
    assert "MI_FINE_LEVEL ignored" not in stdout
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


def _still_assembled(G, dim):
    assert G.get_tuning("fine_level") == 0
    G.set_interface_traction((0.0, -1e3, 0.0)[:dim])
    G.update_acceleration()
    G.assemble()
    x = np.random.default_rng(9).standard_normal(G.n)
    assert np.all(np.isfinite(G.spmv(x)))


@pytest.mark.parametrize("case", ["q3_slabs", "q3_fp32_storage", "q4", "q2_2d"])
def test_q3_matrix_free_refusals(case):
    """Q3 on a decomposed mesh, Q3 with "precond_storage" 32, Q4 and 2D stay refused; the refused team keeps its
    assembled level"""
    kw = dict(q3_slabs=dict(dim=3, degree=3, reps=(2, 2, 4), slabs=2), q3_fp32_storage=dict(dim=3, degree=3, reps=(2, 2, 2)),
              q4=dict(dim=3, degree=4, reps=(1, 1, 2)), q2_2d=dict(dim=2, degree=2, reps=(4, 3), hi=(1, 1)))[case]
    G = M.Context(**kw)
    if case == "q3_fp32_storage":
        G.set_tuning("precond_storage", 32)
    with pytest.raises(M.MiError):
        G.set_tuning("fine_level", 1)
    _still_assembled(G, kw["dim"])
    if case != "q3_slabs":
        assert G.csr().nnz > 0
    G.close()
