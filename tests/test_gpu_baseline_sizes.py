"""The HIP path with DEFAULT tuning against oracle results at the BASELINE sizes (tests/golden/baseline_sizes.npz, written
by tests/golden/make_golden_big.py from the CPU restatement of the reference algorithm).

These are the sizes at which the product's default solver path is multigrid-PCG with the matrix-free smoother and the
sum-factorised element kernel (above 100 k nodes); everything the oracle is compared with elsewhere runs on <= ~10 k DoFs,
where the preconditioner is Jacobi and the smoother the assembled matrix.

  blk24  24^3 Q2 cells (352,947 DoFs), two Newmark steps, linear tolerance 1e-12   [REF nonlinear_elasticity.cc:410-499]
  blk24d the same block with distorted cells (general-geometry kernels)
  cfg3   BASELINE configuration 3, 34^3 Q2 cells (985,527 DoFs), the first three steps of the ramp, "Residual" 1e-10
  cfg4   BASELINE configuration 4, 59^3 Q2 cells (5,055,477 DoFs), one Newton iteration (residual, operator, update)
  cfg4s  the same configuration, the first three Newmark steps of the ramp
  cfg2   BASELINE configuration 2, 40^3 Q1 cells of the linear model (206,763 DoFs), three theta-steps
                                                                                    [REF linear_elasticity.cc:378-586]
Compared: values at a lattice subsample of the nodes (same lexicographic node ids on both sides), the Euclidean norm of
each whole vector and its inner product with w_i = cos(0.37 i + 0.11), the Newton table."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg

M = load_pkg()
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_sizes.npz")


def _g():
    return np.load(GOLD)


def _w(n):
    return np.cos(0.37 * np.arange(n, dtype=np.float64) + 0.11)


def _fun(v):
    return np.array([np.linalg.norm(v), float(v @ _w(v.size))])


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _relfun(v, ref):
    """functionals of a whole vector against the stored pair: both relative to the vector's norm"""
    f = _fun(v)
    return max(abs(f[0] / ref[0] - 1.0), abs(f[1] - ref[1]) / ref[0] / np.sqrt(v.size / 2.0))


def test_fixture_layout():
    g = _g()
    assert int(g["q1_48_cells"]) == 48 and int(g["q2_2d_cells"]) == 300 and g["q2_2d_u"].shape[-1] == 2
    for name, cells, p in (("blk24", 24, 2), ("blk24d", 24, 2), ("cfg3", 34, 2), ("cfg4", 59, 2), ("cfg4s", 59, 2), ("cfg2", 40, 1)):
        assert int(g[name + "_cells"]) == cells
        ids = g[name + "_nodes"]
        assert np.all(np.diff(ids) > 0) and ids[0] == 0 and ids[-1] == (p * cells + 1) ** 3 - 1
    assert os.path.getsize(GOLD) < 1_000_000


def test_oracle_reproduces_config2_fixture():
    """seconds on CPU: the one case of the file the CPU suite can afford to regenerate"""
    g = _g()
    L = O.LinearProblem(O.make_desc(dim=3, degree=1, reps=(40,) * 3, hi=(10.0, 1.0, 1.0), theta=0.5))
    inodes, ids = L.interface_nodes, g["cfg2_nodes"]
    for s in range(2):
        L.vec(O.L_STRESS)[:] = 0
        for c in range(3):
            L.vec(O.L_STRESS)[inodes * 3 + c] = g["cfg2_traction"][c]
        rc, _, _ = L.step(O.SOLVER_CG_JACOBI, True, abs_tol=float(g["cfg2_abs_tol"]))
        assert rc == 0
        assert _rel(L.vec(O.L_D).reshape(-1, 3)[ids], g["cfg2_d"][s]) < 1e-11
        assert _rel(L.vec(O.L_V).reshape(-1, 3)[ids], g["cfg2_v"][s]) < 1e-11


def _nonlinear(name, tol_u, tol_va, start=0, distorted=False, dim=3, degree=2, slabs=1, cut_axis=0, dist_nodes=None,
               smoother_precision=64, fine_level=0, quadrature=None):
    g = _g()
    n = int(g[name + "_cells"])
    # (make_golden_big.distortion: vertices moved by 8 % of the cell size, seeded)
    perturb = 0.08 / n * np.random.default_rng(77).standard_normal(((n + 1) ** 3, 3)) if distorted else None
    G = M.Context(dim=dim, degree=degree, reps=(n,) * dim, perturb=perturb, slabs=slabs, cut_axis=cut_axis)
    if dist_nodes is not None:  # (the hierarchy exists since the context's creation above 75 k dofs: the key rebuilds it)
        G.set_tuning("mg_dist_nodes", dist_nodes)
    assert G.get_tuning("precond") == 1  # multigrid: the default above 75 k dofs
    if slabs > 1:  # levels cut into slabs: fine + Q1 on the same cells (+ the first coarsened level when forced / big enough)
        assert G.get_tuning("mg_distributed_levels") == (2 if degree > 1 else 1) + (1 if dist_nodes == 0 else 0)
    G.set_tuning("cg_warm_start", start)  # 0: the library's default; 2: what the executable and bench.py set
    if quadrature is not None:  # (default 3 since round 6: the smoother's fine-level operator with 27 Gauss points)
        G.set_tuning("smoother_quadrature", quadrature)
    if smoother_precision != 64:
        G.set_tuning("smoother_precision", smoother_precision)
    if fine_level:  # round 6: no assembled fine tangent -- records + residual + diagonal blocks, every product on mf_spmv
        G.set_tuning("fine_level", 1)
        assert G.get_tuning("fine_level") == 1
        G.set_tuning("mf_diag_lag", 1 if fine_level == 2 else 0)  # 2: the policy bench.py and the executable run with
    ids = g[name + "_nodes"]
    for s, trac in enumerate(g[name + "_traction"]):
        G.set_interface_traction(trac)
        rc, info = G.newmark_step(tol_lin=float(g[name + "_tol_lin"]), max_it_mult=2.0)
        row = g[name + "_log"][s]
        assert rc == 0 and info.converged == 1
        assert [info.newton_iterations, info.assemblies] == [int(row[0]), int(row[1])]  # nonlinear_elasticity.cc:446-469
        u = G.get(M.V_U)
        assert _rel(u.reshape(-1, dim)[ids], g[name + "_u"][s]) < tol_u
        assert _relfun(u, g[name + "_fun"][s][0]) < tol_u
        for k, which in ((1, M.V_V), (2, M.V_A)):
            assert _relfun(G.get(which), g[name + "_fun"][s][k]) < tol_va
    # 3D Q2: the matrix-free smoother was what ran; the other elements smooth with the assembled matrix
    if slabs == 1 or fine_level:  # (a slab of a quarter of this block is below the size at which the matrix-free form is chosen)
        assert G.get_tuning("smoother_operator_active") == (2 if (dim, degree) == (3, 2) else 0)
        if (dim, degree) == (3, 2):  # ... from the 27-point records unless asked otherwise; the fp32 products keep 64 points
            assert G.get_tuning("smoother_quadrature_active") == (4 if smoother_precision == 32 else (quadrature or 3))
    if fine_level:  # nothing was assembled: no matrix to export
        with pytest.raises(M.MiError):
            G.csr()
    assert _rel(G.get(M.V_V).reshape(-1, dim)[ids], g[name + "_v"]) < tol_va
    assert _rel(G.get(M.V_A).reshape(-1, dim)[ids], g[name + "_a"]) < tol_va  # amplified by 1/dt^2
    G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("start", [0, 2])
def test_gpu_24cube_block_two_steps_default_path(start):
    """(the second step runs on the coarse operators of the first and, with start = 2, from the first step's solutions)"""
    _nonlinear("blk24", 1e-8, 1e-6, start)


@pytest.mark.gpu
@pytest.mark.parametrize("slabs,cut_axis", [(2, 0), (4, 2), (3, 1)])
def test_gpu_24cube_block_decomposed_against_the_oracle(slabs, cut_axis):
    """the same fixture on 2 / 4 / 3 slabs cut along the default (last), the y and the x direction: the distributed
    multigrid levels, halo exchanges and the matrix-free smoother on slabs against the oracle, not against the
    undecomposed run"""
    _nonlinear("blk24", 1e-8, 1e-6, 2, slabs=slabs, cut_axis=cut_axis)


@pytest.mark.gpu
@pytest.mark.parametrize("slabs,cut_axis", [(3, 0), (4, 2), (2, 1)])
def test_gpu_24cube_block_with_a_distributed_first_coarsened_level(slabs, cut_axis):
    """round 5: past a size threshold the first COARSENED multigrid level (12^3 cells here, forced by tuning "mg_dist_nodes" 0) is
    cut into slabs of its own instead of being replicated on every slab: cuts induced by the finer level's, restriction and
    coarse state through partial results on ghost planes (team_halo_accumulate), prolongation of the owned planes from
    the slab's own box.  Same fixture, same tolerances as the replicated hierarchy: against the oracle."""
    _nonlinear("blk24", 1e-8, 1e-6, 2, slabs=slabs, cut_axis=cut_axis, dist_nodes=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,slabs", [("blk24", 1), ("cfg3", 1), ("cfg3", 4)])
def test_gpu_fp32_smoother_products_against_the_oracle(name, slabs):
    """opt-in "smoother_precision" 32 (round 5): the multigrid smoother's matrix-free fine-level products in fp32 arithmetic on
    fp32 point records -- a preconditioner-only change: the CG, its product, the residuals, the assembly and the stopping rule
    [REF nonlinear_elasticity.cc:1171-1174] stay fp64, so the converged steps are the oracle's to the same tolerances as with
    the fp64 smoother (Newton tables equal, displacement 1e-8, velocity / acceleration 1e-6).  Not the headline setting."""
    _nonlinear(name, 1e-8, 1e-6, 2, slabs=slabs, smoother_precision=32)


@pytest.mark.gpu
@pytest.mark.parametrize("name,slabs,cut_axis,start,distorted,mode",
                         [("blk24", 1, 0, 0, False, 1), ("blk24", 1, 0, 2, False, 2), ("blk24d", 1, 0, 2, True, 2), ("blk24", 3, 1, 2, False, 1),
                          ("cfg3", 1, 0, 2, False, 1), ("cfg3", 1, 0, 2, False, 2), ("cfg3", 4, 0, 2, False, 2),
                          ("cfg4s", 1, 0, 2, False, 1), ("cfg4s", 1, 0, 2, False, 2), ("cfg4s", 8, 0, 2, False, 2)])
def test_gpu_matrix_free_fine_level_against_the_oracle(name, slabs, cut_axis, start, distorted, mode):
    """round 6, tuning "fine_level" 1: the fine level keeps NO assembled tangent -- a tangent assembly is the residual pass
    that writes the point records plus the nodes' diagonal blocks formed from them (mf_diag), and the CG's product, the
    residual / start-vector products and the smoother all run on mf_spmv.  Same fixtures, same tolerances, same Newton
    tables as the assembled path (the oracle's steps [REF nonlinear_elasticity.cc:410-499, 1044-1087, 1153-1191]): boxes and
    distorted cells, one slab and decomposed (the CG's matrix-free product around the halo exchange), BASELINE
    configurations 3 and 4 on 1 and 4 / 8 slabs.  mode 2: with "mf_diag_lag" 1 -- the diagonal blocks (smoother side only)
    formed at the first tangent of a time step and kept over its Newton iterations: the policy bench.py's
    with_matrix_free_fine_level and the executable (MI_FINE_LEVEL=1) run with."""
    _nonlinear(name, 1e-8, 1e-6, start, distorted=distorted, slabs=slabs, cut_axis=cut_axis, fine_level=mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name,slabs,fine_level,distorted", [("blk24", 1, 0, False), ("blk24d", 1, 0, True), ("cfg3", 1, 0, False),
                                                             ("cfg3", 4, 2, False), ("cfg4s", 1, 2, False)])
def test_gpu_smoother_with_the_assembly_quadrature_against_the_oracle(name, slabs, fine_level, distorted):
    """the multigrid smoother's fine-level operator with the assembly's 4 x 4 x 4 Gauss points (tuning "smoother_quadrature" 4: the
    smoother of rounds 3-5, mf_spmv) -- the library's default since round 6 is the 27-point rule (mf_spmv27), which every
    other test of this file runs under; both against the same oracle steps at the same tolerances"""
    _nonlinear(name, 1e-8, 1e-6, 2, distorted=distorted, slabs=slabs, fine_level=fine_level, quadrature=4)


@pytest.mark.gpu
def test_gpu_24cube_distorted_block_two_steps_default_path():
    """no cell is a box: the general-geometry branches of the element kernel and of the matrix-free product, at the
    size where the multigrid + matrix-free path is the default"""
    _nonlinear("blk24d", 1e-8, 1e-6, 2, distorted=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dim,degree", [("q1_48", 3, 1), ("q2_2d", 2, 2)])
def test_gpu_other_element_families_on_the_multigrid_path(name, dim, degree):
    """48^3 Q1 cells in 3D, 300^2 Q2 cells in 2D: the node-pair element kernel and the multigrid with the assembled
    smoother, two steps against the oracle"""
    _nonlinear(name, 1e-8, 1e-6, 2, dim=dim, degree=degree)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [0, 2])
def test_gpu_config3_three_steps_default_path(start):
    """(steps 2 and 3 run on the coarse operators of step 1 and, with start = 2, from the previous step's solutions)"""
    _nonlinear("cfg3", 1e-8, 1e-6, start)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [0, 2])
def test_gpu_config4_three_steps_default_path(start):
    """the headline size through the first three Newmark steps of the bench's ramp against the oracle; start = 2: under
    the policies bench.py runs with (start vectors from the previous step; the coarse operators are those of step 1
    in both parametrisations)"""
    _nonlinear("cfg4s", 1e-8, 1e-6, start)


@pytest.mark.gpu
@pytest.mark.parametrize("name,slabs,cut_axis", [("cfg4s", 8, 0), ("cfg4s", 4, 1), ("cfg3", 8, 0)])
def test_gpu_baseline_configurations_decomposed_against_the_oracle(name, slabs, cut_axis):
    """BASELINE configuration 4 IS a decomposed run ("domain-decomposed 8 x MI355X"): the headline block on 8 slabs
    (automatic cut direction) and on 4 slabs cut along x (the lattice lies rotated over the box), configuration 3 on 8
    slabs -- three ramp steps each with the executable's start vectors, against the oracle's steps, not against the
    undecomposed run (emulated slabs: the same halo / all-reduce choreography on one GPU)
    [REF nonlinear_elasticity.cc:410-499; adapter.h:152-154: the reference itself is single rank]"""
    _nonlinear(name, 1e-8, 1e-6, 2, slabs=slabs, cut_axis=cut_axis)


@pytest.mark.gpu
def test_gpu_config4_at_the_shipped_linear_tolerance():
    """what bench.py times -- configuration 4, "Residual" = 1e-6 as shipped (parameters.prm:51), the executable's solver
    policies -- against the oracle's steps at 1e-10: the same Newton tables, displacements to 1e-5 (with the
    shipped tolerance only ~1e-5 can be claimed; the iterates of different preconditioners differ that much)"""
    g = _g()
    n = int(g["cfg4s_cells"])
    G = M.Context(dim=3, degree=2, reps=(n, n, n))
    G.set_tuning("cg_warm_start", 2)
    ids = g["cfg4s_nodes"]
    for s, trac in enumerate(g["cfg4s_traction"]):
        G.set_interface_traction(trac)
        rc, info = G.newmark_step(tol_lin=1e-6, max_it_mult=1.0)
        row = g["cfg4s_log"][s]
        assert rc == 0 and info.converged == 1
        assert [info.newton_iterations, info.assemblies] == [int(row[0]), int(row[1])]
        u = G.get(M.V_U)
        assert _rel(u.reshape(-1, 3)[ids], g["cfg4s_u"][s]) < 1e-5 and _relfun(u, g["cfg4s_fun"][s][0]) < 1e-5
    G.close()


@pytest.mark.gpu
def test_gpu_config4_one_newton_iteration_default_path():
    g = _g()
    n = int(g["cfg4_cells"])
    G = M.Context(dim=3, degree=2, reps=(n, n, n))
    assert G.n == 5055477 and G.nnz == 952414353  # SURVEY.md section 8 size table
    ids = g["cfg4_nodes"]
    G.set_interface_traction(g["cfg4_traction"])
    G.newton_begin_step()
    G.update_acceleration()
    rn = G.assemble()
    assert abs(rn / float(g["cfg4_res_norm"]) - 1) < 1e-12                       # get_error_residual :549-560
    rhs = G.get(M.V_RHS)
    assert _rel(rhs.reshape(-1, 3)[ids], g["cfg4_rhs"]) < 1e-12 and _relfun(rhs, g["cfg4_rhs_fun"]) < 1e-12
    Kw = G.spmv(_w(G.n))                                                         # the assembled tangent, 952 M non-zeros
    assert _rel(Kw.reshape(-1, 3)[ids], g["cfg4_Kw"]) < 1e-12 and _relfun(Kw, g["cfg4_Kw_fun"]) < 1e-12
    rc, its, res = G.cg_solve(float(g["cfg4_tol_lin"]), 2 * G.n)                 # :1153-1211, multigrid-PCG
    assert rc == 0 and 0 < its < 40
    assert G.get_tuning("smoother_operator_active") == 2
    du = G.get(M.V_NEWTON)
    assert _rel(du.reshape(-1, 3)[ids], g["cfg4_upd"]) < 1e-7 and _relfun(du, g["cfg4_upd_fun"]) < 1e-7
    upd = G.apply_newton_update()
    assert abs(upd / float(g["cfg4_upd_norm_unconstrained"]) - 1) < 1e-7         # get_error_update :564-576
    G.close()


@pytest.mark.gpu
def test_gpu_config2_linear_model_three_steps():
    g = _g()
    n = int(g["cfg2_cells"])
    G = M.Context(dim=3, degree=1, reps=(n, n, n), hi=(10.0, 1.0, 1.0))
    assert G.n == 206763 and G.nnz == 15944049
    L = M.lib()
    L.mi_linear_setup.argtypes = [C.c_void_p, C.c_double]
    L.mi_linear_step.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert L.mi_linear_setup(G.h, 0.5) == 0, L.mi_last_error(G.h)
    ids = g["cfg2_nodes"]
    for s in range(3):
        G.set_interface_traction(g["cfg2_traction"])
        its, res = C.c_int(0), C.c_double(0)
        assert L.mi_linear_step(G.h, 1, float(g["cfg2_abs_tol"]), 4 * G.n, C.byref(its), C.byref(res)) == 0, \
            L.mi_last_error(G.h)
        d, v = G.get(0), G.get(2)
        assert _rel(d.reshape(-1, 3)[ids], g["cfg2_d"][s]) < 1e-8 and _rel(v.reshape(-1, 3)[ids], g["cfg2_v"][s]) < 1e-8
        assert _relfun(d, g["cfg2_fun"][s][0]) < 1e-8 and _relfun(v, g["cfg2_fun"][s][1]) < 1e-8
    G.close()
