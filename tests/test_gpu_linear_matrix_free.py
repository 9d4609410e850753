"""The linear model without matrices (tuning "linear_operator" 1, 3D Q3 on one slab): K, M and the stepping matrix
A = M + theta^2 dt^2 K as one kernel on the model's own 4 x 4 x 4 rule (mf_linear_q3) + the slot gathers, the diagonal of A
from mf_linear_diag_q3, the body force as M (b, b, ...).  Against the CPU oracle's assembled matrices and direct solve, against
the assembled operators of a second context on distorted cells, through mi_linear_step and the executable; what the key
refuses and what a matrix-free context refuses; and the inspection hooks on the default (assembled) path."""
import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg
from test_host_gpu import _check_rows, _run_case

M = load_pkg()
pytestmark = pytest.mark.gpu

ROLES = [O.FACE_CLAMPED] + [O.FACE_INTERFACE] * 5  # one clamped face, the others interface
THETA = 0.6
MAT = dict(mu=0.5e6, nu=0.4, rho=1000.0, delta_t=0.005)
BODY = (0.0, -9.81, 2.0)
# 18 cells, 7 x 10 x 10 nodes: the last workgroup has two idle waves, nodes shared across faces, edges and corners in every
# direction | one cell: three idle waves, every node on the boundary.  Anisotropic boxes
SHAPES = {"3x2x3": ((3, 2, 3), (1.5, 0.7, 1.1)), "1x1x1": ((1, 1, 1), (0.5, 0.35, 0.55))}


def _relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _oracle(shape, body=BODY):
    reps, hi = SHAPES[shape]
    return O.LinearProblem(O.make_desc(dim=3, degree=3, reps=reps, hi=hi, face_role=ROLES, theta=THETA, body_force=body, **MAT))


def _context(shape, operator, body=BODY, perturb=None, setup=True):
    reps, hi = SHAPES[shape]
    G = M.Context(dim=3, degree=3, reps=reps, hi=hi, face_role=ROLES, body_force=body, perturb=perturb, **MAT)
    if operator is not None:
        G.set_tuning("linear_operator", operator)
    if setup:
        G.linear_setup(THETA)
    return G


def _constrain(S, cons):
    """MatrixTools::apply_boundary_values with zero values on the stepping matrix: rows and columns dropped, diagonal kept"""
    import scipy.sparse as sp
    free = sp.diags((~cons).astype(float))
    return free @ S @ free + sp.diags(S.diagonal() * cons)


@pytest.fixture(scope="module")
def oracles():
    return {s: _oracle(s) for s in SHAPES}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_operators_against_the_oracle(oracles, shape):
    """y = K x, M x, A x through mf_linear_q3<true> + mf_gather against the oracle's assembled matrices, x random and non-zero
    on constrained dofs too: A (constrained columns dropped, rows of constrained dofs = diag x) on all rows, K and M (which
    stay unconstrained) on the rows of unconstrained dofs -- and here on all rows as well, since nothing replaces them"""
    P = oracles[shape]
    G = _context(shape, 1)
    assert G.get_tuning("linear_operator_active") == 1
    cons = P.constrained
    assert np.array_equal(G.constrained, cons) and cons.any()
    x = np.random.default_rng(7).standard_normal(G.n)
    assert np.all(x[cons] != 0)
    A = _constrain(P.matrix(2), cons)
    err = {}
    for which, ref in ((0, P.matrix(0) @ x), (1, P.matrix(1) @ x), (2, A @ x)):
        y = G.linear_apply(which, x)
        rows = slice(None) if which == 2 else ~cons
        err[which] = np.abs(y[rows] - ref[rows]).max() / np.abs(ref[rows]).max()
        err[which, "all"] = _relmax(y, ref)
        assert np.array_equal(G.linear_apply(which, x), y)  # fixed summation order
    print("relative max-norm errors", shape, err)
    assert all(e < 1e-13 for e in err.values()), err
    G.close()


def test_distorted_cells_against_the_assembled_operators():
    """vertices perturbed by 5 % (the oracle's linear problem takes no perturbation): mf_linear_q3<false> and
    mf_linear_diag_q3<false> against the assembled operators of a second context, read with linear_csr"""
    reps, hi = SHAPES["3x2x3"]
    nverts = int(np.prod([r + 1 for r in reps]))
    perturb = 0.05 * 0.1 * np.random.default_rng(41).standard_normal((nverts, 3))
    G0, G1 = _context("3x2x3", 0, perturb=perturb), _context("3x2x3", 1, perturb=perturb)
    assert (G0.get_tuning("linear_operator_active"), G1.get_tuning("linear_operator_active")) == (0, 1)
    cons = G0.constrained
    x = np.random.default_rng(8).standard_normal(G0.n)
    err = {}
    for which in range(3):
        ref = G0.linear_csr(which) @ x
        y = G1.linear_apply(which, x)
        rows = slice(None) if which == 2 else ~cons
        err[which] = np.abs(y[rows] - ref[rows]).max() / np.abs(ref[rows]).max()
    d0 = G0.linear_csr(2).diagonal()
    err["diag"] = _relmax(G1.linear_diagonal(), d0)
    err["diag_assembled_hook"] = _relmax(G0.linear_diagonal(), d0)
    print("relative max-norm errors (distorted)", err)
    assert all(e < 1e-12 for e in err.values()), err
    G0.close()
    G1.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_diagonal(oracles, shape):
    """the Jacobi diagonal of A from mf_linear_diag_q3<true> against the oracle's; a constrained dof keeps its diagonal, and
    its row of A x is diag_i x_i"""
    P = oracles[shape]
    G = _context(shape, 1)
    d = G.linear_diagonal()
    e = _relmax(d, P.matrix(2).diagonal())
    print("diagonal: relative max-norm error", shape, e)
    assert e < 1e-12
    cons = P.constrained
    x = np.random.default_rng(9).standard_normal(G.n)
    y = G.linear_apply(2, x)
    assert np.array_equal(y[cons], d[cons] * x[cons])
    G.close()


def _three_steps(P, Gs, seed):
    """three steps alternating "Stress" and "Force" with random interface data, as test_random_linear_model: every context of
    Gs against the oracle's direct solve; returns the CG iterations and (d, v) per step of every context"""
    rng = np.random.default_rng(seed)
    ids = P.interface_nodes
    out = [[] for _ in Gs]
    for step in range(3):
        consistent = step != 1
        t = MAT["mu"] * 1e-4 * rng.standard_normal((len(ids), 3))
        P.vec(O.L_STRESS)[:] = 0
        for c in range(3):
            P.vec(O.L_STRESS)[ids * 3 + c] = t[:, c]
        assert P.step(O.SOLVER_DIRECT, consistent)[0] == 0
        scale = max(np.abs(P.vec(O.L_RHS)).max(), 1e-30)
        for k, G in enumerate(Gs):
            G.set_interface_traction(t)
            its, res = G.linear_step(consistent, 1e-13 * scale)
            assert res <= 1e-13 * scale
            for vo, vg in ((O.L_D, 0), (O.L_V, 2)):
                ref = P.vec(vo)
                assert np.abs(G.get(vg) - ref).max() <= 1e-7 * max(np.abs(ref).max(), 1e-300), (step, vo, k)
            out[k].append((its, G.get(0), G.get(2)))
    return out


@pytest.mark.parametrize("body", [BODY, (0.0, 0.0, 0.0)], ids=["body_force", "no_body_force"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_steps(shape, body):
    """mi_linear_step on the matrix-free operators against the oracle's direct solve (absolute tolerance 1e-13 max|rhs|,
    displacement and velocity to 1e-7), and against an assembled context on the same data: CG iterations within one,
    displacement and velocity to 1e-9 (both solve to 1e-13 max|rhs|)"""
    P = _oracle(shape, body)
    G1, G0 = _context(shape, 1, body), _context(shape, 0, body)
    mf, asm = _three_steps(P, [G1, G0], seed=11)
    for (i1, d1, v1), (i0, d0, v0) in zip(mf, asm):
        print("CG iterations matrix-free / assembled", i1, i0, "d, v apart", _relmax(d1, d0), _relmax(v1, v0))
        assert abs(i1 - i0) <= 1, (i1, i0)
        assert _relmax(d1, d0) < 1e-9 and _relmax(v1, v0) < 1e-9
    # the load vector F_n carries the body force on every dof, constrained ones included: M (b, b, ...) is the assembled vector
    assert _relmax(G1.get(4), G0.get(4)) < 1e-12
    G0.close()
    G1.close()


def test_solver_type_direct_takes_the_pcg_route():
    """"solver_type" 1 on a matrix-free context: there is no matrix to factorise, mi_linear_step solves by PCG -- the route
    of a system too large for the band solver -- and matches the oracle as above"""
    P = _oracle("3x2x3")
    G = _context("3x2x3", 1, setup=False)
    G.set_tuning("solver_type", 1)
    G.linear_setup(THETA)
    (steps,) = _three_steps(P, [G], seed=12)
    assert all(its > 1 for its, _, _ in steps)  # (the band solver reports one)
    G.close()


@pytest.mark.parametrize("case", ["q3_slabs", "q2", "q3_2d"])
def test_key_refusals(case):
    """the key at 1 on a decomposed mesh, on another degree, in 2D: refused before anything changes; the context then sets up
    and steps assembled"""
    kw = dict(q3_slabs=dict(dim=3, degree=3, reps=(2, 2, 4), slabs=2), q2=dict(dim=3, degree=2, reps=(2, 2, 2)),
              q3_2d=dict(dim=2, degree=3, reps=(3, 2), hi=(1, 1)))[case]
    G = M.Context(**kw)
    with pytest.raises(M.MiError) as e:
        G.set_tuning("linear_operator", 1)
    assert e.value.code == M.MI_EINVAL and "3D Q3" in str(e.value)
    assert G.get_tuning("linear_operator") == 0
    G.linear_setup(THETA)
    assert G.get_tuning("linear_operator_active") == 0
    G.set_interface_traction((0.0, -1e3, 0.0)[:kw["dim"]])
    its, _ = G.linear_step(True, 1e-8)
    assert its >= 1 and np.all(np.isfinite(G.get(0))) and np.abs(G.get(2)).max() > 0
    G.close()


def test_key_semantics_and_what_a_matrix_free_context_refuses(oracles):
    """"linear_operator_active" follows the set-ups; no assembled array exists on a matrix-free context, so the entry points
    that need one say so; a set-up with the key at 0 brings everything back"""
    P = oracles["3x2x3"]
    G = _context("3x2x3", None, setup=False)
    assert G.get_tuning("linear_operator") == 0 and G.get_tuning("linear_operator_active") == 0
    G.set_tuning("linear_operator", 1)
    assert G.get_tuning("linear_operator_active") == 0  # read by the next set-up
    G.linear_setup(THETA)
    assert G.get_tuning("linear_operator_active") == 1
    for call in (lambda: G.linear_csr(0), lambda: G.linear_csr(2), G.assemble, G.csr, lambda: G.newmark_step(),
                 lambda: G.set_tuning("fine_level", 1)):
        with pytest.raises(M.MiError) as e:
            call()
        assert e.value.code == M.MI_EINVAL
    G.set_tuning("linear_operator", 0)
    assert G.get_tuning("linear_operator_active") == 1  # until the next set-up
    G.linear_setup(THETA)
    assert G.get_tuning("linear_operator_active") == 0
    for which in (0, 1):
        assert _relmax(G.linear_csr(which).data, P.matrix(which).data) < 1e-12
    # ... the nonlinear path included: the tangent array is allocated again
    G.set_interface_traction((0.0, -1e3, 0.0))
    G.update_acceleration()
    G.assemble()
    x = np.random.default_rng(3).standard_normal(G.n)
    assert _relmax(G.spmv(x), G.csr() @ x) < 1e-13
    G.close()


def test_default_path_is_untouched(oracles):
    """the key never set: mi_linear_apply runs the sliced-ELL product on the assembled arrays and equals csr @ x"""
    G = _context("3x2x3", None)
    assert G.get_tuning("linear_operator_active") == 0
    x = np.random.default_rng(4).standard_normal(G.n)
    for which in range(3):
        e = _relmax(G.linear_apply(which, x), G.linear_csr(which) @ x)
        assert e < 1e-13, (which, e)
    assert np.array_equal(G.linear_diagonal(), G.linear_csr(2).diagonal())
    G.close()


def test_executable_matrix_free_linear_operators(tmp_path):
    """the shipped 3D Q3 linear case plain and with MI_LINEAR_OPERATOR=1: the same output rows, and the second log names the
    matrix-free operators"""
    name = "fsi3_linear_3d_shipped"
    (tmp_path / "asm").mkdir()
    (tmp_path / "mf").mkdir()
    out0, rows0 = _run_case(name, "elasticity3d", tmp_path / "asm")
    out1, rows1 = _run_case(name, "elasticity3d", tmp_path / "mf", env={"MI_LINEAR_OPERATOR": "1"})
    assert "Linear operators: matrix-free" in out1 and "MI_LINEAR_OPERATOR ignored" not in out1
    assert "matrix-free" not in out0
    assert len(rows0) >= 3
    _check_rows(rows1, [(r[0], r[1:].reshape(-1, 3)) for r in rows0], 3)
