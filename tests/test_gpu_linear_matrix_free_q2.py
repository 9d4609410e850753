"""The linear model without matrices on 3D Q2 meshes (tuning "linear_operator" 2 on one slab): K, M and the stepping matrix
A = M + theta^2 dt^2 K as one kernel on the model's own 3 x 3 x 3 rule (mf_linear_q2, two cells per wave) + the slot gathers,
the diagonal of A from mf_linear_diag_q2, the body force as M (b, b, ...).  The tests of test_gpu_linear_matrix_free.py one by
one at that file's tolerances, on the smallest meshes that reach every branch of a two-cells-per-wave kernel:

  1x1x1   one cell: the wave's second half mirrors the first, every node on the boundary
  3x3x1   9 cells, an odd count: the last pair is half empty, 5 pairs are no multiple of the 8 XCD chunks, one cell thick
  3x2x3   18 cells, 9 pairs: nodes shared across faces, edges and corners in every direction

and on top of them: NaN on the constrained entries of x (the mask is a select), every slot layout, what value 2 means on the
other elements and on a team, the energies and the vibration modes through the matrix-free products."""
import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg

M = load_pkg()
pytestmark = pytest.mark.gpu

ROLES = [O.FACE_CLAMPED] + [O.FACE_INTERFACE] * 5  # one clamped face, the others interface
THETA = 0.6
MAT = dict(mu=0.5e6, nu=0.4, rho=1000.0, delta_t=0.005)
BODY = (0.0, -9.81, 2.0)
SHAPES = {"1x1x1": ((1, 1, 1), (0.5, 0.35, 0.55)), "3x3x1": ((3, 3, 1), (1.5, 0.9, 0.4)), "3x2x3": ((3, 2, 3), (1.5, 0.7, 1.1))}
L_D, L_V = 0, 2  # the linear model's displacement and velocity among the context's vectors
TOL_MODES = 1e-8  # tests/test_gpu_linear_modes.py


def _relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _oracle(shape, body=BODY, degree=2):
    reps, hi = SHAPES[shape]
    return O.LinearProblem(O.make_desc(dim=3, degree=degree, reps=reps, hi=hi, face_role=ROLES, theta=THETA, body_force=body, **MAT))


def _context(shape, operator, body=BODY, perturb=None, setup=True, degree=2, keys=()):
    reps, hi = SHAPES[shape]
    G = M.Context(dim=3, degree=degree, reps=reps, hi=hi, face_role=ROLES, body_force=body, perturb=perturb, **MAT)
    for k, v in keys:
        G.set_tuning(k, v)
    if operator is not None:
        G.set_tuning("linear_operator", operator)
    if setup:
        G.linear_setup(THETA)
    return G


def _perturbation(shape, seed):
    reps, _ = SHAPES[shape]
    nverts = int(np.prod([r + 1 for r in reps]))
    return 0.05 * 0.1 * np.random.default_rng(seed).standard_normal((nverts, 3))


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
    """y = K x, M x, A x through mf_linear_q2<true, .> + mf_gather against the oracle's assembled matrices, x random and
    non-zero on constrained dofs too: A (constrained columns dropped, rows of constrained dofs = diag x) on all rows, K and M
    (which stay unconstrained) on the rows of unconstrained dofs -- and on all rows as well, since nothing replaces them"""
    P = oracles[shape]
    G = _context(shape, 2)
    assert G.get_tuning("linear_operator") == 2 and G.get_tuning("linear_operator_active") == 2
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


@pytest.mark.parametrize("perturbed", [False, True], ids=["boxes", "distorted"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_constrained_entries_of_x_are_masked_by_a_select(shape, perturbed):
    """A x with NaN on the constrained entries of x: on the free rows the bits of the product with zeros there (a mask by
    multiplication would spread the NaN over every row of the neighbouring cells)"""
    G = _context(shape, 2, perturb=_perturbation(shape, 5) if perturbed else None)
    cons = G.constrained
    x = np.random.default_rng(17).standard_normal(G.n)
    x0, xn = x.copy(), x.copy()
    x0[cons], xn[cons] = 0.0, np.nan
    y0, yn = G.linear_apply(2, x0), G.linear_apply(2, xn)
    assert np.all(np.isfinite(y0)) and np.abs(y0[~cons]).max() > 0
    assert np.array_equal(yn[~cons], y0[~cons])
    G.close()


@pytest.mark.parametrize("shape", ["3x2x3", "3x3x1"])
def test_distorted_cells_against_the_assembled_operators(shape):
    """vertices perturbed by 5 % (the oracle's linear problem takes no perturbation): mf_linear_q2<false, .> and
    mf_linear_diag_q2<false, false> against the assembled operators of a second context, read with linear_csr"""
    perturb = _perturbation(shape, 41)
    G0, G2 = _context(shape, 0, perturb=perturb), _context(shape, 2, perturb=perturb)
    assert (G0.get_tuning("linear_operator_active"), G2.get_tuning("linear_operator_active")) == (0, 2)
    cons = G0.constrained
    x = np.random.default_rng(8).standard_normal(G0.n)
    err = {}
    for which in range(3):
        ref = G0.linear_csr(which) @ x
        y = G2.linear_apply(which, x)
        rows = slice(None) if which == 2 else ~cons
        err[which] = np.abs(y[rows] - ref[rows]).max() / np.abs(ref[rows]).max()
    d0 = G0.linear_csr(2).diagonal()
    err["diag"] = _relmax(G2.linear_diagonal(), d0)
    err["diag_assembled_hook"] = _relmax(G0.linear_diagonal(), d0)
    print("relative max-norm errors (distorted)", shape, err)
    assert all(e < 1e-12 for e in err.values()), err
    G0.close()
    G2.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_diagonal(oracles, shape):
    """the Jacobi diagonal of A from mf_linear_diag_q2<true, false> against the oracle's; a constrained dof keeps its diagonal,
    and its row of A x is diag_i x_i"""
    P = oracles[shape]
    G = _context(shape, 2)
    d = G.linear_diagonal()
    e = _relmax(d, P.matrix(2).diagonal())
    print("diagonal: relative max-norm error", shape, e)
    assert e < 1e-12
    cons = P.constrained
    x = np.random.default_rng(9).standard_normal(G.n)
    y = G.linear_apply(2, x)
    assert np.array_equal(y[cons], d[cons] * x[cons])
    G.close()


@pytest.mark.parametrize("perturbed", [False, True], ids=["boxes", "distorted"])
def test_every_slot_layout(oracles, perturbed):
    """"mf_slots_cell_major" 0, 1 and 2 before the set-up builds the slots (node-major, cell-major, line-major): the kernel
    stores through the slot table or by arithmetic, the gathers sum a node's contributions in the same order in all three, so
    products and diagonal have the same bits -- and, on boxes, are the oracle's"""
    shape = "3x2x3"
    perturb = _perturbation(shape, 43) if perturbed else None
    x = np.random.default_rng(10).standard_normal(oracles[shape].n)
    out = []
    for layout in (0, 1, 2):
        G = _context(shape, 2, perturb=perturb, keys=[("mf_slots_cell_major", layout)])
        assert G.get_tuning("linear_operator_active") == 2
        out.append([G.linear_apply(w, x) for w in range(3)] + [G.linear_diagonal()])
        G.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    if not perturbed:
        P = oracles[shape]
        assert _relmax(out[0][0], P.matrix(0) @ x) < 1e-13 and _relmax(out[0][3], P.matrix(2).diagonal()) < 1e-12


@pytest.mark.parametrize("perturbed", [False, True], ids=["boxes", "distorted"])
@pytest.mark.parametrize("shape", ["3x3x1", "3x2x3"])
def test_node_ids_from_the_connectivity(shape, perturbed):
    """"cell_lattice" 0: the kernel reads its node ids from the connectivity instead of computing them (mf_linear_q2<., false>).
    The same nodes, so the same bits"""
    perturb = _perturbation(shape, 47) if perturbed else None
    Ga, Gb = _context(shape, 2, perturb=perturb), _context(shape, 2, perturb=perturb, keys=[("cell_lattice", 0)])
    assert Ga.get_tuning("cell_lattice") == 1 and Gb.get_tuning("cell_lattice") == 0
    x = np.random.default_rng(15).standard_normal(Ga.n)
    for which in range(3):
        ya = Ga.linear_apply(which, x)
        assert np.abs(ya).max() > 0 and np.array_equal(Gb.linear_apply(which, x), ya)
    Ga.close()
    Gb.close()


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
            for vo, vg in ((O.L_D, L_D), (O.L_V, L_V)):
                ref = P.vec(vo)
                assert np.abs(G.get(vg) - ref).max() <= 1e-7 * max(np.abs(ref).max(), 1e-300), (step, vo, k)
            out[k].append((its, G.get(L_D), G.get(L_V)))
    return out


@pytest.mark.parametrize("body", [BODY, (0.0, 0.0, 0.0)], ids=["body_force", "no_body_force"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_steps(shape, body):
    """mi_linear_step on the matrix-free operators against the oracle's direct solve (absolute tolerance 1e-13 max|rhs|,
    displacement and velocity to 1e-7), and against an assembled context on the same data: CG iterations within one,
    displacement and velocity to 1e-9 (both solve to 1e-13 max|rhs|)"""
    P = _oracle(shape, body)
    G2, G0 = _context(shape, 2, body), _context(shape, 0, body)
    mf, asm = _three_steps(P, [G2, G0], seed=11)
    for (i2, d2, v2), (i0, d0, v0) in zip(mf, asm):
        print("CG iterations matrix-free / assembled", i2, i0, "d, v apart", _relmax(d2, d0), _relmax(v2, v0))
        assert abs(i2 - i0) <= 1, (i2, i0)
        assert _relmax(d2, d0) < 1e-9 and _relmax(v2, v0) < 1e-9
    # the load vector F_n carries the body force on every dof, constrained ones included: M (b, b, ...) is the assembled vector
    assert _relmax(G2.get(4), G0.get(4)) < 1e-12
    G0.close()
    G2.close()


def test_solver_type_direct_takes_the_pcg_route():
    """"solver_type" 1 on a matrix-free context: there is no matrix to factorise, mi_linear_step solves by PCG -- the route
    of a system too large for the band solver -- and matches the oracle as above"""
    P = _oracle("3x2x3")
    G = _context("3x2x3", 2, setup=False)
    G.set_tuning("solver_type", 1)
    G.linear_setup(THETA)
    (steps,) = _three_steps(P, [G], seed=12)
    assert all(its > 1 for its, _, _ in steps)  # (the band solver reports one)
    G.close()


@pytest.mark.parametrize("case", ["q2_2d", "q1", "q4", "q2_slabs"])
def test_key_refusals(case):
    """the key at 2 in 2D, on degrees 1 and 4, on a decomposed Q2 mesh: refused before anything changes, the message names the
    meshes it exists for; the context then sets up and steps assembled"""
    kw = dict(q2_2d=dict(dim=2, degree=2, reps=(3, 2), hi=(1, 1)), q1=dict(dim=3, degree=1, reps=(2, 2, 2)),
              q4=dict(dim=3, degree=4, reps=(1, 1, 2)), q2_slabs=dict(dim=3, degree=2, reps=(2, 2, 4), slabs=2))[case]
    G = M.Context(**kw)
    with pytest.raises(M.MiError) as e:
        G.set_tuning("linear_operator", 2)
    assert e.value.code == M.MI_EINVAL and "3D Q2 and Q3" in str(e.value)
    assert G.get_tuning("linear_operator") == 0
    G.linear_setup(THETA)
    assert G.get_tuning("linear_operator_active") == 0
    G.set_interface_traction((0.0, -1e3, 0.0)[:kw["dim"]])
    its, _ = G.linear_step(True, 1e-8)
    assert its >= 1 and np.all(np.isfinite(G.get(L_D))) and np.abs(G.get(L_V)).max() > 0
    G.close()


def test_value_2_on_a_q3_mesh_is_value_1():
    """3D Q3: 2 reads back as 2, runs mf_linear_q3 ("linear_operator_active" 1) and gives the bits of a context set with 1"""
    Ga, Gb = _context("3x2x3", 2, degree=3), _context("3x2x3", 1, degree=3)
    assert (Ga.get_tuning("linear_operator"), Gb.get_tuning("linear_operator")) == (2, 1)
    assert Ga.get_tuning("linear_operator_active") == 1 and Gb.get_tuning("linear_operator_active") == 1
    x = np.random.default_rng(13).standard_normal(Ga.n)
    for which in range(3):
        assert np.array_equal(Ga.linear_apply(which, x), Gb.linear_apply(which, x))
    assert np.array_equal(Ga.linear_diagonal(), Gb.linear_diagonal())
    Ga.close()
    Gb.close()


def test_key_semantics_and_what_a_matrix_free_context_refuses(oracles):
    """"linear_operator_active" follows the set-ups; no assembled array exists on a matrix-free context, so the entry points
    that need one say so; a set-up with the key at 0 brings everything back"""
    P = oracles["3x2x3"]
    G = _context("3x2x3", None, setup=False)
    assert G.get_tuning("linear_operator") == 0 and G.get_tuning("linear_operator_active") == 0
    G.set_tuning("linear_operator", 2)
    assert G.get_tuning("linear_operator") == 2 and G.get_tuning("linear_operator_active") == 0  # read by the next set-up
    G.linear_setup(THETA)
    assert G.get_tuning("linear_operator_active") == 2
    x = np.random.default_rng(3).standard_normal(G.n)
    for call in (lambda: G.linear_csr(0), lambda: G.linear_csr(2), G.assemble, G.csr, lambda: G.newmark_step(),
                 lambda: G.cg_solve(1e-8, 10), lambda: G.spmv(x), lambda: G.tangent_modes(1),
                 lambda: G.set_tuning("fine_level", 1)):
        with pytest.raises(M.MiError) as e:
            call()
        assert e.value.code == M.MI_EINVAL
    G.set_tuning("linear_operator", 0)
    assert G.get_tuning("linear_operator_active") == 2  # until the next set-up
    G.linear_setup(THETA)
    assert G.get_tuning("linear_operator_active") == 0
    for which in (0, 1):
        assert _relmax(G.linear_csr(which).data, P.matrix(which).data) < 1e-12
    # ... the nonlinear path included: the tangent array is allocated again
    G.set_interface_traction((0.0, -1e3, 0.0))
    G.update_acceleration()
    G.assemble()
    assert _relmax(G.spmv(x), G.csr() @ x) < 1e-13
    G.close()


def test_energies_through_the_matrix_free_products():
    """mi_linear_energy on a random state: 1/2 d.K d, 1/2 v.M v and -d.f_body through mf_linear_q2 + mf_gather_dot against the
    sliced-ELL products of an assembled context"""
    G2, G0 = _context("3x2x3", 2), _context("3x2x3", 0)
    rng = np.random.default_rng(14)
    free = ~G0.constrained
    d, v = 1e-3 * rng.standard_normal(G0.n) * free, rng.standard_normal(G0.n) * free
    for G in (G2, G0):
        G.set(L_D, d)
        G.set(L_V, v)
    e2, e0 = G2.linear_energy(), G0.linear_energy()
    print("energies matrix-free", e2, "assembled", e0)
    for k in ("strain", "kinetic", "body"):
        assert e0[k] != 0 and abs(e2[k] - e0[k]) <= 1e-12 * abs(e0[k]), (k, e2[k], e0[k])
    G0.close()
    G2.close()


def test_modes_through_the_matrix_free_products():
    """mi_linear_modes, 3 modes at the tolerance of tests/test_gpu_linear_modes.py: converged on both forms, the eigenvalues
    of the matrix-free context are those of the assembled one to that tolerance"""
    G2, G0 = _context("3x2x3", 2), _context("3x2x3", 0)
    o2, o0 = G2.linear_modes(3, tol=TOL_MODES), G0.linear_modes(3, tol=TOL_MODES)
    print("eigenvalues matrix-free", o2["lam"], "assembled", o0["lam"], "iterations", o2["its"], o0["its"])
    assert np.all(o2["residual"] <= TOL_MODES) and np.all(o0["residual"] <= TOL_MODES)
    assert np.all(o0["lam"] > 0) and np.all(np.abs(o2["lam"] - o0["lam"]) <= TOL_MODES * o0["lam"].max())
    G0.close()
    G2.close()
