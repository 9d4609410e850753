"""GPU: mi_evaluate_points (Context.evaluate, the kernel family field_at_points) against tests/golden/point_eval_reference.py, the
numpy reference anchored by test_mirror_point_eval.py, and against known answers.

Meshes (tests/golden/point_eval_cases.py): 3D Q1-Q4 on 3 x 2 x 3 boxes with edges 0.1, 0.13, 0.07 and on 1 x 1 x 1, 2D Q1-Q4 on 3 x 2,
each plain (field_at_points<.., true>: xi in closed form) and with the vertices moved by 0.05 hmin randn (<.., false>: the walk over
neighbour cells and Newton on the Q1 map); one 6 x 5 x 4 Q2 mesh with 70,001 points (274 workgroups, the count's second stage).
Point counts 1, 257 and 1,000.  Points: random interior (cell, xi) pairs with xi in [0.05, 0.95] (cell exact, gradients compared),
the context's own nodes, points on the faces, edges and corners of every cell, and points outside.

Tolerance 1e-12 relmax against the reference, the project's standing tolerance for device sums against numpy: values relative to
the largest nodal value, gradients to that over the shortest edge.  Every comparison prints its worst figure.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import point_eval_cases as PC  # noqa: E402
import point_eval_reference as PE  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

TOL = 1e-12
SIX = [M.V_U, M.V_U_OLD, M.V_V, M.V_V_OLD, M.V_A, M.V_A_OLD]
MESHES = [(3, p, (3, 2, 3)) for p in (1, 2, 3, 4)] + [(3, p, (1, 1, 1)) for p in (1, 2, 3, 4)] + [(2, p, (3, 2)) for p in (1, 2, 3, 4)]
BIG = (3, 2, (6, 5, 4))
_states = {}


def _state(c):
    """ten random vectors of the case, made once"""
    key = id(c)
    if key not in _states:
        _states[key] = np.random.default_rng(5 + c["mesh"].n).standard_normal((10, c["mesh"].n))
    return _states[key]


def _loaded(c, **kw):
    G = PC.context(M, c, **kw)
    for w, v in enumerate(_state(c)):
        G.set(w, v)
    return G


def _hmin(c):
    return min(PC.EDGE[:c["dim"]])


def _compare(c, G, which, cells, xi, npts_label=""):
    """values, gradients, cells and count of the (cell, xi) pairs against the reference; returns the worst two figures"""
    m = c["mesh"]
    X = PE.points(m, cells, xi)
    val, grad, cell, nout = G.evaluate(which, X, gradients=True)
    ev = eg = 0.0
    for k, w in enumerate(which):
        rv, rg = PE.evaluate_batch(m, _state(c)[w], cells, xi)
        scale = np.abs(_state(c)[w]).max()
        ev = max(ev, np.abs(val[k] - rv).max() / scale)
        eg = max(eg, np.abs(grad[k] - rg).max() / (scale / _hmin(c)))
    print("%dD Q%d %s %s%d points: values %.2e gradients %.2e" % (c["dim"], c["p"], c["reps"], npts_label, len(cells), ev, eg))
    assert nout == 0 and np.array_equal(cell, cells)
    assert ev < TOL and eg < TOL
    return ev, eg


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_interior_points_against_reference(mesh, perturbed):
    c = PC.make_mesh(*mesh, perturbed)
    G = _loaded(c)
    rng = np.random.default_rng(77)
    for n in (1, 257):
        _compare(c, G, SIX, *PC.interior_pairs(c["mesh"], n, rng))
    G.close()


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [MESHES[1], MESHES[2], MESHES[9]])
def test_thousand_points_all_ten_vectors(mesh, perturbed):
    c = PC.make_mesh(*mesh, perturbed)
    G = _loaded(c)
    _compare(c, G, list(range(10)), *PC.interior_pairs(c["mesh"], 1000, np.random.default_rng(78)))
    G.close()


@pytest.mark.parametrize("perturbed", [False, True])
def test_many_points(perturbed):
    c = PC.make_mesh(*BIG, perturbed)
    G = _loaded(c)
    _compare(c, G, [M.V_U, M.V_V], *PC.interior_pairs(c["mesh"], 70001, np.random.default_rng(79)))
    G.close()


# ------------------------------------------------------------------ 2. the context's own nodes, cell boundaries, outside
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_own_nodes_and_cell_boundaries(mesh, perturbed):
    c = PC.make_mesh(*mesh, perturbed)
    m = c["mesh"]
    G = _loaded(c)
    val, _, cell, nout = G.evaluate(SIX, G.coords)
    err = max(np.abs(val[k].reshape(-1) - _state(c)[w]).max() / np.abs(_state(c)[w]).max() for k, w in enumerate(SIX))
    print("own nodes: %.2e" % err)
    assert nout == 0 and cell.min() >= 0 and err < TOL
    # faces, edges and corners of every cell (the domain's own among them): values only, any containing cell
    cells, xi = PC.boundary_pairs(m)
    val, _, cell, nout = G.evaluate(M.V_U, PE.points(m, cells, xi))
    ref, _ = PE.evaluate_batch(m, _state(c)[M.V_U], cells, xi)
    err = np.abs(val - ref).max() / np.abs(_state(c)[M.V_U]).max()
    print("faces, edges, corners (%d points): %.2e" % (len(cells), err))
    assert nout == 0 and err < TOL
    for k in range(len(cells)):
        assert cell[k] in PC.containing_cells(m, cells[k], xi[k]), (k, cell[k])
    G.close()


@pytest.mark.parametrize("mesh", [MESHES[1], MESHES[5], MESHES[10]])
def test_outside_points(mesh):
    c = PC.make_mesh(*mesh, False)
    dim, hi = c["dim"], np.array(c["hi"])
    G = _loaded(c)
    h = np.array(PC.EDGE[:dim])
    mid = 0.5 * hi
    pts = [mid]  # the only point inside
    for d in range(dim):
        for side in (0, 1):
            x = mid.copy()
            x[d] = hi[d] + 1e-3 * h[d] if side else -1e-3 * h[d]
            pts.append(x)
    pts += [hi + 1e-3 * h, -1e-3 * h, 1e6 * np.ones(dim), -1e300 * np.ones(dim), np.full(dim, np.nan), np.array([np.nan] + list(mid[1:])),
            np.full(dim, np.inf)]
    pts = np.array(pts)
    val, grad, cell, nout = G.evaluate([M.V_U, M.V_V], pts, gradients=True)
    assert cell[0] >= 0 and np.abs(val[:, 0]).max() > 0
    assert np.array_equal(cell[1:], np.full(len(pts) - 1, -1)) and nout == len(pts) - 1
    assert np.all(val[:, 1:] == 0.0) and np.all(grad[:, 1:] == 0.0)
    G.close()


# ------------------------------------------------------------------ 3. known answers without the reference
@pytest.mark.parametrize("mesh", MESHES)
def test_polynomials_and_affine_fields_are_reproduced(mesh):
    dim, p, _ = mesh
    for perturbed, field in ((False, PC.Poly(dim, p, PC.make_mesh(*mesh, False)["hi"], np.random.default_rng(3))),
                             (True, PC.Affine(dim, np.random.default_rng(4)))):
        c = PC.make_mesh(*mesh, perturbed)
        m = c["mesh"]
        G = PC.context(M, c)
        u = field(m.coords).reshape(-1)
        G.set(M.V_V, u)
        X = PE.points(m, *PC.interior_pairs(m, 257, np.random.default_rng(5)))
        val, grad, _, nout = G.evaluate(M.V_V, X, gradients=True)
        ev = np.abs(val - field(X)).max() / np.abs(u).max()
        eg = np.abs(grad - field.grad(X)).max() / (np.abs(u).max() / _hmin(c))
        print("%s: values %.2e gradients %.2e" % (type(field).__name__, ev, eg))
        assert nout == 0 and ev < TOL and eg < TOL
        G.close()


# ------------------------------------------------------------------ 4. the same bits
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [MESHES[2], MESHES[9]])
def test_one_call_per_vector_and_repeated_calls_give_the_same_bits(mesh, perturbed):
    c = PC.make_mesh(*mesh, perturbed)
    m = c["mesh"]
    G = _loaded(c)
    bc, bxi = PC.boundary_pairs(m)
    X = np.concatenate([PE.points(m, *PC.interior_pairs(m, 257, np.random.default_rng(6))), PE.points(m, bc, bxi)])
    val, grad, cell, _ = G.evaluate(list(range(10)), X, gradients=True)
    again = G.evaluate(list(range(10)), X, gradients=True)
    assert val.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes() and np.array_equal(cell, again[2])
    for w in range(10):
        v1, g1, c1, _ = G.evaluate(w, X, gradients=True)
        assert v1.tobytes() == val[w].tobytes() and g1.tobytes() == grad[w].tobytes() and np.array_equal(c1, cell)
    assert G.evaluate(3, X)[0].tobytes() == val[3].tobytes()  # without the gradients: the same values
    G.close()


# ------------------------------------------------------------------ 5. purity
@pytest.mark.parametrize("mesh", [MESHES[1], MESHES[2], MESHES[9]])
def test_evaluation_changes_nothing(mesh):
    c = PC.make_mesh(*mesh, True)
    m = c["mesh"]
    X = PE.points(m, *PC.interior_pairs(m, 257, np.random.default_rng(8)))
    G, H = PC.context(M, c), PC.context(M, c)
    for Y in (G, H):
        Y.set_profiling(True)
        Y.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        Y.newmark_step(tol_lin=1e-10)
    vecs = [G.get(w) for w in range(10)]
    counts = {k: v[1] for k, v in G.timings().items()}
    G.evaluate(list(range(10)), X, gradients=True)
    assert counts == {k: v[1] for k, v in G.timings().items()}
    for w in range(10):
        assert np.array_equal(vecs[w], G.get(w)), w
    _, ig = G.newmark_step(tol_lin=1e-10)
    _, ih = H.newmark_step(tol_lin=1e-10)
    assert bytes(ig) == bytes(ih)
    for w in range(10):
        assert np.array_equal(G.get(w), H.get(w)), w
    G.close()
    H.close()
    # the linear model
    G, H = PC.context(M, c), PC.context(M, c)
    for Y in (G, H):
        Y.linear_setup(0.5)
        Y.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        Y.linear_step(1, 1e-12)
    G.evaluate([M.V_U, M.V_V], X, gradients=True)  # (MI_L_DISPLACEMENT, MI_L_VELOCITY: the same slots)
    assert G.linear_step(1, 1e-12) == H.linear_step(1, 1e-12)
    for w in range(10):
        assert np.array_equal(G.get(w), H.get(w)), w
    G.close()
    H.close()


# ------------------------------------------------------------------ 6. the operator modes
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("p", [2, 3])
def test_same_values_under_the_operator_modes(p, perturbed):
    c = PC.make_mesh(3, p, (3, 2, 3), perturbed)
    m = c["mesh"]
    X = PE.points(m, *PC.interior_pairs(m, 257, np.random.default_rng(9)))
    G = PC.context(M, c)

    def load():  # (displacements small enough for an assembly: no folded cell)
        for w, v in enumerate(_state(c)):
            G.set(w, 1e-3 * _hmin(c) * v * ~m.constrained if w in (M.V_U, M.V_U_OLD, M.V_DELTA) else v)

    load()
    want = G.evaluate(SIX, X, gradients=True)
    G.set_tuning("fine_level", 1)
    G.assemble()
    got = G.evaluate(SIX, X, gradients=True)
    assert all(np.array_equal(a, b) for a, b in zip(want[:3], got[:3]))
    if p == 3:  # the matrix-free linear set-up releases the tangent array and clears the state vectors
        G.set_tuning("linear_operator", 1)
        G.linear_setup(0.5)
        assert G.get_tuning("linear_operator_active") == 1
        load()
        got = G.evaluate(SIX, X, gradients=True)
        assert all(np.array_equal(a, b) for a, b in zip(want[:3], got[:3]))
    G.close()


# ------------------------------------------------------------------ 7. refusals
def test_teams_are_refused():
    c = PC.make_mesh(3, 2, (2, 2, 4), False)
    T = PC.context(M, c, slabs=2)
    assert T.comm_info()[0] == 2
    with pytest.raises(M.MiError) as err:
        T.evaluate(M.V_U, np.zeros((1, 3)))
    assert err.value.code == M.MI_EINVAL and "one slab only" in str(err.value)
    T.close()


def test_argument_errors():
    c = PC.make_mesh(2, 2, (3, 2), False)
    G = _loaded(c)
    L = M.lib()
    X = np.array([[0.05, 0.05], [0.2, 0.1]])
    val = np.full((2, 2, 2), 7.0)
    which = (C.c_int * 2)(M.V_U, M.V_V)
    dp, vp = val.ctypes.data_as(C.POINTER(C.c_double)), X.ctypes.data_as(C.POINTER(C.c_double))
    nout = C.c_int64(5)
    assert L.mi_evaluate_points(None, 2, which, 2, vp, dp, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_points(G.h, 2, None, 2, vp, dp, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_points(G.h, 2, which, 2, None, dp, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_points(G.h, 2, which, 2, vp, None, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_points(G.h, 2, which, -1, vp, dp, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_points(G.h, 0, which, 2, vp, dp, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_points(G.h, 11, which, 2, vp, dp, None, None, None) == M.MI_EINVAL
    for bad in (-1, 10):
        assert L.mi_evaluate_points(G.h, 2, (C.c_int * 2)(M.V_U, bad), 2, vp, dp, None, None, None) == M.MI_EINVAL
    assert np.all(val == 7.0)
    assert L.mi_evaluate_points(G.h, 2, which, 0, vp, dp, None, None, C.byref(nout)) == M.MI_OK  # no points: nothing written
    assert np.all(val == 7.0) and nout.value == 0
    assert L.mi_evaluate_points(G.h, 2, which, 2, vp, dp, None, None, None) == M.MI_OK  # every output but the values is optional
    want, _, _, _ = G.evaluate([M.V_U, M.V_V], X)
    assert np.array_equal(val, want)
    G.close()
