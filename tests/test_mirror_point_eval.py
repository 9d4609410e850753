"""CPU anchor of tests/golden/point_eval_reference.py, the numpy reference the device's point evaluation and state transfer are
held to (test_gpu_point_eval.py, test_gpu_state_transfer.py).  No device, no library:

  (a) N_a(xi_b) = delta_ab at the element's support points, 2D / 3D, p = 1..4
  (b) polynomials of degree <= p per direction and their gradients are reproduced on box meshes (an FE_Q(p) function there)
  (c) affine fields A X + b are reproduced on distorted meshes, gradient = A everywhere (the Q1 map reproduces X itself)
  (d) conditioning: the double evaluation agrees with the same sums in long double
  (e) evaluate_batch (the vectorised form the large device cases use) equals evaluate
  (f) nodes_as_points / refine_pairs map back to the nodes' coordinates, and interpolate() onto the same mesh is the identity

Tolerance 1e-12 of the field's largest nodal value (gradients: of that over the shortest edge): sums of at most 125 products of
O(1) bases, whose rounding stays below 1e-14.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import point_eval_cases as PC  # noqa: E402
import point_eval_reference as PE  # noqa: E402

TOL = 1e-12
ELEMENTS = [(2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (3, 3), (3, 4)]
REPS = {2: (3, 2), 3: (3, 2, 3)}


@pytest.mark.parametrize("dim,p", ELEMENTS)
def test_basis_is_nodal(dim, p):
    nodes = Mi.feq_nodes(p)
    npc = (p + 1) ** dim
    for b in range(npc):
        xi = [nodes[(b // (p + 1) ** d) % (p + 1)] for d in range(dim)]
        N, _ = Mi.shape_at(dim, p, nodes, xi)
        assert np.abs(N - np.eye(npc)[b]).max() < 1e-14


def _errors(c, field, rng, n=60):
    m = c["mesh"]
    u = field(m.coords).reshape(-1)
    cells, xi = PC.interior_pairs(m, n, rng)
    X = PE.points(m, cells, xi)
    val, grad = PE.evaluate(m, u, cells, xi)
    scale = np.abs(u).max()
    return np.abs(val - field(X)).max() / scale, np.abs(grad - field.grad(X)).max() / (scale / min(PC.EDGE[:m.dim]))


@pytest.mark.parametrize("dim,p", ELEMENTS)
def test_polynomials_are_reproduced_on_boxes(dim, p):
    c = PC.make_mesh(dim, p, REPS[dim], False)
    rng = np.random.default_rng(10 * dim + p)
    ev, eg = _errors(c, PC.Poly(dim, p, c["hi"], rng), rng)
    print("values %.2e gradients %.2e" % (ev, eg))
    assert ev < TOL and eg < TOL


@pytest.mark.parametrize("dim,p", ELEMENTS)
def test_affine_fields_are_reproduced_on_distorted_meshes(dim, p):
    c = PC.make_mesh(dim, p, REPS[dim], True)
    rng = np.random.default_rng(20 * dim + p)
    ev, eg = _errors(c, PC.Affine(dim, rng), rng)
    print("values %.2e gradients %.2e" % (ev, eg))
    assert ev < TOL and eg < TOL


def _evaluate_long_double(mesh, u, cells, xi):
    """the values of PE.evaluate with bases and sums in long double"""
    dim, p = mesh.dim, mesh.p
    ld = np.longdouble
    nodes = Mi.feq_nodes(p).astype(ld)
    U = np.asarray(u).reshape(-1, dim).astype(ld)
    out = np.zeros((len(cells), dim), dtype=ld)
    for k, (c, x) in enumerate(zip(cells, xi)):
        one = []
        for d in range(dim):
            L = np.ones(p + 1, dtype=ld)
            for a in range(p + 1):
                for m in range(p + 1):
                    if m != a:
                        L[a] *= (ld(x[d]) - nodes[m]) / (nodes[a] - nodes[m])
            one.append(L)
        conn = mesh.cells[c][0]
        for a in range((p + 1) ** dim):
            w = ld(1)
            for d in range(dim):
                w *= one[d][(a // (p + 1) ** d) % (p + 1)]
            out[k] += w * U[conn[a]]
    return out


@pytest.mark.parametrize("dim,p", [(2, 4), (3, 2), (3, 4)])
def test_agrees_with_long_double(dim, p):
    c = PC.make_mesh(dim, p, REPS[dim], True)
    m = c["mesh"]
    rng = np.random.default_rng(30 * dim + p)
    u = rng.standard_normal(m.n)
    cells, xi = PC.interior_pairs(m, 40, rng)
    val, _ = PE.evaluate(m, u, cells, xi)
    err = float(np.abs(val - _evaluate_long_double(m, u, cells, xi)).max() / np.abs(u).max())
    print("double against long double %.2e" % err)
    assert err < 1e-14


@pytest.mark.parametrize("dim,p,perturbed", [(2, 3, True), (3, 2, True), (3, 3, False), (3, 4, True)])
def test_batch_form_equals_pointwise_form(dim, p, perturbed):
    c = PC.make_mesh(dim, p, REPS[dim], perturbed)
    m = c["mesh"]
    rng = np.random.default_rng(40 * dim + p)
    u = rng.standard_normal(m.n)
    cells, xi = PC.interior_pairs(m, 50, rng)
    bc, bxi = PC.boundary_pairs(m)
    cells, xi = np.concatenate([cells, bc[:50]]), np.concatenate([xi, bxi[:50]])
    v0, g0 = PE.evaluate(m, u, cells, xi)
    v1, g1 = PE.evaluate_batch(m, u, cells, xi)
    assert np.abs(v1 - v0).max() < 1e-14 * np.abs(u).max()
    assert np.abs(g1 - g0).max() < 1e-13 * np.abs(u).max() / min(PC.EDGE[:dim])


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 3)])
def test_node_pairs_and_refinement_pairs(dim, p):
    c = PC.make_mesh(dim, p, REPS[dim], True)
    m = c["mesh"]
    cells, xi = PE.nodes_as_points(m)
    assert np.abs(PE.points(m, cells, xi) - m.coords).max() < 1e-15
    u = np.random.default_rng(50 + dim).standard_normal(m.n)
    same = PE.interpolate(m, u, m)
    assert np.abs(same - u * ~m.constrained).max() < 1e-14 * np.abs(u).max()
    coarse = PC.make_mesh(dim, p, REPS[dim], False)["mesh"]
    fine = PC.make_mesh(dim, p, REPS[dim], False, refine=2)["mesh"]
    cells, xi = PE.refine_pairs(coarse, fine)
    assert np.abs(PE.points(coarse, cells, xi) - fine.coords).max() < 1e-15
