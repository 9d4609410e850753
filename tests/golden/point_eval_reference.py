"""Numpy reference of the point evaluation (mi_evaluate_points, mi_state_transfer), from mirror.py's pieces alone: Mesh, q1_map,
q1_jacobian, shape_at.

It needs no point location: test points are made as (cell, xi) pairs and mapped to X by the d-linear map of the cell, so each is
inside its cell by construction.  Cells are numbered as mirror.Mesh.cells lists them: lexicographic, x fastest -- the `cell` the
device returns.

  points()            X [n, dim] of (cell, xi) pairs
  evaluate()          u_h and d u_c / d X_d there, point by point with mirror.shape_at / q1_jacobian
  evaluate_batch()    the same sums vectorised over the points (einsum), for the large cases; test_mirror_point_eval.py holds it to
                      evaluate()
  nodes_as_points()   every node of a mesh as a (cell, xi) pair of its first containing cell: the points of a transfer
  interpolate()       nodal interpolation of a field onto another mesh of the SAME cells (any degree): mi_state_transfer's
                      definition where no location is needed
  refine_pairs()      the nodes of a mesh whose cells are nested in a coarser box mesh's, as (coarse cell, xi) pairs
"""
import numpy as np

from mirror import feq_nodes, q1_jacobian, q1_map, shape_at


def points(mesh, cells, xi):
    return np.array([q1_map(mesh.dim, mesh.cells[c][1], x) for c, x in zip(cells, xi)])


def evaluate(mesh, u, cells, xi):
    """(values [n, dim], gradients [n, dim, dim]) of the field u (mesh.n dofs) at the (cell, xi) pairs"""
    dim, p = mesh.dim, mesh.p
    nodes = feq_nodes(p)
    U = np.asarray(u, float).reshape(-1, dim)
    val, grad = np.zeros((len(cells), dim)), np.zeros((len(cells), dim, dim))
    for k, (c, x) in enumerate(zip(cells, xi)):
        conn, verts, _ = mesh.cells[c]
        N, dN = shape_at(dim, p, nodes, x)
        Jm = q1_jacobian(dim, verts, x)
        val[k] = U[conn].T @ N
        grad[k] = U[conn].T @ (dN @ np.linalg.inv(Jm))
    return val, grad


def evaluate_batch(mesh, u, cells, xi):
    """evaluate() with the points as the leading axis of every array"""
    dim, p = mesh.dim, mesh.p
    nodes = feq_nodes(p)
    cells, xi = np.asarray(cells), np.asarray(xi, float)
    n, np1 = len(cells), p + 1
    L = np.ones((dim, n, np1))
    dL = np.zeros((dim, n, np1))
    for d in range(dim):
        for a in range(np1):
            for m in range(np1):
                if m != a:
                    L[d, :, a] *= (xi[:, d] - nodes[m]) / (nodes[a] - nodes[m])
            for k in range(np1):
                if k != a:
                    t = np.full(n, 1.0 / (nodes[a] - nodes[k]))
                    for m in range(np1):
                        if m not in (a, k):
                            t *= (xi[:, d] - nodes[m]) / (nodes[a] - nodes[m])
                    dL[d, :, a] += t
    npc = np1 ** dim
    N, dN = np.ones((n, npc)), np.ones((n, npc, dim))
    for a in range(npc):
        ai = [(a // np1 ** d) % np1 for d in range(dim)]
        for d in range(dim):
            N[:, a] *= L[d, :, ai[d]]
            for k in range(dim):
                dN[:, a, k] *= (dL if d == k else L)[d, :, ai[d]]
    conn = np.array([c[0] for c in mesh.cells])[cells]
    verts = np.array([c[1] for c in mesh.cells])[cells]  # [n, 2^dim, dim]
    Jm = np.zeros((n, dim, dim))
    for v in range(1 << dim):
        for j in range(dim):
            g = np.full(n, 1.0 if (v >> j) & 1 else -1.0)
            for d in range(dim):
                if d != j:
                    g = g * (xi[:, d] if (v >> d) & 1 else 1 - xi[:, d])
            Jm[:, :, j] += verts[:, v, :] * g[:, None]
    Ue = np.asarray(u, float).reshape(-1, dim)[conn]  # [n, npc, dim]
    val = np.einsum("na,nac->nc", N, Ue)
    grad = np.einsum("nac,nae,ned->ncd", Ue, dN, np.linalg.inv(Jm))
    return val, grad


def nodes_as_points(mesh):
    """(cells [nnodes], xi [nnodes, dim]): every node in the first cell (lexicographic) that contains it"""
    dim, p = mesh.dim, mesh.p
    nodes = feq_nodes(p)
    cells = np.full(mesh.nnodes, -1)
    xi = np.zeros((mesh.nnodes, dim))
    for c, (conn, _, _) in enumerate(mesh.cells):
        for a, node in enumerate(conn):
            if cells[node] < 0:
                cells[node] = c
                xi[node] = [nodes[(a // (p + 1) ** d) % (p + 1)] for d in range(dim)]
    return cells, xi


def interpolate(src, u, dst):
    """src's field u at dst's nodes, dst a mesh of the same cells (same box, reps and perturbation; any degree), constrained dofs
    of dst set to 0: what mi_state_transfer(dst, src) writes into each vector"""
    assert src.reps == dst.reps and src.dim == dst.dim
    cells, xi = nodes_as_points(dst)
    val, _ = evaluate_batch(src, u, cells, xi)
    out = val.reshape(-1)
    out[dst.constrained] = 0.0
    return out


def refine_pairs(coarse, fine):
    """the nodes of `fine` (a box mesh whose reps are integer multiples of coarse's, same box) as (coarse cell, xi) pairs"""
    dim = coarse.dim
    ratio = [f // c for f, c in zip(fine.reps, coarse.reps)]
    assert all(f == c * r for f, c, r in zip(fine.reps, coarse.reps, ratio))
    fcells, fxi = nodes_as_points(fine)
    cells, xi = np.zeros(fine.nnodes, int), np.zeros((fine.nnodes, dim))
    for k in range(fine.nnodes):
        f, cid, stride = fcells[k], 0, 1
        for d in range(dim):
            fi = f % fine.reps[d]
            f //= fine.reps[d]
            cid += stride * (fi // ratio[d])
            stride *= coarse.reps[d]
            xi[k, d] = (fi % ratio[d] + fxi[k, d]) / ratio[d]
        cells[k] = cid
    return cells, xi
