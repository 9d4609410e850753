"""Dense numpy reference of the consistent mass and of the L2 projection between two meshes (mi_mass_apply, mi_mass_solve,
mi_project_load, mi_state_project), from mirror.py's Mesh, _rule, _q1_jacobians and shape_at.

  M        the unit-density scalar mass on QGauss(p + 2), dense [nnodes, nnodes]; the vector mass is M on every component
  load     b_(i,c) = sum_{dst cells} sum_q N_i(xi_q) w_c^src(X_q) JxW(q) on the composite rule: every dst cell cut into sub^dim
           boxes in xi with QGauss(p + 2) on each.  The points are (cell, xi) pairs of dst; src is located by floor on box meshes
           or by identity on equal lattices (the same reps and the same vertices), never by a search
  solve    w = 0 on constrained dofs, M_ff w_f = b_f, dense, component by component (the constraint flags differ by component)

The 1D Lagrange bases are evaluated for whole arrays of points (lagrange_many); test_mirror_projection.py holds them to
mirror.shape_at.
"""
import numpy as np

import mirror as Mi


def lagrange_many(nodes, x):
    """N[..., a] of the 1D Lagrange basis on `nodes` at the points x[...]"""
    x = np.asarray(x, float)
    N = np.ones(x.shape + (len(nodes),))
    for a in range(len(nodes)):
        for m in range(len(nodes)):
            if m != a:
                N[..., a] *= (x - nodes[m]) / (nodes[a] - nodes[m])
    return N


def shape_many(dim, p, xi):
    """N[..., A] of the tensor-product basis (A lexicographic, x fastest) at the unit points xi[..., dim]"""
    one = [lagrange_many(Mi.feq_nodes(p), xi[..., d]) for d in range(dim)]
    if dim == 2:
        N = np.einsum("...j,...i->...ji", one[1], one[0])
    else:
        N = np.einsum("...k,...j,...i->...kji", one[2], one[1], one[0])
    return N.reshape(xi.shape[:-1] + ((p + 1) ** dim,))


def cell_jxw(mesh, xi, w):
    """JxW[E, Q] of the points xi[Q, dim] with weights w[Q] in every cell"""
    verts = np.array([c[1] for c in mesh.cells])
    return np.linalg.det(Mi._q1_jacobians(mesh.dim, verts, xi)) * w[None, :]


def scalar_mass(mesh):
    xi, w, N, _ = Mi._rule(mesh.dim, mesh.p, mesh.p + 2)
    JxW = cell_jxw(mesh, xi, w)
    M = np.zeros((mesh.nnodes, mesh.nnodes))
    for e, (conn, _, _) in enumerate(mesh.cells):
        M[np.ix_(conn, conn)] += np.einsum("qa,qb,q->ab", N, N, JxW[e])
    return M


def mass_apply(M, x, dim, constrained=None):
    """y = (M on every component) x for x[..., n]; constrained: the masked product"""
    x = np.array(x, float)
    if constrained is not None:
        x[..., constrained] = 0.0
    y = np.zeros_like(x)
    for c in range(dim):
        y[..., c::dim] = x[..., c::dim] @ M.T
    if constrained is not None:
        y[..., constrained] = 0.0
    return y


def solve(M, b, dim, constrained):
    """w[..., n]: 0 on constrained dofs, M_ff w_f = b_f"""
    b = np.asarray(b, float)
    w = np.zeros_like(b)
    for c in range(dim):
        free = ~constrained[c::dim]
        wc = np.zeros(b[..., c::dim].shape)
        wc[..., free] = np.linalg.solve(M[np.ix_(free, free)], b[..., c::dim][..., free].T).T
        w[..., c::dim] = wc
    return w


def free_blocks(M, dim, constrained):
    """the distinct free-free blocks of the vector mass (one per set of component flags)"""
    seen, out = set(), []
    for c in range(dim):
        free = ~constrained[c::dim]
        if free.tobytes() not in seen:
            seen.add(free.tobytes())
            out.append(M[np.ix_(free, free)])
    return out


def composite_rule(dim, p, sub):
    """xi[Q, dim], w[Q] of the composite rule, x fastest, per direction index k = box * (p + 2) + gauss point"""
    qx, qw = Mi.gauss01(p + 2)
    x1 = np.array([(s + qx[g]) / sub for s in range(sub) for g in range(p + 2)])
    w1 = np.array([qw[g] / sub for s in range(sub) for g in range(p + 2)])
    pts = [q[::-1] for q in np.ndindex(*([len(x1)] * dim))]
    return np.array([[x1[k] for k in qi] for qi in pts]), np.array([np.prod([w1[k] for k in qi]) for qi in pts])


def _is_box(mesh):
    h = (mesh.hi - mesh.lo) / np.array(mesh.reps)
    for e, (_, verts, _) in enumerate(mesh.cells):
        ci = [(e // int(np.prod(mesh.reps[:d]))) % mesh.reps[d] for d in range(mesh.dim)]
        ref = np.array([[mesh.lo[d] + h[d] * (ci[d] + ((v >> d) & 1)) for d in range(mesh.dim)] for v in range(1 << mesh.dim)])
        if not np.array_equal(verts, ref):
            return False
    return True


def locate(dst, src, xi):
    """(cell[E, Q], xi_src[E, Q, dim]) of the points (e, xi[q]) of dst's cells in src: the identity on equal lattices, floor on
    boxes"""
    E, Q = len(dst.cells), len(xi)
    if dst.reps == src.reps and all(np.array_equal(a[1], b[1]) for a, b in zip(dst.cells, src.cells)):
        return np.repeat(np.arange(E)[:, None], Q, axis=1), np.broadcast_to(xi, (E, Q, dst.dim)).copy()
    assert _is_box(dst) and _is_box(src), "points are located by floor on boxes or by identity on equal lattices"
    hd, hs = (dst.hi - dst.lo) / np.array(dst.reps), (src.hi - src.lo) / np.array(src.reps)
    cell, xis, stride = np.zeros((E, Q), int), np.zeros((E, Q, dst.dim)), 1
    e = np.arange(E)
    for d in range(dst.dim):
        ci = (e // int(np.prod(dst.reps[:d]))) % dst.reps[d]
        X = dst.lo[d] + hd[d] * (ci[:, None] + xi[None, :, d])
        t = (X - src.lo[d]) / hs[d]
        k = np.floor(t).astype(int)
        assert k.min() >= 0 and (t.max() <= src.reps[d]), "a point of dst lies outside src"
        k = np.minimum(k, src.reps[d] - 1)
        cell += stride * k
        xis[:, :, d] = t - k
        stride *= src.reps[d]
    return cell, xis


def source_values(dst, src, w_src, xi):
    """w^src[..., E, Q, dim] at the points (e, xi[q]) of dst's cells, for the src vectors w_src[..., n_src]"""
    w_src = np.asarray(w_src, float)
    cell, xis = locate(dst, src, xi)
    conn = np.array([c[0] for c in src.cells])
    out = np.zeros(w_src.shape[:-1] + cell.shape + (src.dim,))
    for e in range(len(dst.cells)):  # (cell by cell: the bases of a cell's points are the large array)
        N = shape_many(src.dim, src.p, xis[e])  # [Q, A]
        nodes = conn[cell[e]]  # [Q, A]
        for c in range(src.dim):
            out[..., e, :, c] = np.einsum("qa,...qa->...q", N, w_src[..., nodes * src.dim + c])
    return out


def load(dst, src, w_src, sub):
    """(b[..., n_dst], src_sq[...]) of the src vectors w_src[..., n_src]"""
    xi, w = composite_rule(dst.dim, dst.p, sub)
    N = shape_many(dst.dim, dst.p, xi)  # [Q, A]
    JxW = cell_jxw(dst, xi, w)
    val = source_values(dst, src, w_src, xi)  # [..., E, Q, dim]
    b = np.zeros(val.shape[:-3] + (dst.n,))
    for e, (conn, _, _) in enumerate(dst.cells):
        be = np.einsum("qa,...qc,q->...ac", N, val[..., e, :, :], JxW[e])
        for c in range(dst.dim):
            b[..., conn * dst.dim + c] += be[..., c]
    return b, np.einsum("...eqc,...eqc,eq->...", val, val, JxW)


def error_sq(dst, src, w_src, w_dst, sub):
    """int |w_src - w_dst|^2 on the composite rule over dst's cells"""
    xi, w = composite_rule(dst.dim, dst.p, sub)
    JxW = cell_jxw(dst, xi, w)
    d = source_values(dst, src, w_src, xi) - source_values(dst, dst, w_dst, xi)
    return np.einsum("...eqc,...eqc,eq->...", d, d, JxW)


class VectorMass:
    """the vector mass as an operator on whole dof vectors: M on every component, masked by `constrained` (or None)"""

    def __init__(self, M, dim, constrained=None):
        self.M, self.dim, self.constrained = M, dim, constrained

    def __matmul__(self, x):
        return mass_apply(self.M, x, self.dim, self.constrained)

    def diagonal(self):
        return np.repeat(np.diag(self.M), self.dim)


def jacobi_pcg(A, b, tol, max_it):
    """(x, iterations) of the Jacobi-preconditioned CG from x = 0, stopped at |r| <= tol |b| (the recurrence's residual).
    A: a matrix or a VectorMass; with constrained dofs b is taken as 0 there and they take no part"""
    mask = getattr(A, "constrained", None)
    dinv = 1.0 / A.diagonal()
    b = np.array(b, float)
    if mask is not None:
        dinv[mask], b[mask] = 0.0, 0.0
    x, r = np.zeros_like(b), b.copy()
    bb = np.sqrt(b @ b)
    if bb == 0.0:
        return x, 0
    z = dinv * r
    p, rz = z.copy(), r @ z
    for it in range(1, max_it + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        rz_new = r @ z
        if np.sqrt(r @ r) <= tol * bb:
            return x, it
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it


def kappa2(M, dim, constrained):
    """the largest kappa_2 of the free-free blocks"""
    k = 0.0
    for A in free_blocks(M, dim, constrained):
        ev = np.linalg.eigvalsh(A)
        k = max(k, ev[-1] / ev[0])
    return k
