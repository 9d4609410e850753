"""Independent numpy reference of the geometric multigrid V-cycle (dealii-adapter_amd/csrc/mi_mg.cpp), written from the
description at the top of that file and not from its kernels.

  hierarchy()        the shape of the hierarchy from (dim, degree, reps, mg_coarsest, mg_dense)
  interp_1d()        linear interpolation in lattice index space, s = t (n_s - 1) / (n_t - 1), in exact integer arithmetic
  Transfer           prolongation (fine constrained dofs zeroed), restriction (its transpose, coarse constrained dofs zeroed)
                     and the state transfer (fine -> coarse with the coarse mask), as Kronecker products applied axis by axis
  operator_matrix()  a mirror.Operator as a scipy CSR matrix, from the operator's own point data cell by cell (the operator
                     applied to every unit vector, which operator_matrix_by_unit_vectors() does literally on small meshes)
  Reference          the levels (all from mirror.py: Mi.Operator on the fine Mi.Mesh at u + du, Q1 Mi.Mesh boxes at the
                     interpolated state below), D = the dim x dim node diagonal blocks, and the V-cycle over a generic dtype

The smoother is the textbook Chebyshev iteration of the first kind for D^-1 A on [lmax / ratio, lmax] in its d-form
(Saad, Iterative Methods for Sparse Linear Systems, algorithm 12.1): one form only.  The cycle: nu steps from zero, residual,
restrict, recurse, prolongate and add, nu steps; nu = 3 on level 0 and 2 below; the last level is solved exactly (dense) or
by 12 steps over [lmax / 60, lmax].  lmax per level is an argument: the one scalar the reference takes from outside.

Precision: every product of the cycle runs in the dtype of the call (float64 or np.longdouble).  Level matrices are cast up
and multiplied with np.add.at; block inverses, the Cholesky factor of the coarsest level and the transfers are written in
plain array arithmetic, because LAPACK and scipy's sparse kernels exist in double only.

The fp32 opt-ins of the preconditioner (levels(), vcycle() and lambda_true() take them; the defaults are the fp64 cycle, bit
for bit what it was):
  storage=32 ("precond_storage" 32).  In the library every product of a cycle -- smoother steps, the cycle's residual, the
    eigenvalue estimates -- goes through level_spmv with smoother = true and reads the fp32-rounded copy of the level's values
    (d_sell_vals32) in fp64 arithmetic; D^-1 (extract_dinv_blk) and the coarsest level's dense inverse
    (launch_dense_inverse_from_sell) read the fp64 values.  So _Level.mult multiplies with astype(float32).astype(dtype) of the
    product matrix, and dinv / dense() keep the unrounded A.  product_matrices: one CSR per level to round instead of A --
    the device's own exports, so that both sides round the same bits (a value that differs in the last fp64 bit may round to
    the other fp32 neighbour).  lambda_true(l, storage=32) is the largest eigenvalue of D^-1 A_32.
  product0="f32" / "f32r" ("smoother_precision" 32).  Level 0 multiplies in an emulation of fp32 arithmetic, in two
    accumulation orders; no attempt at the kernel's own arithmetic: E32 below is a measured distance, not an equality.
"""
import numpy as np
import scipy.sparse as sp

import mirror as Mi

NU_FINE, NU_COARSE, RATIO = 3, 2, 20.0
COARSE_DEGREE, COARSE_RATIO = 12, 60.0
DENSE_MAX_DOFS = 384
# the reference's own rounding: worst relmax between the float64 and the long double cycle over CASES (random right-hand side),
# measured and asserted by tests/test_mirror_multigrid.py (8.98e-16).  The tolerance of the GPU tests rests on it.
E_REF = 1.0e-15


# ------------------------------------------------------------------ shape
def hierarchy(dim, degree, reps, coarsest=4, dense=1):
    """levels, finest first: dicts of degree, reps, n_dofs, exact (0/1), nu (smoother steps; polynomial degree on a coarsest
    level that is not solved exactly, 0 on one that is) and ratio (0 where exact)"""
    reps = [int(r) for r in reps[:dim]]
    shapes = [(degree, tuple(reps))]
    if degree > 1:
        shapes.append((1, tuple(reps)))  # p -> 1 on the same cells
    floor = min(2, coarsest)
    while max(reps) > coarsest:
        reps = [max(floor, -(-r // 2)) if r > floor else r for r in reps]
        shapes.append((1, tuple(reps)))
    out = []
    for l, (p, rp) in enumerate(shapes):
        n = dim * int(np.prod([p * r + 1 for r in rp]))
        last = l + 1 == len(shapes) and len(shapes) > 1
        exact = int(last and dense == 1 and n <= DENSE_MAX_DOFS)
        if exact:
            nu, ratio = 0, 0.0
        elif last:
            nu, ratio = COARSE_DEGREE, COARSE_RATIO
        else:
            nu, ratio = (NU_FINE if l == 0 else NU_COARSE), RATIO
        out.append(dict(degree=p, reps=rp, n_dofs=n, exact=exact, nu=nu, ratio=ratio))
    return out


# ------------------------------------------------------------------ transfers
def interp_1d(nt, ns, dtype=np.float64):
    """[nt, ns]: values on a lattice of nt points from one of ns points over the same interval, linear in the index"""
    P = np.zeros((nt, ns), dtype)
    if ns == 1:
        P[:, 0] = 1
        return P
    for t in range(nt):
        num, den = (t * (ns - 1), nt - 1) if nt > 1 else (0, 1)
        i = min(num // den, ns - 2)
        w = dtype(num - i * den) / dtype(den)
        P[t, i] += 1 - w
        P[t, i + 1] += w
    return P


def _apply_axes(mats, v, nn_src, dim):
    """(mats[dim-1] (x) ... (x) mats[0] (x) I_dim) v for a nodal vector v on the lattice nn_src (x fastest, dim components)"""
    a = v.reshape(tuple(nn_src[::-1]) + (dim,))
    for d in range(dim):
        ax = dim - 1 - d
        a = np.moveaxis(np.tensordot(mats[d], a, axes=([1], [ax])), 0, ax)
    return a.reshape(-1)


class Transfer:
    def __init__(self, dim, nn_fine, nn_coarse, fine_constrained, coarse_constrained, dtype=np.float64):
        self.dim, self.nf, self.nc = dim, list(nn_fine), list(nn_coarse)
        self.P = [interp_1d(self.nf[d], self.nc[d], dtype) for d in range(dim)]
        self.PT = [p.T.copy() for p in self.P]
        self.S = [interp_1d(self.nc[d], self.nf[d], dtype) for d in range(dim)]
        self.free_f, self.free_c = ~np.asarray(fine_constrained, bool), ~np.asarray(coarse_constrained, bool)

    def prolong(self, xc):
        return _apply_axes(self.P, xc, self.nc, self.dim) * self.free_f

    def restrict(self, rf):
        return _apply_axes(self.PT, rf * self.free_f, self.nf, self.dim) * self.free_c

    def state(self, uf):
        return _apply_axes(self.S, uf, self.nf, self.dim) * self.free_c


# ------------------------------------------------------------------ level operators
def operator_matrix(op):
    """The matrix of a mirror.Operator (scipy CSR, float64): its element tangents K_e from the operator's own point data
    (.g, .Jc, .tau, .N, .JxW, .mass), summed over the cells, rows and columns of constrained dofs replaced by .cdiag.
    K_e(ac, bd) = sum_q JxW [g_a . S(c, ., d, .) . g_b + delta_cd (g_a tau g_b + mass N_a N_b)] with S the minor-symmetrised
    Jc, which is Operator.__call__ on the unit vectors of a cell; the tests hold A x to op(x)."""
    m = op.m
    dim = m.dim
    Jc = op.Jc
    S = 0.25 * (Jc + np.swapaxes(Jc, -1, -2) + np.swapaxes(Jc, -3, -4) + np.swapaxes(np.swapaxes(Jc, -1, -2), -3, -4))
    h = np.einsum("eqaj,eqcjdl->eqacdl", op.g, S)
    Ke = np.einsum("eqacdl,eqbl,eq->eacbd", h, op.g, op.JxW, optimize=True)
    sc = np.einsum("eqaj,eqjk,eqbk,eq->eab", op.g, op.tau, op.g, op.JxW, optimize=True)
    sc += op.mass * np.einsum("qa,qb,eq->eab", op.N, op.N, op.JxW, optimize=True)
    for c in range(dim):
        Ke[:, :, c, :, c] += sc
    E, A = op.conn.shape
    dofs = (op.conn[:, :, None] * dim + np.arange(dim)).reshape(E, -1)
    rows = np.repeat(dofs, A * dim, axis=1).reshape(-1)
    cols = np.tile(dofs, (1, A * dim)).reshape(-1)
    vals = Ke.reshape(-1).copy()
    con = m.constrained
    vals[con[rows] | con[cols]] = 0.0
    cd = np.nonzero(con)[0]
    M = sp.coo_matrix((np.concatenate([vals, op.cdiag[cd]]), (np.concatenate([rows, cd]), np.concatenate([cols, cd]))),
                      shape=(m.n, m.n)).tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def operator_matrix_by_unit_vectors(op):
    """the same matrix, column by column (small meshes: the check of operator_matrix)"""
    n = op.m.n
    return sp.csr_matrix(np.stack([op(np.eye(n)[:, j]) for j in range(n)], -1))


def node_blocks(A, dim):
    """[n_nodes, dim, dim] diagonal blocks of a scipy matrix"""
    base = np.arange(A.shape[0] // dim) * dim
    return np.stack([np.stack([np.asarray(A[base + i, base + j]).ravel() for j in range(dim)], -1) for i in range(dim)], -2)


def invert_blocks(B):
    """inverses of [N, d, d] blocks (d = 2, 3) by the adjugate, in the dtype of B"""
    d = B.shape[-1]
    out = np.empty_like(B)
    if d == 2:
        det = B[:, 0, 0] * B[:, 1, 1] - B[:, 0, 1] * B[:, 1, 0]
        out[:, 0, 0], out[:, 1, 1] = B[:, 1, 1] / det, B[:, 0, 0] / det
        out[:, 0, 1], out[:, 1, 0] = -B[:, 0, 1] / det, -B[:, 1, 0] / det
        return out
    assert d == 3
    cof = np.empty_like(B)
    for i in range(3):
        for j in range(3):
            r, c = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            cof[:, i, j] = (-1) ** (i + j) * (B[:, r[0], c[0]] * B[:, r[1], c[1]] - B[:, r[0], c[1]] * B[:, r[1], c[0]])
    det = (B[:, 0, :] * cof[:, 0, :]).sum(-1)
    return np.swapaxes(cof, 1, 2) / det[:, None, None]


def spd_inverse(A):
    """inverse of a dense symmetric positive definite matrix through its Cholesky factor, in the dtype of A"""
    n = A.shape[0]
    L = np.tril(A).copy()
    for k in range(n):
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    Y = np.eye(n, dtype=A.dtype)
    for k in range(n):  # L Y = I
        Y[k] /= L[k, k]
        Y[k + 1:] -= np.outer(L[k + 1:, k], Y[k])
    for k in reversed(range(n)):  # L^T X = Y
        Y[k] /= L[k, k]
        Y[:k] -= np.outer(L[k, :k], Y[k])
    return Y


class _Level:
    """one level in one dtype: the matrix as COO arrays, D^-1 as node blocks.  product: the matrix that mult() multiplies
    with (None: A itself); storage 32: its values rounded to float32 and cast back, the arithmetic stays in dtype.  dense()
    -- what the coarsest level inverts -- is A at full precision whatever the product reads.  f32: None, or 0 / 1 = mult()
    emulates a product in fp32 arithmetic: values and operand cast to float32, accumulated in float32 with np.add.at in the
    stored order of the entries (0) or in the reverse of it (1), result cast back"""

    def __init__(self, A, Dinv, dim, dtype, product=None, storage=64, f32=None):
        coo = A.tocoo()
        self.n, self.dim = A.shape[0], dim
        self.rows, self.cols, self.vals = coo.row, coo.col, coo.data.astype(dtype)
        self.Dinv = Dinv.astype(dtype)
        self.dtype = dtype
        self.inverse = None
        self.f32 = f32
        if product is None and storage == 64:
            self.prows, self.pcols, self.pvals = self.rows, self.cols, self.vals
        else:
            assert storage in (64, 32)
            pc = coo if product is None else product.tocoo()
            assert pc.shape == A.shape
            data = pc.data.astype(np.float32).astype(dtype) if storage == 32 else pc.data.astype(dtype)
            self.prows, self.pcols, self.pvals = pc.row, pc.col, data
        if f32 is not None:
            order = slice(None) if f32 == 0 else slice(None, None, -1)
            self.prows, self.pcols = self.prows[order], self.pcols[order]
            self.pvals = self.pvals[order].astype(np.float32)

    def mult(self, x):
        if self.f32 is not None:
            y = np.zeros(self.n, np.float32)
            np.add.at(y, self.prows, self.pvals * x.astype(np.float32)[self.pcols])
            return y.astype(self.dtype)
        y = np.zeros(self.n, self.dtype)
        np.add.at(y, self.prows, self.pvals * x[self.pcols])
        return y

    def dinv(self, r):
        return (self.Dinv * r.reshape(-1, 1, self.dim)).sum(-1).reshape(-1)

    def dense(self):
        M = np.zeros((self.n, self.n), self.dtype)
        np.add.at(M, (self.rows, self.cols), self.vals)
        return M


def chebyshev(L, b, x, steps, lmax, ratio):
    """`steps` steps of the Chebyshev iteration for D^-1 A on [lmax / ratio, lmax] from x (None: zero), d-form"""
    dt = L.dtype
    beta = dt(lmax)
    alpha = beta / dt(ratio)
    theta, delta = (beta + alpha) / 2, (beta - alpha) / 2
    sigma = theta / delta
    rho = 1 / sigma
    if x is None:
        x, r = np.zeros(L.n, dt), b.copy()
    else:
        r = b - L.mult(x)
    d = L.dinv(r) / theta
    for k in range(steps):
        x = x + d
        if k + 1 == steps:
            break
        r = r - L.mult(d)
        rho_new = 1 / (2 * sigma - rho)
        d = rho_new * rho * d + (2 * rho_new / delta) * L.dinv(r)
        rho = rho_new
    return x


class Reference:
    """The hierarchy of one problem.  mesh: the fine Mi.Mesh; u_total: u + du; nq0 / fold0: the rule of the fine level's
    smoother product (None: the assembly's p + 2); the smoother's D always comes from the assembly rule, as in the library.
    coarse_from: None, or the fine u + du that the levels >= 1 are interpolated from instead of u_total (coarse operators
    that lag behind the fine tangent)."""

    def __init__(self, mesh, u_total, coarsest=4, dense=1, nq0=None, fold0=False, coarse_from=None, fine=None, **material):
        m = mesh
        dim = self.dim = m.dim
        self.shape = hierarchy(dim, m.p, m.reps, coarsest, dense)
        self.meshes, self.states, self.A, self.D = [m], [np.asarray(u_total, float)], [], []
        if fine is not None:  # another Reference of the same mesh, state and rule: its fine level is this one's
            A0, A_asm, D0 = fine.A[0], fine.A_assembled, fine.D[0]
        else:
            op_asm = Mi.Operator(m, u_total, **material)
            A_asm = operator_matrix(op_asm)
            if nq0 is None or (nq0 == m.p + 2 and not fold0):
                A0 = A_asm
            else:
                A0 = operator_matrix(Mi.Operator(m, u_total, nq=nq0, fold_to_identity=fold0, cdiag=op_asm.cdiag, **material))
            D0 = node_blocks(A_asm, dim)
        self.A.append(A0)
        self.D.append(D0)
        self.A_assembled = A_asm
        self.T = []
        src = np.asarray(u_total if coarse_from is None else coarse_from, float)
        for lv in self.shape[1:]:
            mc = Mi.Mesh(dim, 1, lv["reps"], m.lo, m.hi, m.roles)
            mf = self.meshes[-1]
            t = Transfer(dim, mf.nn, mc.nn, mf.constrained, mc.constrained)
            uc = t.state(src)
            src = uc
            Ac = operator_matrix(Mi.Operator(mc, uc, **material))
            self.meshes.append(mc)
            self.states.append(uc)
            self.T.append(t)
            self.A.append(Ac)
            self.D.append(node_blocks(Ac, dim))
        self._cache = {}

    def lambda_true(self, l, storage=64, product_matrices=None):
        """largest eigenvalue of D^-1 A on level l; storage 32: of D^-1 A_32, A_32 = the product matrix of the level
        (product_matrices[l], or A) with fp32-rounded values, D from the unrounded A as ever"""
        import scipy.sparse.linalg as spla
        A, D, dim = self.A[l], self.D[l], self.dim
        if product_matrices is not None:
            A = product_matrices[l].tocsr()
        if storage == 32:
            A = sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices, A.indptr), shape=A.shape)
        w, V = np.linalg.eigh(D)  # D^-1/2 by blocks
        Dmh = np.einsum("nij,nj,nkj->nik", V, 1 / np.sqrt(w), V)
        S = sp.bsr_matrix((Dmh, np.arange(len(Dmh)), np.arange(len(Dmh) + 1)), shape=A.shape).tocsr()
        B = (S @ A @ S)
        B = 0.5 * (B + B.T)
        if A.shape[0] <= 1500:
            return float(np.linalg.eigvalsh(B.toarray())[-1])
        v0 = np.random.default_rng(0).standard_normal(A.shape[0])  # (a seeded start vector: the same digits in every run)
        return float(spla.eigsh(B, k=1, which="LA", tol=1e-12, v0=v0, return_eigenvectors=False)[0])

    def levels(self, dtype, storage=64, product_matrices=None, product0=None):
        """(levels, transfers) in one dtype.  storage 32: every product of the cycle multiplies with fp32-rounded values;
        product_matrices: one CSR matrix per level that the products read in place of A (D^-1 and the dense inverse keep
        coming from A); product0 "f32" / "f32r": level 0 multiplies in the fp32 emulation, stored / reverse order"""
        if dtype in self._cache and storage == 64 and product_matrices is None and product0 is None:
            return self._cache[dtype][:2]
        key = (dtype, storage, None if product_matrices is None else tuple(id(P) for P in product_matrices), product0)
        if key not in self._cache:
            base = self._cache.get(dtype)
            f32 = {None: None, "f32": 0, "f32r": 1}[product0]
            Ls = []
            for l, (A, D) in enumerate(zip(self.A, self.D)):
                Dinv = base[0][l].Dinv if base else invert_blocks(D.astype(dtype))
                P = None if product_matrices is None else product_matrices[l]
                Ls.append(_Level(A, Dinv, self.dim, dtype, P, storage, f32 if l == 0 else None))
            if self.shape[-1]["exact"]:
                Ls[-1].inverse = base[0][-1].inverse if base else spd_inverse(Ls[-1].dense())
            Ts = base[1] if base else [Transfer(self.dim, t.nf, t.nc, ~t.free_f, ~t.free_c, dtype) for t in self.T]
            # (the entry keeps product_matrices alive: an id in the key is never that of another list's matrix)
            self._cache[key] = (Ls, Ts, product_matrices)
            if key == (dtype, 64, None, None):
                self._cache[dtype] = self._cache[key]
        return self._cache[key][:2]

    def vcycle(self, r, lmax, dtype=np.float64, nu=None, l=0, storage=64, product_matrices=None, product0=None):
        """B r: one V-cycle on the right-hand side r; lmax[l] per smoothed level (ignored on an exact one);
        nu: override of the smoother steps of every level but an inexact coarsest one (tests of the reference itself);
        storage, product_matrices, product0: as for levels()"""
        Ls, Ts = self.levels(dtype, storage, product_matrices, product0)
        L, sh = Ls[l], self.shape[l]
        b = np.asarray(r).astype(dtype)
        if l + 1 == len(Ls) and len(Ls) > 1:
            if sh["exact"]:
                return L.inverse @ b
            return chebyshev(L, b, None, sh["nu"], lmax[l], sh["ratio"])
        k = sh["nu"] if nu is None else nu
        x = chebyshev(L, b, None, k, lmax[l], sh["ratio"])
        res = b - L.mult(x)
        xc = self.vcycle(Ts[l].restrict(res), lmax, dtype, nu, l + 1, storage, product_matrices, product0)
        x = x + Ts[l].prolong(xc)
        return chebyshev(L, b, x, k, lmax[l], sh["ratio"])

    def true_lmax(self, safety=1.15):
        return [0.0 if sh["exact"] else safety * self.lambda_true(l) for l, sh in enumerate(self.shape)]


# ------------------------------------------------------------------ the cases of tests/test_gpu_multigrid_reference.py
# (here, so that tests/test_mirror_multigrid.py measures the reference's own rounding on the same inputs without a GPU)
CL, IF, ZC = Mi.CLAMPED, Mi.INTERFACE, Mi.ZCLAMP
ROLES_A = [CL, IF, IF, IF, ZC, IF]
ROLES_B = [CL, IF, IF, IF, ZC, ZC]
ROLES_2D = [CL, IF, IF, IF, 0, 0]
A1 = 1.0 / (0.25 * 0.005**2)  # alpha_1 of the default Newmark parameters

# keys: tuning keys set before "precond" 1.  nq0 / fold0: the rule of the fine level's smoother product (None: the assembled
# matrix), which the GPU test also reads back from the library.  coarsest / dense: what the keys make of the defaults 4 / 1.
CASES = {
    "q2_654": dict(dim=3, p=2, reps=(6, 5, 4), kind="cube", roles=ROLES_A),
    "q2_753_mf27": dict(dim=3, p=2, reps=(7, 5, 3), kind="distorted", roles=ROLES_B, keys=[("element_tangents", 2)], nq0=3,
                        fold0=True),
    "q2_543_mf_fine": dict(dim=3, p=2, reps=(5, 4, 3), kind="graded", roles=ROLES_A, keys=[("fine_level", 1)], nq0=3,
                           fold0=True),
    "q3_532_rule5": dict(dim=3, p=3, reps=(5, 3, 2), kind="cube", roles=ROLES_A,
                         keys=[("fine_level", 1), ("smoother_quadrature_q3", 5)], nq0=5),
    "q3_532_rule4": dict(dim=3, p=3, reps=(5, 3, 2), kind="cube", roles=ROLES_A,
                         keys=[("fine_level", 1), ("smoother_quadrature_q3", 4)], nq0=4, fold0=True),
    "q1_987": dict(dim=3, p=1, reps=(9, 8, 7), kind="cube", roles=ROLES_B),
    "q2_444_coarsest2": dict(dim=3, p=2, reps=(4, 4, 4), kind="cube", roles=ROLES_A, keys=[("mg_coarsest", 2)], coarsest=2),
    "q2_888": dict(dim=3, p=2, reps=(8, 8, 8), kind="cube", roles=ROLES_A),
    "q2_444_polynomial": dict(dim=3, p=2, reps=(4, 4, 4), kind="cube", roles=ROLES_B,
                              keys=[("mg_dense", 0), ("mg_coarsest", 1)], coarsest=1, dense=0),
    "q2_1231": dict(dim=3, p=2, reps=(12, 3, 1), kind="cube", roles=ROLES_A),
    "2d_q2_186": dict(dim=2, p=2, reps=(18, 6), kind="cube", roles=ROLES_2D),
    "2d_q4_64": dict(dim=2, p=4, reps=(6, 4), kind="cube", roles=ROLES_2D),
    "q2_4412_3slabs_z": dict(dim=3, p=2, reps=(4, 4, 12), kind="cube", roles=ROLES_A, slabs=3, cut_axis=3),
    "q2_1244_2slabs_x": dict(dim=3, p=2, reps=(12, 4, 4), kind="cube", roles=ROLES_B, slabs=2, cut_axis=1),
    "q2_4416_induced": dict(dim=3, p=2, reps=(4, 4, 16), kind="cube", roles=ROLES_A, slabs=2, cut_axis=3,
                            keys=[("mg_dist_nodes", 0)]),
}
# Mid-size cases, a table of their own (CASES and what was measured on it stay what they are): the smallest meshes of their
# kind with more than 10,240 nodes, i.e. more than 160 slices of 64 rows, above which a product of level 0 leaves
# sell_spmv_split for sell_spmv (tests/test_gpu_sell_lds_product.py); vertices moved by 5 % of the cell size.
# e_ref of these cases, float64 against long double cycle as for E_REF (tests/test_mirror_multigrid.py): q1_3d 6.22e-16,
# q2_11 9.04e-16, 2d_q4 8.16e-16 -- within E_REF, so the tolerance of the GPU tests is the one of CASES.
MID_CASES = {
    "q1_3d": dict(dim=3, p=1, reps=(22, 21, 21), kind="perturbed", roles=ROLES_A),
    "q2_11": dict(dim=3, p=2, reps=(11, 11, 11), kind="perturbed", roles=ROLES_A),
    "2d_q4": dict(dim=2, p=4, reps=(26, 25), kind="perturbed", roles=ROLES_2D),
}
# The fp32 opt-ins of the preconditioner (tests/test_gpu_multigrid_fp32.py), a table of their own again.  One new mesh: 3D Q3
# with the fine level assembled.  Both opt-ins make the fine level's smoother multiply with the assembly-rule operator, so
# every reference of these tests is built by assembled_reference(), whatever rule the case's own keys select under fp64.
FP32_CASES = {
    "q3_532_assembled": dict(dim=3, p=3, reps=(5, 3, 2), kind="cube", roles=ROLES_A),
}
# "precond_storage" 32: fp64 arithmetic on fp32-rounded values (modelled exactly: Reference.vcycle(storage=32)).  Its own
# rounding, float64 against long double cycle as for E_REF, lies within E_REF on every case (measured worst 8.9e-16 on
# q2_4412_3slabs_z, tests/test_mirror_multigrid.py), so the GPU tolerance is the one of the fp64 tests.
STORAGE_CASES = ["q2_654", "q1_987", "2d_q4_64", "q3_532_assembled", "q2_753_mf27", "q2_4412_3slabs_z", "q2_11"]
# "smoother_precision" 32: fp32 arithmetic on fp32 point records, on level 0 only.  Not reproducible in numpy; E32 is the
# worst relmax between the fp64 reference cycle and the cycle whose level-0 products run in the fp32 emulation of
# _Level.mult, over these cases, three right-hand sides and both accumulation orders, measured and asserted by
# tests/test_mirror_multigrid.py.  TOL32 = 16 x E32 rounded up to a power of ten, never above 1e-4: the kernel
# rounds point records and sums in a sum-factorised order, the emulation rounds matrix entries and sums in row order.
PRECISION_CASES = ["q2_543_mf_fine", "q2_654", "q2_4412_3slabs_z"]
E32 = 6.0e-7  # measured 5.74e-7 (q2_654, unit vector, reverse order), rounded up in the second digit; TOL32 = 1e-5


def tol32():
    import math
    return min(1e-4, 10.0 ** math.ceil(math.log10(16 * E32)))


def geometry(kind, dim, reps, seed):
    """lo, hi, perturb of a cube / graded / distorted mesh of reps cells"""
    reps = np.array(reps[:dim])
    lo = (0.0,) * dim
    if kind == "cube":
        return lo, tuple(0.1 * reps), None
    if kind == "perturbed":  # cells of 0.1, every vertex moved by 5 % of that (standard deviation)
        nverts = int(np.prod(reps + 1))
        return lo, tuple(0.1 * reps), 0.05 * 0.1 * np.random.default_rng(seed).standard_normal((nverts, dim))
    h = np.array([0.13, 0.1, 0.07])[:dim]
    hi = tuple(h * reps)
    rng = np.random.default_rng(seed)
    nv = reps + 1
    vid = np.stack(np.unravel_index(np.arange(int(np.prod(nv))), tuple(nv[::-1])), -1)[:, ::-1]  # vertices, x fastest
    if kind == "graded":  # rectilinear: every vertex plane moved along its own axis
        planes = [0.3 * h[d] * rng.uniform(-1, 1, nv[d]) for d in range(dim)]
        return lo, hi, np.stack([planes[d][vid[:, d]] for d in range(dim)], -1)
    assert kind == "distorted"
    return lo, hi, 0.08 * h.min() * rng.standard_normal((len(vid), dim))


def case(name):
    return CASES[name] if name in CASES else MID_CASES[name] if name in MID_CASES else FP32_CASES[name]


def case_mesh(name):
    c = case(name)
    lo, hi, perturb = geometry(c["kind"], c["dim"], c["reps"], seed=sum(c["reps"]))
    return Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, c["roles"], perturb=perturb), lo, hi, perturb


def shear(X):
    """a smooth deformation with shear (F != F^T, J != 1) that vanishes on x = min x and, in 3D, has u_z = 0 on both z faces"""
    dim = X.shape[1]
    L = np.ptp(X, axis=0).max()
    s = (X - X.min(axis=0)) / L
    u = np.zeros_like(X)
    z = s[:, 2] if dim == 3 else 0.5 * s[:, 1]
    u[:, 0] = s[:, 0] * (0.3 * s[:, 1] + 0.2 * z)
    u[:, 1] = s[:, 0] * (0.25 + 0.3 * z**2)
    if dim == 3:
        tz = np.ptp(z)
        u[:, 2] = s[:, 0] * z * (tz - z) * (0.6 * np.sin(3.0 * s[:, 1]) - 0.5)
    return L * u.reshape(-1)


def case_state(m, seed, amplitude=0.25):
    """u, du: V_U and V_DELTA both non-zero on the free dofs -- a smooth shear plus small noise -- and V_U small and non-zero
    on the constrained ones.  (At twice this amplitude the
    tangent of the 8 x 8 x 8 cube is indefinite, smallest eigenvalue -865 against 1.5e6: no case for a CG.)"""
    rng = np.random.default_rng(seed)
    free = ~m.constrained
    h = ((m.hi - m.lo) / np.array(m.reps)).min() / m.p
    s = amplitude * shear(m.coords) * free
    noise = 2e-3 * h * rng.standard_normal(m.n) * free
    # V_U also carries values on the constrained dofs: the fine tangent reads them as they are, the state transfer masks them
    # on every coarser level, and only with them does a transfer that forgets the mask compute something else
    held = 2e-3 * h * rng.standard_normal(m.n) * ~free
    return 0.6 * s + noise + held, 0.4 * s - 0.5 * noise


def case_reference(name, u_total, m, **kw):
    c = case(name)
    args = dict(coarsest=c.get("coarsest", 4), dense=c.get("dense", 1), nq0=c.get("nq0"), fold0=c.get("fold0", False), alpha1=A1)
    args.update(kw)
    return Reference(m, u_total, **args)


def assembled_reference(name, u_total, m, **kw):
    """the reference of a case with the assembly-rule operator on the fine level, whatever its keys select: what both fp32
    opt-ins of the preconditioner multiply with"""
    return case_reference(name, u_total, m, nq0=None, fold0=False, **kw)


def second_increment(m, du):
    """V_DELTA of the second tangent in the tests that re-assemble at a changed state (the one of the lagged-operators test)"""
    return 0.55 * du + 1e-5 * np.random.default_rng(2).standard_normal(m.n) * ~m.constrained


def cpu_rhs_set(m, seed=5):
    """three right-hand sides without a device: white noise, a smooth field, a unit vector next to the clamped face"""
    free = ~m.constrained
    node = 1
    for d in range(1, m.dim):
        node += int(np.prod(m.nn[:d]))
    e = np.zeros(m.n)
    e[node * m.dim] = 1.0
    return [("random", np.random.default_rng(seed).standard_normal(m.n) * free), ("smooth", shear(m.coords) * free), ("unit", e)]
