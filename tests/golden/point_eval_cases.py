"""Meshes, fields and point sets shared by test_mirror_point_eval.py, test_gpu_point_eval.py and test_gpu_state_transfer.py.

Meshes: anisotropic boxes with distinct edge lengths (0.1, 0.13, 0.07 per cell), plain or with the vertices moved by
0.05 hmin randn (the recipe of test_gpu_linear_matrix_free.py; hmin the shortest edge, so the offsets stay far below a quarter
of it).  Fields with known answers: Poly, a polynomial of degree <= p in every direction with random coefficients (an FE_Q(p)
function on a box mesh: reproduced exactly, values and gradients), and its degree-1 total form, the affine field A X + b
(reproduced on every mesh, since the Q1 map reproduces X itself).
"""
import numpy as np

import mirror as Mi

EDGE = (0.1, 0.13, 0.07)
ROLES = [1, 7, 0, 7, 8, 0]  # x- clamped, x+ / y+ interface, z- clamped in z (3D)
_meshes = {}


def make_mesh(dim, p, reps, perturbed, roles=None, lo=None, refine=1):
    """dict(dim, p, reps, lo, hi, perturb, roles, mesh) -- built once per key and left unchanged.  refine = k: the same box in
    k x reps cells (nested in the cells of refine = 1)"""
    reps = tuple(reps)
    roles = list(ROLES[:2 * dim] if roles is None else roles)
    lo = (0.0,) * dim if lo is None else tuple(lo)
    key = (dim, p, reps, perturbed, tuple(roles), lo, refine)
    if key not in _meshes:
        hi = tuple(lo[d] + EDGE[d] * reps[d] for d in range(dim))
        reps = tuple(refine * r for r in reps)
        nv = int(np.prod([r + 1 for r in reps]))
        rng = np.random.default_rng(1000 * dim + sum(reps))  # (not the degree: meshes of one shape share their cells)
        perturb = 0.05 * min(EDGE[:dim]) / refine * rng.standard_normal((nv, dim)) if perturbed else None
        assert perturb is None or np.linalg.norm(perturb, axis=1).max() < 0.25 * min(EDGE[:dim]) / refine
        _meshes[key] = dict(dim=dim, p=p, reps=reps, lo=lo, hi=hi, perturb=perturb, roles=roles,
                            mesh=Mi.Mesh(dim, p, reps, lo, hi, roles, perturb=perturb))
    return _meshes[key]


def context(M, c, **kw):
    fr = list(c["roles"]) + [0] * (6 - len(c["roles"]))
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=c["lo"], hi=c["hi"], face_role=fr, perturb=c["perturb"], **kw)
    assert G.n == c["mesh"].n and np.array_equal(G.constrained, c["mesh"].constrained)
    return G


class Poly:
    """u_c(X) = sum_k coef[c, k] prod_d (X_d / scale_d)^(k_d), 0 <= k_d <= p"""

    def __init__(self, dim, p, scale, rng):
        self.dim, self.p, self.scale = dim, p, np.asarray(scale, float)[:dim]
        self.coef = rng.uniform(-1, 1, (dim,) + (p + 1,) * dim)
        self.sub = {2: "cij,ni,nj->nc", 3: "cijk,ni,nj,nk->nc"}[dim]

    def _powers(self, X, deriv):
        k = np.arange(self.p + 1)
        out = []
        for d in range(self.dim):
            s = X[:, d, None] / self.scale[d]
            if d == deriv:
                out.append(k * s ** np.maximum(k - 1, 0) / self.scale[d])
            else:
                out.append(s ** k)
        return out

    def __call__(self, X):
        return np.einsum(self.sub, self.coef, *self._powers(np.asarray(X, float), -1))

    def grad(self, X):
        X = np.asarray(X, float)
        return np.stack([np.einsum(self.sub, self.coef, *self._powers(X, d)) for d in range(self.dim)], axis=2)  # [n, c, d]


class Affine:
    def __init__(self, dim, rng):
        self.A, self.b = rng.uniform(-1, 1, (dim, dim)), rng.uniform(-1, 1, dim)

    def __call__(self, X):
        return np.asarray(X, float) @ self.A.T + self.b

    def grad(self, X):
        return np.broadcast_to(self.A, (len(X),) + self.A.shape)


def interior_pairs(mesh, n, rng):
    """n random (cell, xi) pairs with xi in [0.05, 0.95]^dim"""
    return rng.integers(0, len(mesh.cells), n), rng.uniform(0.05, 0.95, (n, mesh.dim))


def boundary_pairs(mesh):
    """(cell, xi) pairs on every face, edge and corner of every cell (xi in {0, 0.37, 1}^dim, not all inner): the cells' shared
    faces, edges and corners and the domain's own corners among them"""
    cells, xi = [], []
    for c in range(len(mesh.cells)):
        for t in np.ndindex(*([3] * mesh.dim)):
            if any(k != 1 for k in t):
                cells.append(c)
                xi.append([(0.0, 0.37, 1.0)[k] for k in t])
    return np.array(cells), np.array(xi)


def containing_cells(mesh, cell, xi):
    """lexicographic ids of the cells that contain the point (cell, xi), xi on the cell's boundary where components are 0 or 1"""
    ci, c = [], cell
    for d in range(mesh.dim):
        ci.append(c % mesh.reps[d])
        c //= mesh.reps[d]
    options = []
    for d in range(mesh.dim):
        o = [ci[d]]
        if xi[d] == 0.0 and ci[d] > 0:
            o.append(ci[d] - 1)
        if xi[d] == 1.0 and ci[d] < mesh.reps[d] - 1:
            o.append(ci[d] + 1)
        options.append(o)
    out = set()
    for t in np.ndindex(*[len(o) for o in options]):
        cid, stride = 0, 1
        for d in range(mesh.dim):
            cid += stride * options[d][t[d]]
            stride *= mesh.reps[d]
        out.add(cid)
    return out
