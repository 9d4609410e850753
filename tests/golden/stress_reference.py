"""Numpy reference of the nodal stress recovery (mi_stress_field), from mirror.py's pieces alone.

  W_i       = sum_cells sum_q N_i(q) JxW(q)                         lumped weight
  sigma_i   = ( sum_cells sum_q N_i(q) sigma(q) JxW(q) ) / W_i       lumped L2 projection, reference configuration

  model 0   sigma(q) = tau(F)/det F with tau of mirror.material at F = I + grad u, on QGauss(p + 2) (qf_cell,
            nonlinear_elasticity.cc:74; compressible_neo_hook_material.h:62-138)
  model 1   sigma(q) = lambda tr(eps) I + 2 mu eps, eps = sym grad u, lambda = 2 mu nu / (1 - 2 nu) (parameters.cc:189), on
            QGauss(p + 1) (linear_elasticity.cc:61)

Components: xx, yy, zz, xy, xz, yz in 3D and xx, yy, xy in 2D.  Von Mises from the projected nodal tensor: 3D
sqrt(3/2 s : s) with s = sigma - tr(sigma)/3 I, 2D the in-plane form sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2).

Nothing here comes from the device code: points, weights, shape functions and the d-linear map are mirror.py's, the material
is mirror.material.  dtype: the sums can be carried in np.longdouble (the conditioning check of test_mirror_stress.py).
"""
import numpy as np

from mirror import feq_nodes, gauss01, material, q1_jacobian, shape_at

NEOHOOKE, LINEAR = 0, 1
PAIRS = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]}


def point_stress(dim, mu, nu, H, model):
    """sigma(q) [dim, dim] and det F (model 1: 1.0) from the displacement gradient H = grad u"""
    if model == NEOHOOKE:
        F = np.eye(dim) + H
        J = np.linalg.det(F)
        return material(dim, mu, nu, F)[0] / J, J
    lam = 2 * mu * nu / (1 - 2 * nu)
    eps = 0.5 * (H + H.T)
    return lam * np.trace(eps) * np.eye(dim) + 2 * mu * eps, 1.0


def _rule(dim, p, nq):
    nodes = feq_nodes(p)
    qx, qw = gauss01(nq)
    rule = []
    for q in np.ndindex(*([nq] * dim)):
        qi = q[::-1]  # x fastest
        xi = np.array([qx[k] for k in qi])
        N, dN = shape_at(dim, p, nodes, xi)
        rule.append((xi, np.prod([qw[k] for k in qi]), N, dN))
    return rule


def _points(mesh, u, mu, nu, model):
    """(conn, N, sigma(q) as ncomp numbers, JxW, det F) of every point of every cell"""
    dim, p = mesh.dim, mesh.p
    rule = _rule(dim, p, p + 2 if model == NEOHOOKE else p + 1)
    U = np.asarray(u, float).reshape(-1, dim)
    for conn, verts, _ in mesh.cells:
        Ue = U[conn]
        for xi, w, N, dN in rule:
            Jm = q1_jacobian(dim, verts, xi)
            H = Ue.T @ (dN @ np.linalg.inv(Jm))
            s, det = point_stress(dim, mu, nu, H, model)
            yield conn, N, np.array([s[d, e] for d, e in PAIRS[dim]]), np.linalg.det(Jm) * w, det


def von_mises(dim, sigma):
    s = np.asarray(sigma)
    if dim == 2:
        return np.sqrt(s[:, 0] ** 2 - s[:, 0] * s[:, 1] + s[:, 1] ** 2 + 3 * s[:, 2] ** 2)
    m = (s[:, 0] + s[:, 1] + s[:, 2]) / 3
    dev = s[:, :3] - m[:, None]
    return np.sqrt(1.5 * ((dev ** 2).sum(axis=1) + 2 * (s[:, 3:] ** 2).sum(axis=1)))


def points(mesh, u, mu, nu, model):
    """the point values as a list, to sum them more than once (nodal_stress(..., pts=...))"""
    return list(_points(mesh, u, mu, nu, model))


def nodal_stress(mesh, u, mu, nu, model, dtype=np.float64, pts=None):
    """(sigma[nnodes, ncomp], von_mises[nnodes], W[nnodes], smallest det F) of the state u on a mirror.Mesh"""
    ncomp = len(PAIRS[mesh.dim])
    acc, W = np.zeros((mesh.nnodes, ncomp), dtype), np.zeros(mesh.nnodes, dtype)
    min_det = np.inf
    for conn, N, s, JxW, det in (_points(mesh, u, mu, nu, model) if pts is None else pts):
        min_det = min(min_det, det)
        Nw = N.astype(dtype) * dtype(JxW)
        W[conn] += Nw
        acc[conn] += Nw[:, None] * s.astype(dtype)[None, :]
    sigma = acc / W[:, None]
    return sigma, von_mises(mesh.dim, sigma), W, min_det


def mean_stress(mesh, u, mu, nu, model):
    """sum over cells and points of sigma(q) JxW, ncomp numbers"""
    tot = np.zeros(len(PAIRS[mesh.dim]))
    for _, _, s, JxW, _ in _points(mesh, u, mu, nu, model):
        tot += s * JxW
    return tot
