"""Numpy reference of the energy diagnostics (mi_energy, mi_linear_energy), from mirror.py's pieces alone.

  psi()       get_Psi = Psi_vol(J) + Psi_iso(b_bar), compressible_neo_hook_material.h:30-35, 62-72:
              kappa/4 (J^2 - 1 - 2 ln J) + c_1 (tr b_bar - dim),  c_1 = mu/2,  b_bar = J^(-2/dim) F F^T
  energies()  strain  = sum over cells and points of Psi(F(u)) JxW on QGauss(p + 2) (qf_cell, nonlinear_elasticity.cc:74)
              kinetic = 1/2 rho sum |v_h|^2 JxW,  body = -rho sum b . u_h JxW  on the same rule
              and the smallest det F over all points
  linear_energies()  1/2 d^T K d, 1/2 v^T M v, -d . body_vec with the matrices of mirror.Linear

Nothing here comes from the device code: points, weights, shape functions and the d-linear map are mirror.py's, the
stored-energy function is written out from the reference's formulas.
"""
import numpy as np

from mirror import feq_nodes, gauss01, q1_jacobian, shape_at


def psi(dim, mu, nu, F):
    kappa = 2 * mu * (1 + nu) / (3 * (1 - 2 * nu))  # compressible_neo_hook_material.h:20
    J = np.linalg.det(F)
    b_bar = J ** (-2.0 / dim) * F @ F.T
    return kappa / 4 * (J * J - 1 - 2 * np.log(J)) + mu / 2 * (np.trace(b_bar) - dim)


def energies(mesh, u, v, mu=0.5e6, nu=0.4, rho=1000.0, body=(0, 0, 0), nq=None):
    """(strain, kinetic, body, min det F) of the state u, v (vectors of mesh.n dofs) on a mirror.Mesh"""
    dim, p = mesh.dim, mesh.p
    nq = p + 2 if nq is None else nq
    nodes = feq_nodes(p)
    qx, qw = gauss01(nq)
    rule = []
    for q in np.ndindex(*([nq] * dim)):
        qi = q[::-1]  # x fastest
        xi = np.array([qx[k] for k in qi])
        N, dN = shape_at(dim, p, nodes, xi)
        rule.append((xi, np.prod([qw[k] for k in qi]), N, dN))
    b = np.asarray(body, float)[:dim]
    U, V = np.asarray(u, float).reshape(-1, dim), np.asarray(v, float).reshape(-1, dim)
    strain = kinetic = pot = 0.0
    min_det = np.inf
    for conn, verts, _ in mesh.cells:
        Ue, Ve = U[conn], V[conn]
        for xi, w, N, dN in rule:
            Jm = q1_jacobian(dim, verts, xi)
            JxW = np.linalg.det(Jm) * w
            F = np.eye(dim) + Ue.T @ (dN @ np.linalg.inv(Jm))
            det = np.linalg.det(F)
            min_det = min(min_det, det)
            if det > 0:
                strain += psi(dim, mu, nu, F) * JxW
            vq, uq = Ve.T @ N, Ue.T @ N
            kinetic += 0.5 * rho * (vq @ vq) * JxW
            pot -= rho * (b @ uq) * JxW
    return strain, kinetic, pot, min_det


def volume(mesh):
    """sum of JxW on the assembly's rule"""
    dim, p = mesh.dim, mesh.p
    qx, qw = gauss01(p + 2)
    vol = 0.0
    for _, verts, _ in mesh.cells:
        for q in np.ndindex(*([p + 2] * dim)):
            xi = np.array([qx[k] for k in q[::-1]])
            vol += np.linalg.det(q1_jacobian(dim, verts, xi)) * np.prod([qw[k] for k in q])
    return vol


def linear_strain_pointwise(mesh, d, mu, nu):
    """int (lambda/2 tr(eps)^2 + mu eps : eps) on the linear model's rule QGauss(p + 1) (linear_elasticity.cc:61): the
    quadratic form of the K of :301-320, point by point instead of through the matrix"""
    dim, p = mesh.dim, mesh.p
    lam = 2 * mu * nu / (1 - 2 * nu)  # parameters.cc:189
    nodes = feq_nodes(p)
    qx, qw = gauss01(p + 1)
    D = np.asarray(d, float).reshape(-1, dim)
    W = 0.0
    for conn, verts, _ in mesh.cells:
        for q in np.ndindex(*([p + 1] * dim)):
            xi = np.array([qx[k] for k in q[::-1]])
            _, dN = shape_at(dim, p, nodes, xi)
            Jm = q1_jacobian(dim, verts, xi)
            H = D[conn].T @ (dN @ np.linalg.inv(Jm))
            eps = 0.5 * (H + H.T)
            W += (0.5 * lam * np.trace(eps) ** 2 + mu * np.sum(eps * eps)) * np.linalg.det(Jm) * np.prod([qw[k] for k in q])
    return W


def linear_energies(lin, d, v):
    """(strain, kinetic, body) of the linear model: mirror.Linear's K, M and body vector"""
    d, v = np.asarray(d, float), np.asarray(v, float)
    return 0.5 * d @ (lin.K @ d), 0.5 * v @ (lin.M @ v), -(d @ lin.body_vec)
