"""Numpy reference of the nodal forces, support reactions and load resultants (mi_reactions), from mirror.py's pieces alone.

All nodal, UNMASKED (every dof, constrained ones too), node and dof order of mirror.Mesh:

  model 0   internal_i = sum_cells sum_q tau(F) F^-T grad_X N_i JxW   on QGauss(p + 2), F = I + grad u, tau of mirror.material_batch
            inertia_i  = rho sum N_i a_h JxW                          on the same rule
            body_i     = rho b W_i,  W_i = sum N_i JxW
            load_i     = mirror.neumann_cell of the interface faces at the displacement u (the pull-back at the cell point whose
                         index is the face-point counter)
  model 1   internal   = K d as the integral of (lambda tr eps I + 2 mu eps) grad N on QGauss(p + 1); inertia as above with the
            acceleration the caller hands over; load: the vector the caller hands over; body = 0

  forces = internal + inertia - body - load;  reaction: forces on the constrained dofs;  unbalanced: on the free dofs
  resultant of f over a dof set: sum f_i;  moment about x0: sum (x_i - x0) x f_i, x_i = X_i + u_i (model 0) or X_i (model 1)

Vectorised over cells and points; no element matrix is formed.  Nothing here comes from the device code.
"""
import numpy as np

import mirror as Mi

NEOHOOKE, LINEAR = 0, 1
SETS = ("reaction", "unbalanced", "inertia", "body", "load")


def cell_terms(mesh, model, u, acc, mu, nu, rho):
    """(internal[n], inertia[n], W[nnodes], smallest det F) of the cells"""
    dim, p = mesh.dim, mesh.p
    conn = np.array([c for c, _, _ in mesh.cells])
    verts = np.array([v for _, v, _ in mesh.cells])
    xi, w, N, dN = Mi._rule(dim, p, p + 2 if model == NEOHOOKE else p + 1)
    Jm = Mi._q1_jacobians(dim, verts, xi)
    G = np.einsum("qak,eqkj->eqaj", dN, np.linalg.inv(Jm))  # reference-configuration gradients [E, Q, A, dim]
    JxW = np.linalg.det(Jm) * w
    U = np.asarray(u, float).reshape(-1, dim)[conn]
    H = np.einsum("eai,eqaj->eqij", U, G)
    if model == NEOHOOKE:
        F = np.eye(dim) + H
        det = np.linalg.det(F)
        tau = Mi.material_batch(dim, mu, nu, F)[0]
        P = tau @ np.swapaxes(np.linalg.inv(F), -1, -2)  # tau F^-T
    else:
        lam = 2 * mu * nu / (1 - 2 * nu)
        eps = 0.5 * (H + np.swapaxes(H, -1, -2))
        P = lam * np.trace(eps, axis1=-2, axis2=-1)[..., None, None] * np.eye(dim) + 2 * mu * eps
        det = np.ones(JxW.shape)
    fe = np.einsum("eqcj,eqaj,eq->eac", P, G, JxW)
    A = np.asarray(acc, float).reshape(-1, dim)[conn]
    aq = np.einsum("qa,eac->eqc", N, A)
    ie = rho * np.einsum("qa,eqc,eq->eac", N, aq, JxW)
    We = np.einsum("qa,eq->ea", N, JxW)
    internal, inertia, W = np.zeros((mesh.nnodes, dim)), np.zeros((mesh.nnodes, dim)), np.zeros(mesh.nnodes)
    np.add.at(internal, conn, fe)
    np.add.at(inertia, conn, ie)
    np.add.at(W, conn, We)
    return internal.reshape(-1), inertia.reshape(-1), W, det.min()


def traction_load(mesh, u, traction):
    """the interface faces' contribution as the nonlinear assembly forms it, unmasked"""
    dim = mesh.dim
    load = np.zeros(mesh.n)
    for conn, verts, bfaces in mesh.cells:
        ifaces = [f for f, role in bfaces.items() if role == Mi.INTERFACE]
        if ifaces:
            d = mesh.dofs(conn)
            load[d] += Mi.neumann_cell(dim, mesh.p, verts, u[d].reshape(-1, dim), traction[d].reshape(-1, dim), ifaces)
    return load


def terms(mesh, model, u, acc, mu, nu, rho, body=None, traction=None, load=None):
    """terms[4, n] = internal, inertia, body, load; and the smallest det F.  model 0: body (dim numbers) and the nodal traction
    vector; model 1: the load vector as it is"""
    dim = mesh.dim
    internal, inertia, W, det = cell_terms(mesh, model, u, acc, mu, nu, rho)
    if model == NEOHOOKE:
        b = rho * np.outer(W, np.asarray(body, float)[:dim]).reshape(-1)
        ld = traction_load(mesh, np.asarray(u, float), np.asarray(traction, float))
    else:
        b, ld = np.zeros(mesh.n), np.asarray(load, float).copy()
    return np.array([internal, inertia, b, ld]), det


def _embed(mesh, v):
    out = np.zeros((mesh.nnodes, 3))
    out[:, :mesh.dim] = np.asarray(v).reshape(-1, mesh.dim)
    return out


def sum_and_moment(mesh, x, f):
    """(sum f_i, sum x_i x f_i) and the absolute sums of the same products: (force[3], moment[3], force scale[3], moment scale[3])"""
    f3, x3 = _embed(mesh, f), _embed(mesh, x)
    a3, ax = np.abs(f3), np.abs(x3)
    return (f3.sum(axis=0), np.cross(x3, f3).sum(axis=0), a3.sum(axis=0),
            np.stack([ax[:, 1] * a3[:, 2] + ax[:, 2] * a3[:, 1], ax[:, 2] * a3[:, 0] + ax[:, 0] * a3[:, 2],
                      ax[:, 0] * a3[:, 1] + ax[:, 1] * a3[:, 0]], axis=1).sum(axis=0))


def resultants(mesh, model, u, T, about=None):
    """what mi_reaction_info holds, from terms T[4, n]: a dict with, per set of SETS, the force, `<set>_moment`, and
    `<set>_scale`, `<set>_moment_scale` -- the sums of the absolute values of the same addends (for reaction and unbalanced: of all
    four terms on those dofs, since forces is their sum), the scale of a sum's round-off"""
    dim = mesh.dim
    x0 = np.zeros(dim) if about is None else np.asarray(about, float)
    x = mesh.coords + (np.asarray(u, float).reshape(-1, dim) if model == NEOHOOKE else 0.0) - x0
    r = T[0] + T[1] - T[2] - T[3]
    con = mesh.constrained
    tabs = np.abs(T).sum(axis=0)
    out = dict(forces=r, about=np.concatenate([x0, np.zeros(3 - dim)]))
    for name, f, a in (("reaction", r * con, tabs * con), ("unbalanced", r * ~con, tabs * ~con), ("inertia", T[1], None),
                       ("body", T[2], None), ("load", T[3], None), ("internal", T[0], None)):
        s, m, ss, ms = sum_and_moment(mesh, x, f)
        if a is not None:
            _, _, ss, ms = sum_and_moment(mesh, x, a)
        out[name], out[name + "_moment"], out[name + "_scale"], out[name + "_moment_scale"] = s, m, ss, ms
    out["internal_abs"] = np.abs(T[0]).sum()
    out["max_unbalanced"] = np.abs(r * ~con).max()
    R = np.linalg.norm((r * con).reshape(-1, dim), axis=1)
    out["max_reaction"], out["max_reaction_node"] = R.max(), int(np.argmax(R))
    return out
