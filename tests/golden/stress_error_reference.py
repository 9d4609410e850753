"""Numpy reference of the a posteriori stress error indicator (mi_stress_error), from mirror.py and stress_reference.py alone.

With sigma*_i the nodal field of stress_reference.nodal_stress (the lumped L2 projection), sigma*(q) = sum_i N_i(q) sigma*_i and
e(q) = sigma*(q) - sigma_h(q) at the points of the model's own rule:

  m(s)     = ( s:s - c tr(s)^2 ) / (2 mu)        s:s counts an off-diagonal entry twice; c = nu / (1 + nu) in 3D, nu in 2D (the
                                                 plane-strain compliance of the 2 x 2 formulation, which has no sigma_zz)
  eta_K^2  = sum_{q in K} m(e(q)) JxW(q)         n_K^2 = sum_{q in K} m(sigma_h(q)) JxW(q)
  eta = sqrt(sum_K eta_K^2)    n = sqrt(sum_K n_K^2)    relative = eta / sqrt(n^2 + eta^2)   (0 where both vanish)

Cells in lexicographic order, x fastest -- the order of mirror.Mesh.cells.  The Zienkiewicz-Zhu indicator in the complementary
energy norm: for model 1, n^2 = u^T K u on the model's rule.  dtype: every sum, sigma* included, can be carried in
np.longdouble (the conditioning check of test_mirror_stress_error.py).
"""
import numpy as np

import stress_reference as S


def metric(dim, mu, nu, s):
    """m(s) of s given as its ncomp unique entries (stress_reference.PAIRS: the diagonal first)"""
    c = nu if dim == 2 else nu / (1 + nu)
    d, o = s[:dim], s[dim:]
    tr = d.sum()
    return ((d * d).sum() + 2 * (o * o).sum() - c * tr * tr) / (2 * mu)


def stress_error(mesh, u, mu, nu, model, dtype=np.float64, pts=None, sigma=None):
    """dict(eta2_cell, n2_cell [ncells]; eta_cell, norm_cell; error, norm, relative, max_cell_error, max_cell) of the state u.
    pts: stress_reference.points(mesh, u, mu, nu, model), to share them; sigma: the nodal field, else nodal_stress in dtype"""
    dim = mesh.dim
    if pts is None:
        pts = S.points(mesh, u, mu, nu, model)
    if sigma is None:
        sigma = S.nodal_stress(mesh, u, mu, nu, model, dtype=dtype, pts=pts)[0]
    sigma = np.asarray(sigma, dtype)
    ncells = len(mesh.cells)
    per_cell = len(pts) // ncells
    assert per_cell * ncells == len(pts)
    eta2, n2 = np.zeros(ncells, dtype), np.zeros(ncells, dtype)
    for k, (conn, N, s, JxW, _) in enumerate(pts):
        K = k // per_cell
        sh = s.astype(dtype)
        e = N.astype(dtype) @ sigma[conn] - sh
        eta2[K] += metric(dim, mu, nu, e) * dtype(JxW)
        n2[K] += metric(dim, mu, nu, sh) * dtype(JxW)
    eta_cell, norm_cell = np.sqrt(eta2), np.sqrt(n2)
    e2, nn2 = eta2.sum(), n2.sum()
    tot = e2 + nn2
    k = int(np.argmax(eta_cell))  # the first of equal maxima: the smallest lexicographic id
    return dict(eta2_cell=eta2, n2_cell=n2, eta_cell=eta_cell, norm_cell=norm_cell, error=np.sqrt(e2), norm=np.sqrt(nn2),
                relative=np.sqrt(e2 / tot) if tot > 0 else dtype(0.0), max_cell_error=eta_cell[k], max_cell=k)
