"""Reference of the tangent's modal analysis (mi_tangent_modes): the lowest eigenpairs of  K_T(u) phi = lambda rho M phi  on the
free dofs by a dense scipy.linalg.eigh.  K_T is the tangent the solver steps with, minus its mass term: on the CPU
mirror.Solid.assemble minus alpha_1 times the mirror's mass (projection_reference.scalar_mass: rho N N on QGauss(p + 2), the rule
the tangent integrates its mass with); on the device the context's own exported tangent minus alpha_1 rho times the dense mass
from mass_apply on unit columns.  free_pencil, eigh_free and condition are modes_reference's.

  mirror_pencil()   A_ff = (K_T + alpha_1 rho M)_ff, rho M_ff, K_T_ff = their difference, and the free dofs, of a case and state
  clusters()        the wanted eigenvalues grouped: neighbours closer than CLUSTER_REL |lambda|_top belong together (the double
                    bending modes of a beam with a square section)
  gaps()            per wanted j the distance of its cluster to the nearest eigenvalue outside it
  floor()           the a priori rounding bound of K_T x formed as A x - alpha_1 rho M x, relative to the stopping rule's scale
Nothing here comes from the device code.
"""
import numpy as np

import mirror as Mi
import modes_reference as MR
import projection_reference as PR
import tangent_modes_cases as TC

EPS = np.finfo(np.float64).eps
CLUSTER_REL = 1e-6  # of max |lambda_k|, k < n_modes: closer neighbours form one cluster
free_pencil, eigh_free, condition = MR.free_pencil, MR.eigh_free, MR.condition


def vector_mass(mesh, rho=TC.RHO):
    """rho M, dense [n, n], dof = dim * node + component"""
    return rho * np.kron(PR.scalar_mass(mesh), np.eye(mesh.dim))


def mirror_pencil(name, kind):
    mesh = TC.case_mesh(name)
    s = Mi.Solid(mesh)
    assert s.a1 == TC.ALPHA1 and s.rho == TC.RHO
    s.u = TC.state(kind, mesh.coords)
    A, _ = s.assemble(np.zeros(mesh.n))
    Af, Mf, free = free_pencil(A, vector_mass(mesh), mesh.constrained)
    return Af, Mf, Af - TC.ALPHA1 * Mf, free


def clusters(w, n_modes):
    """[(first, last + 1)] over the eigenvalues that the first n_modes belong to"""
    w = np.asarray(w)
    near = CLUSTER_REL * np.abs(w[:n_modes]).max()
    out, a = [], 0
    while a < n_modes:
        b = a + 1
        while b < len(w) and w[b] - w[b - 1] <= near:
            b += 1
        out.append((a, b))
        a = b
    return out


def gaps(w, n_modes):
    """gap_j, j < n_modes, and the cluster (a, b) of every j"""
    w = np.asarray(w)
    g, of = np.zeros(n_modes), []
    for a, b in clusters(w, n_modes):
        lo = w[a] - w[a - 1] if a > 0 else np.inf
        hi = w[b] - w[b - 1] if b < len(w) else np.inf
        for j in range(a, min(b, n_modes)):
            g[j] = min(lo, hi)
            of.append((a, b))
    return g, of


def floor(Af, Mf, X, lam_scale, alpha1=TC.ALPHA1):
    """Per column x_j of X [n_free, k]: the bound on |fl(A x - alpha_1 (rho M x)) - K_T x|_2 relative to lam_scale |rho M x|_2.
    Each entry of A x and of rho M x is a sum of at most r products, r the longest row; summed in any order its error is at
    most gamma_r (|A| |x|)_i resp. gamma_r (rho |M| |x|)_i (Higham, Accuracy and Stability, (3.5)); scaling by alpha_1 and the
    subtraction add two roundings: gamma_(r + 2) (|A| |x| + alpha_1 rho |M| |x|) bounds the difference's error."""
    r = int((np.abs(Af) > 0).sum(axis=1).max()) + 2
    gamma = r * EPS / (1 - r * EPS)
    err = gamma * (np.abs(Af) @ np.abs(X) + alpha1 * (np.abs(Mf) @ np.abs(X)))
    return np.linalg.norm(err, axis=0) / (lam_scale * np.linalg.norm(Mf @ X, axis=0))
