"""Reference of the modal analysis (mi_linear_modes): the lowest eigenpairs of  K phi = lambda M phi  on the free dofs, by a
dense scipy.linalg.eigh of K_ff, M_ff.  The matrices are mirror.Linear's on the CPU (tests/test_mirror_modes.py) and the
assembled context's own exported ones on the device (tests/test_gpu_linear_modes.py); this file owns the cases, the
eigen-decomposition and the quantities the assertions of both are derived from.

  free_pencil()   K_ff, M_ff (dense, symmetrised) and the free dofs
  eigh_free()     all eigenpairs of the pencil, ascending, eigenvectors M-orthonormal
  rigid_count()   dimension of the null space of K_ff the boundary conditions leave: 0 with a clamped face, else the rigid
                  motions of the plane (3) or of space (6)
  gaps()          per wanted j the distance of lambda_j to the nearest reference eigenvalue outside its own cluster (the rigid
                  cluster counts as one)

Nothing here comes from the device code.
"""
import numpy as np
import scipy.linalg as sla

import mg_reference as R
import mirror as Mi

DT, THETA = 0.02, 0.5
IF = Mi.INTERFACE
ALL_IF_2D = [IF, IF, IF, IF, 0, 0]
ALL_IF_3D = [IF] * 6
XM_CLAMPED = [Mi.CLAMPED] + [IF] * 5

CASES = {
    "q3_212d": dict(dim=3, p=3, reps=(2, 1, 2), kind="distorted", roles=R.ROLES_A, n_modes=6),  # also run matrix-free
    "q2_432g": dict(dim=3, p=2, reps=(4, 3, 2), kind="graded", roles=R.ROLES_A, n_modes=14),  # m = 17, 3 m = 51
    "q1_543d": dict(dim=3, p=1, reps=(5, 4, 3), kind="distorted", roles=R.ROLES_B, n_modes=1),
    "q4_211": dict(dim=3, p=4, reps=(2, 1, 1), kind="graded", roles=XM_CLAMPED, n_modes=4),
    "2d_q2_93": dict(dim=2, p=2, reps=(9, 3), kind="graded", roles=R.ROLES_2D, n_modes=5),
    "2d_q3_free": dict(dim=2, p=3, reps=(5, 2), kind="graded", roles=ALL_IF_2D, n_modes=6),  # 3 rigid modes
    "q2_free3d": dict(dim=3, p=2, reps=(3, 2, 2), kind="graded", roles=ALL_IF_3D, n_modes=10),  # 6 rigid modes
}

_meshes = {}


def case_geometry(name):
    c = CASES[name]
    return R.geometry(c["kind"], c["dim"], c["reps"], seed=sum(c["reps"]))


def case_mesh(name):
    if name not in _meshes:
        c = CASES[name]
        lo, hi, perturb = case_geometry(name)
        _meshes[name] = Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, c["roles"], perturb=perturb)
    return _meshes[name]


def rigid_count(name):
    c = CASES[name]
    if any(r in (Mi.CLAMPED, Mi.ZCLAMP) for r in c["roles"][:2 * c["dim"]]):
        return 0
    return 3 if c["dim"] == 2 else 6


def free_pencil(K, M, constrained):
    """dense K_ff, M_ff (symmetrised) of dense or scipy.sparse K, M, and the indices of the free dofs"""
    free = np.flatnonzero(~np.asarray(constrained, dtype=bool))
    dense = lambda A: np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)  # noqa: E731
    Kf, Mf = dense(K)[np.ix_(free, free)], dense(M)[np.ix_(free, free)]
    return 0.5 * (Kf + Kf.T), 0.5 * (Mf + Mf.T), free


def eigh_free(Kf, Mf):
    return sla.eigh(Kf, Mf)


def gaps(w, n_modes, n_rigid):
    """gap_j, j < n_modes: distance of w[j] to the nearest eigenvalue that does not belong to j's cluster.  The rigid modes
    w[:n_rigid] form one cluster; every other eigenvalue is a cluster of its own."""
    w = np.asarray(w)
    g = np.zeros(n_modes)
    for j in range(n_modes):
        if j < n_rigid:
            g[j] = w[n_rigid] - w[j]
        else:
            lo = w[j] - w[j - 1] if j > 0 else np.inf
            g[j] = min(lo, w[j + 1] - w[j])
    return g


def condition(w, n_modes, n_rigid):
    """(smallest gap among the first n_modes + 3 eigenvalues outside the rigid cluster, relative to lambda_n_modes;
    lambda_max / lambda_n_modes)"""
    top = w[n_modes - 1]
    hi = min(len(w), n_modes + 3)
    d = np.diff(w[max(n_rigid - 1, 0):hi]) if n_rigid else np.diff(w[:hi])
    return d.min() / top, w[-1] / top
