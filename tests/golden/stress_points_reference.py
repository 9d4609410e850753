"""Numpy reference of the stress at arbitrary points (mi_evaluate_stress), of the principal stresses (mi_principal_stress) and of
the consistent stress recovery (tuning "stress_projection" 1), from mirror.py's pieces (shape_at, q1_map, q1_jacobian, material)
and from stress_reference.py / projection_reference.py.

Points are (cell, xi) pairs, as in point_eval_reference.py: no location is needed, each lies in its cell by construction.

  raw()                 sigma_h at the pairs: stress_reference.point_stress of grad u_h there, in the pair's cell
  interpolate()         sum_a N_a(xi) s_a of a nodal field s [nnodes, ncomp] at the pairs
  quadrature_pairs()    every point of the model's rule in every cell as pairs, with N and JxW: what the lumped sums run over
  lumped()              sum N_i s JxW / W_i of point values, stress_reference.nodal_stress's sums from given point values
  consistent()          the dense solve M sigma*_k = b_k, M = projection_reference.scalar_mass (QGauss(p + 2)), b on the model's rule
  principal()           the device's eigen-solver statement by statement in Python floats (no fused multiply-adds): 3D cyclic
                        Jacobi with SWEEPS sweeps over (0,1), (0,2), (1,2), 2D the closed form through hypot; descending order,
                        ties in place, the component of largest magnitude of every vector positive (the first on ties)
  eig_figures()         how good eigenpairs are, measured against the tensor alone (no gap-dependent comparison of vectors)
"""
import math

import numpy as np

import projection_reference as PR
import stress_reference as S
from mirror import feq_nodes, gauss01, q1_jacobian, shape_at

EPS = np.finfo(float).eps
SWEEPS = 8  # SYM_EIG_SWEEPS
# The mirror's worst figures on eig_tensors(), as test_mirror_stress_points.py measures and prints them (it holds them to be
# upper bounds): residual and trace in eps |sigma|_F -- 3D 1.61 and 1.64, 2D 0.86 and 0.93 --, orthonormality in eps -- 3D 6.00,
# 2D 1.00.  The device is gated at 8 x these (fused multiply-adds, another rounding of the sweeps)
MIRROR_EIG_RES, MIRROR_EIG_ORTH = 1.65, 6.0


def raw(mesh, u, mu, nu, model, cells, xi):
    """(sigma [n, ncomp], det F [n]) of the element's own stress at the (cell, xi) pairs"""
    dim, p = mesh.dim, mesh.p
    nodes = feq_nodes(p)
    U = np.asarray(u, float).reshape(-1, dim)
    out, det = np.zeros((len(cells), len(S.PAIRS[dim]))), np.zeros(len(cells))
    for k, (c, x) in enumerate(zip(cells, xi)):
        conn, verts, _ = mesh.cells[c]
        _, dN = shape_at(dim, p, nodes, x)
        H = U[conn].T @ (dN @ np.linalg.inv(q1_jacobian(dim, verts, x)))
        s, det[k] = S.point_stress(dim, mu, nu, H, model)
        out[k] = [s[d, e] for d, e in S.PAIRS[dim]]
    return out, det


def interpolate(mesh, nodal, cells, xi):
    """the nodal field [nnodes, ncomp] at the (cell, xi) pairs, with the element's basis"""
    nodes = feq_nodes(mesh.p)
    nodal = np.asarray(nodal, float)
    return np.array([shape_at(mesh.dim, mesh.p, nodes, x)[0] @ nodal[mesh.cells[c][0]] for c, x in zip(cells, xi)])


def quadrature_pairs(mesh, model):
    """(cells [n], xi [n, dim], N [n, npc], JxW [n]) of every point of the model's rule (model 0 QGauss(p + 2), model 1
    QGauss(p + 1)) in every cell, x fastest"""
    dim, p = mesh.dim, mesh.p
    nq = p + 2 if model == S.NEOHOOKE else p + 1
    nodes = feq_nodes(p)
    qx, qw = gauss01(nq)
    cells, xi, N, JxW = [], [], [], []
    for c, (_, verts, _) in enumerate(mesh.cells):
        for q in np.ndindex(*([nq] * dim)):
            qi = q[::-1]
            x = np.array([qx[k] for k in qi])
            cells.append(c)
            xi.append(x)
            N.append(shape_at(dim, p, nodes, x)[0])
            JxW.append(np.linalg.det(q1_jacobian(dim, verts, x)) * np.prod([qw[k] for k in qi]))
    return np.array(cells), np.array(xi), np.array(N), np.array(JxW)


def load(mesh, cells, values, N, JxW):
    """(b [nnodes, ncomp], W [nnodes]): sum N_i s JxW and sum N_i JxW of the point values [n, ncomp]"""
    b, W = np.zeros((mesh.nnodes, values.shape[1])), np.zeros(mesh.nnodes)
    for c, s, n, w in zip(cells, values, N, JxW):
        conn = mesh.cells[c][0]
        W[conn] += n * w
        b[conn] += (n * w)[:, None] * s[None, :]
    return b, W


def lumped(mesh, cells, values, N, JxW):
    b, W = load(mesh, cells, values, N, JxW)
    return b / W[:, None]


def consistent(mesh, u, mu, nu, model):
    """(sigma* [nnodes, ncomp], b, W, dense scalar mass) of the consistent projection of the state u"""
    cells, xi, N, JxW = quadrature_pairs(mesh, model)
    b, W = load(mesh, cells, raw(mesh, u, mu, nu, model, cells, xi)[0], N, JxW)
    M = PR.scalar_mass(mesh)
    return np.linalg.solve(M, b), b, W, M


# ---------------------------------------------------------------------------------------------- principal stresses
def _rotate(A, V, p, q, r):
    apq = A[p][q]
    if apq != 0.0:
        theta = (A[q][q] - A[p][p]) / (2.0 * apq)
        with np.errstate(over="ignore"):
            t = math.copysign(1.0, theta) / (abs(theta) + float(np.sqrt(np.float64(theta) * np.float64(theta) + 1.0)))
        c = 1.0 / math.sqrt(t * t + 1.0)
        s = t * c
        A[p][p] -= t * apq
        A[q][q] += t * apq
        A[p][q] = A[q][p] = 0.0
        arp, arq = A[r][p], A[r][q]
        A[r][p] = A[p][r] = c * arp - s * arq
        A[r][q] = A[q][r] = s * arp + c * arq
        for k in range(3):
            vkp, vkq = V[k][p], V[k][q]
            V[k][p] = c * vkp - s * vkq
            V[k][q] = s * vkp + c * vkq


def _eig3(a):
    A = [[a[0], a[3], a[4]], [a[3], a[1], a[5]], [a[4], a[5], a[2]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    lam = [A[k][k] for k in range(3)]
    E = [[V[c][k] for c in range(3)] for k in range(3)]
    for lo in (0, 1, 0):
        if lam[lo] < lam[lo + 1]:
            lam[lo], lam[lo + 1] = lam[lo + 1], lam[lo]
            E[lo], E[lo + 1] = E[lo + 1], E[lo]
    return lam, E


def _eig2(a):
    xx, yy, xy = a
    m, d = 0.5 * (xx + yy), 0.5 * (xx - yy)
    r = math.hypot(d, xy)
    x, y = 1.0, 0.0
    if r > 0.0:
        ex, ey = (d + r, xy) if d >= 0.0 else (xy, r - d)
        h = math.hypot(ex, ey)
        x, y = ex / h, ey / h
    return [m + r, m - r], [[x, y], [-y, x]]


def principal(dim, sigma):
    """(principal [n, dim], directions [n, dim, dim]) of the tensors sigma [n, ncomp] by the device's statements"""
    sigma = np.asarray(sigma, float).reshape(-1, len(S.PAIRS[dim]))
    lam, dirs = np.zeros((len(sigma), dim)), np.zeros((len(sigma), dim, dim))
    for i, a in enumerate(sigma):
        l, E = (_eig3 if dim == 3 else _eig2)([float(v) for v in a])
        for k in range(dim):
            big = E[k][0]
            for c in range(1, dim):
                if abs(E[k][c]) > abs(big):
                    big = E[k][c]
            sg = -1.0 if big < 0.0 else 1.0
            dirs[i, k] = [sg * e for e in E[k]]
        lam[i] = l
    return lam, dirs


def full_tensor(dim, a):
    T = np.zeros((dim, dim))
    for v, (d, e) in zip(a, S.PAIRS[dim]):
        T[d, e] = T[e, d] = v
    return T


def eig_figures(dim, sigma, lam, dirs):
    """the worst of: |sigma v_k - lambda_k v_k|_2 / (eps |sigma|_F), |V V^T - I|_max / eps, |sum lambda - tr sigma| / (eps |sigma|_F)
    over the tensors (a zero tensor: the residual and trace figures count absolutely, they must be 0); and whether every tensor's
    values descend and every vector's component of largest magnitude, the first such, is positive"""
    res = orth = tr = 0.0
    ordered = signed = True
    for a, l, V in zip(np.asarray(sigma, float).reshape(len(lam), -1), lam, dirs):
        T = full_tensor(dim, a)
        scale = EPS * np.linalg.norm(T) if np.any(T != 0.0) else 1.0
        res = max(res, max(np.linalg.norm(T @ V[k] - l[k] * V[k]) for k in range(dim)) / scale)
        orth = max(orth, np.abs(V @ V.T - np.eye(dim)).max() / EPS)
        tr = max(tr, abs(l.sum() - np.trace(T)) / scale)
        ordered = ordered and all(l[k] >= l[k + 1] for k in range(dim - 1))
        for k in range(dim):
            signed = signed and V[k][int(np.argmax(np.abs(V[k])))] > 0.0  # (argmax: the first of equal magnitudes)
    return res, orth, tr, ordered, signed


_eig_tensors = {}


def eig_tensors(dim):
    """the tensors the eigen-solver is tested on, CPU mirror and device alike: the raw stress of the random admissible state of
    a perturbed Q2 case of stress_cases.py at 64 interior points (model 0), and the hand-made ones.  Built once"""
    if dim not in _eig_tensors:
        import point_eval_cases as PC
        import stress_cases as SC
        c = SC.case(*(SC.Q2_MESHES[1] if dim == 3 else SC.GENERIC_MESHES[1]), True)
        cells, xi = PC.interior_pairs(c["mesh"], 64, np.random.default_rng(40 + dim))
        _eig_tensors[dim] = np.concatenate([raw(c["mesh"], c["u"], SC.MU, SC.NU, S.NEOHOOKE, cells, xi)[0], hand_made_tensors(dim)])
    return _eig_tensors[dim]


def hand_made_tensors(dim):
    """tensors an eigen-solver can go wrong at: hydrostatic, two equal eigenvalues, zero, already diagonal (ascending, so the
    sort has work), a rotated pair of equal values, and a general tensor scaled by 1e8 and 1e-8"""
    if dim == 2:
        base = [[3.0, 3.0, 0.0], [-2.5, -2.5, 0.0], [0.0, 0.0, 0.0], [1.0, 4.0, 0.0], [4.0, 1.0, 0.0], [2.0, 2.0, 1.5],
                [1.0, -1.0, 1e-9], [0.3, -1.7, 0.9], [-0.4, 0.2, -2.2]]
    else:
        c, s = math.cos(0.7), math.sin(0.7)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, s, c], [0.0, -c, s]])
        T = R @ np.diag([2.0, 2.0, -1.0]) @ R.T  # two equal eigenvalues, not aligned with the axes
        base = [[3.0, 3.0, 3.0, 0.0, 0.0, 0.0], [-2.5, -2.5, -2.5, 0.0, 0.0, 0.0], [0.0] * 6, [1.0, 2.0, 4.0, 0.0, 0.0, 0.0],
                [4.0, 2.0, 1.0, 0.0, 0.0, 0.0], [2.0, 2.0, -1.0, 0.0, 0.0, 0.0], [T[d, e] for d, e in S.PAIRS[3]],
                [1.0, 1.0, 1.0, 0.5, 0.5, 0.5], [1.0, -1.0, 0.5, 1e-9, 0.0, 2e-9], [0.3, -1.7, 0.9, 0.8, -0.6, 1.1],
                [-0.4, 0.2, -2.2, 1.3, 0.7, -0.9]]
    base = np.array(base)
    return np.concatenate([base, 1e8 * base[-2:], 1e-8 * base[-2:]])
