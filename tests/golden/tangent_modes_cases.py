"""The cases of the tangent's modal analysis (mi_tangent_modes): meshes, committed states and the number of wanted modes, shared by
tests/test_mirror_tangent_modes.py (numpy mirror) and tests/test_gpu_tangent_modes.py (device).  The smallest meshes that
still reach every product form: 3D Q2 and Q3 (assembled and matrix-free fine level), Q1 and Q4 (generic kernels), 2D, and
meshes with perturbed vertices.  Default material (mu 0.5e6, nu 0.4, rho 1000) and Newmark parameters (beta 1/4, dt 0.005:
alpha_1 = 1.6e5).

States are functions of the node coordinates X that vanish on the clamped face x = 0:
  zero      u = 0
  stretch   u_x = 0.05 X_x
  bend      stretch plus a smooth transverse field (u_y quadratic in x; 3D: u_z as well)
  compress  u_x = -0.05 X_x   (the slender 2D strip is past buckling there: lambda_0 < 0, A = K_T + alpha_1 rho M still SPD)
"""
import numpy as np

import mirror as Mi

CL, IF = Mi.CLAMPED, Mi.INTERFACE
XM_3D = [CL] + [IF] * 5
XM_2D = [CL, IF, IF, IF, 0, 0]
ALPHA1 = 1.0 / (0.25 * 0.005**2)
RHO = 1000.0

# perturb: standard deviation of the vertex offsets relative to the smallest cell edge (vertices on x = 0 stay: the states
# and the clamped face are defined there)
CASES = {
    "q2_311": dict(dim=3, p=2, reps=(3, 1, 1), hi=(1.5, 0.3, 0.3), roles=XM_3D, n_modes=5, states=["zero", "stretch"]),
    # the same beam compressed by 5 %: past buckling in 3D (four wanted modes: the fifth would cut a cluster)
    "q2_311_buckled": dict(dim=3, p=2, reps=(3, 1, 1), hi=(1.5, 0.3, 0.3), roles=XM_3D, n_modes=4, states=["compress"]),
    "q3_211": dict(dim=3, p=3, reps=(2, 1, 1), hi=(1.0, 0.3, 0.22), roles=XM_3D, n_modes=3, states=["bend"]),
    "q1_422": dict(dim=3, p=1, reps=(4, 2, 2), hi=(1.2, 0.3, 0.22), roles=XM_3D, n_modes=3, states=["stretch"]),
    "q4_111": dict(dim=3, p=4, reps=(1, 1, 1), hi=(0.8, 0.3, 0.22), roles=XM_3D, n_modes=2, states=["bend"]),
    "2d_q2_61": dict(dim=2, p=2, reps=(6, 1), hi=(3.0, 0.25), roles=XM_2D, n_modes=3, states=["zero", "stretch", "compress"]),
    "2d_q3_32p": dict(dim=2, p=3, reps=(3, 2), hi=(1.5, 0.4), roles=XM_2D, n_modes=3, states=["bend"], perturb=0.04),
    "q2_221p": dict(dim=3, p=2, reps=(2, 2, 1), hi=(1.0, 0.4, 0.15), roles=XM_3D, n_modes=3, states=["bend"], perturb=0.04),
}
# matrix-free fine level ("fine_level" 1) exists for 3D Q2 and Q3
FINE_LEVEL_CASES = ["q2_311", "q2_311_buckled", "q3_211", "q2_221p"]
RUNS = [(name, state) for name, c in CASES.items() for state in c["states"]]

_meshes = {}


def case_geometry(name):
    """lo, hi, perturb (vertex offsets [nverts, dim], x fastest, or None)"""
    c = CASES[name]
    dim, reps = c["dim"], np.array(c["reps"])
    lo, hi = (0.0,) * dim, tuple(c["hi"])
    if "perturb" not in c:
        return lo, hi, None
    h = (np.array(hi) / reps).min()
    nv = reps + 1
    rng = np.random.default_rng(int(reps.sum()) + 10 * c["p"])
    off = c["perturb"] * h * rng.standard_normal((int(np.prod(nv)), dim))
    vid = np.stack(np.unravel_index(np.arange(int(np.prod(nv))), tuple(nv[::-1])), -1)[:, ::-1]  # vertices, x fastest
    off[vid[:, 0] == 0] = 0.0
    return lo, hi, off


def case_mesh(name):
    if name not in _meshes:
        c = CASES[name]
        lo, hi, perturb = case_geometry(name)
        _meshes[name] = Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, c["roles"], perturb=perturb)
    return _meshes[name]


def state(kind, X):
    """the committed displacement [n] at the nodes X [nnodes, dim]"""
    dim = X.shape[1]
    u = np.zeros_like(X)
    if kind == "zero":
        return u.reshape(-1)
    x = X[:, 0]
    L = x.max()
    u[:, 0] = (-0.05 if kind == "compress" else 0.05) * x
    if kind == "bend":
        u[:, 1] = 0.04 * x * x / L
        if dim == 3:
            u[:, 2] = 0.02 * x * np.sin(2.0 * X[:, 1])
    else:
        assert kind in ("stretch", "compress"), kind
    return u.reshape(-1)
