"""numpy reference of the explicit time integrator (mi_explicit_setup / mi_explicit_run / mi_explicit_stable_dt), built from
mirror.py: the lumped weights W_i = sum_q N_i JxW on QGauss(p + 2) from shape_at / q1_jacobian, the force as Solid.assemble's
residual with a = 0 (a residual-only, vectorised copy of mirror.cell and mirror.neumann_cell; test_mirror_explicit.py holds it to
Solid.assemble), the velocity-Verlet step, a Lanczos in the M_L inner product, and the case list shared by
tests/test_mirror_explicit.py (CPU) and tests/test_gpu_explicit.py (device).

The scheme, with minv = 1 / (rho W) on free dofs and 0 on constrained ones:
    du = dt v + dt^2 / 2 a;   F = force(u + du);   a' = minv F;   v <- v + dt / 2 (a + a');   u <- u + du;   a <- a'
"""
import numpy as np

import mirror as Mi

CL, IF = Mi.CLAMPED, Mi.INTERFACE
ROLES_3D = [CL, IF, 0, 0, 0, 0]  # x = 0 clamped, x = L the interface, the rest free
ROLES_2D = [CL, IF, 0, 0, 0, 0]
MU, NU, RHO = 0.5e6, 0.4, 1000.0
BODY = (0.0, -9.81, 2.0)
H = 0.1  # cell edge

# every case: a clamped face, an interface face with a non-uniform traction, a body force
CASES = {
    "q2_311p": dict(dim=3, p=2, reps=(3, 1, 1), perturb=0.04),  # odd cell count: the last wave of the two-cells-per-wave pass holds one cell
    "q2_222": dict(dim=3, p=2, reps=(2, 2, 2)),  # every colour present
    "q3_211": dict(dim=3, p=3, reps=(2, 1, 1)),
    "q3_222": dict(dim=3, p=3, reps=(2, 2, 2)),
    "q1_222": dict(dim=3, p=1, reps=(2, 2, 2)),
    "q4_111": dict(dim=3, p=4, reps=(1, 1, 1)),
    "2d_q1_32": dict(dim=2, p=1, reps=(3, 2)),
    "2d_q2_61": dict(dim=2, p=2, reps=(6, 1)),
    "2d_q3_21": dict(dim=2, p=3, reps=(2, 1)),
    "2d_q4_11": dict(dim=2, p=4, reps=(1, 1)),
}
# the seven cases of the CPU checks that need a dense eigh (2D Q1-Q4, 3D Q1-Q3)
SMALL = ["2d_q1_32", "2d_q2_61", "2d_q3_21", "2d_q4_11", "q1_222", "q2_311p", "q3_211"]
FINE_LEVEL = ["q2_311p", "q2_222", "q3_211", "q3_222"]  # "fine_level" 1 exists for 3D Q2 and Q3
POINT_PASS_Q3 = ["q3_211", "q3_222"]
STEPS, CHECK_AT = 10, (1, 2, 5, 10)


def roles(name):
    return ROLES_3D if CASES[name]["dim"] == 3 else ROLES_2D


def geometry(name):
    """lo, hi, perturb (vertex offsets [nverts, dim], x fastest, or None; the vertices on x = 0 stay)"""
    c = CASES[name]
    dim, reps = c["dim"], np.array(c["reps"])
    lo, hi = (0.0,) * dim, tuple(H * reps)
    if "perturb" not in c:
        return lo, hi, None
    nv = reps + 1
    rng = np.random.default_rng(int(reps.sum()) + 10 * c["p"])
    off = c["perturb"] * H * rng.standard_normal((int(np.prod(nv)), dim))
    vid = np.stack(np.unravel_index(np.arange(int(np.prod(nv))), tuple(nv[::-1])), -1)[:, ::-1]
    off[vid[:, 0] == 0] = 0.0
    return lo, hi, off


def initial_state(X):
    """u [n] with |u| about 3e-3 and v [n] with |v| up to 8 at the nodes X [nnodes, dim]; both vanish on x = 0"""
    dim = X.shape[1]
    x, L = X[:, 0], X[:, 0].max()
    s = x / L
    u, v = np.zeros_like(X), np.zeros_like(X)
    u[:, 0] = 3e-3 * s
    u[:, 1] = 2e-3 * s * s
    v[:, 0] = -3.0 * s
    v[:, 1] = 8.0 * s * np.cos(3.0 * X[:, 1])
    if dim == 3:
        u[:, 2] = 1e-3 * s * np.sin(5.0 * X[:, 1])
        v[:, 2] = 4.0 * s * s
    return u.reshape(-1), v.reshape(-1)


def traction(Xi):
    """a non-uniform traction [k, dim] at the interface nodes Xi [k, dim]"""
    dim = Xi.shape[1]
    t = np.zeros_like(Xi)
    t[:, 0] = 4e3 * (1.0 + 5.0 * Xi[:, 1])
    t[:, 1] = -6e3 * np.cos(4.0 * Xi[:, 1])
    if dim == 3:
        t[:, 2] = 2e3 * (Xi[:, 2] - 0.05) * 10.0
    return t


def fold_velocity(X, dt):
    """a compressive velocity field that drives the cells next to x = L through det F = 0 within a few steps of length dt"""
    x, L = X[:, 0], X[:, 0].max()
    v = np.zeros_like(X)
    v[:, 0] = -(0.3 * H / dt) * np.maximum(x - (L - H), 0.0) / H
    return v.reshape(-1)


def hash_start(n, dim, constrained):
    """column 0 of the device's block_hash_init: a fixed integer hash of the dof mapped to [-1, 1), zero on constrained dofs"""
    with np.errstate(over="ignore"):
        r = np.arange(n, dtype=np.uint64)
        h = (r * np.uint64(64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(30)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(27)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(31)
    u = (h >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0
    u[constrained] = 0.0
    return u


def _tau_batch(dim, F):
    """the Kirchhoff stress of mirror.material over a stack F[..., dim, dim], and det F"""
    kappa = 2 * MU * (1 + NU) / (3 * (1 - 2 * NU))
    I = np.eye(dim)
    J = np.linalg.det(F)
    e2 = (..., None, None)
    with np.errstate(invalid="ignore", divide="ignore"):
        tau_bar = MU * (J ** (-2.0 / dim))[e2] * (F @ np.swapaxes(F, -1, -2))
        tau_iso = tau_bar - (np.trace(tau_bar, axis1=-2, axis2=-1) / dim)[e2] * I
        p = kappa / 2 * (J - 1 / J)
    return (p * J)[e2] * I + tau_iso, J


class Reference:
    """one case: mesh, lumped masses, force and step"""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.dim, self.p = name, c["dim"], c["p"]
        lo, hi, perturb = geometry(name)
        self.mesh = m = Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, roles(name), perturb=perturb)
        dim, p = self.dim, self.p
        self.conn = np.array([cn for cn, _, _ in m.cells])
        self.verts = np.array([v for _, v, _ in m.cells])
        xi, w, self.N, dN = Mi._rule(dim, p, p + 2)
        Jm = Mi._q1_jacobians(dim, self.verts, xi)
        self.G = np.einsum("qak,eqkj->eqaj", dN, np.linalg.inv(Jm))
        self.JxW = np.linalg.det(Jm) * w
        # lumped weights W_i = sum_q N_i JxW per node, the same on every component
        Wn = np.zeros(m.nnodes)
        np.add.at(Wn, self.conn, np.einsum("qa,eq->ea", self.N, self.JxW))
        self.W = np.repeat(Wn, dim)
        self.mass = RHO * self.W
        self.constrained = m.constrained
        self.minv = np.where(m.constrained, 0.0, 1.0 / self.mass)
        self.body = np.array(BODY[:dim])
        self.stress = np.zeros(m.n)
        ids = m.interface_nodes
        self.stress.reshape(-1, dim)[ids] = traction(m.coords[ids])
        # Neumann faces: per (cell, face) the face-point shape values, n dA of the reference configuration, and the gradients
        # at the CELL point whose index equals the face-point counter (mirror.neumann_cell)
        nodes1 = Mi.feq_nodes(p)
        qx, _ = Mi.gauss01(p + 2)
        self.faces = []
        for e, (conn, verts, bfaces) in enumerate(m.cells):
            for face, role in bfaces.items():
                if role != IF:
                    continue
                pts, wts = Mi.face_points(dim, p, p + 2, face)
                Nf, nA, Gc = [], [], []
                for fq, (xi_f, wq) in enumerate(zip(pts, wts)):
                    Nq, _ = Mi.shape_at(dim, p, nodes1, xi_f)
                    Jf = Mi.q1_jacobian(dim, verts, xi_f)
                    n_ref = np.zeros(dim)
                    n_ref[face // 2] = 1.0 if face % 2 else -1.0
                    cof = np.linalg.det(Jf) * np.linalg.inv(Jf).T @ n_ref
                    qi = [(fq // (p + 2) ** d) % (p + 2) for d in range(dim)]
                    xi_c = np.array([qx[k] for k in qi])
                    _, dNc = Mi.shape_at(dim, p, nodes1, xi_c)
                    Nf.append(Nq)
                    nA.append((cof / np.linalg.norm(cof), np.linalg.norm(cof) * wq))
                    Gc.append(dNc @ np.linalg.inv(Mi.q1_jacobian(dim, verts, xi_c)))
                self.faces.append((e, np.array(Nf), np.array([a for a, _ in nA]), np.array([b for _, b in nA]), np.array(Gc)))

    def force(self, u, with_det=False):
        """-f_int(u) + rho b W + Neumann(u, stress), zero on constrained dofs: Solid.assemble's right-hand side with a = 0"""
        m, dim = self.mesh, self.dim
        U = u.reshape(-1, dim)[self.conn]  # [E, A, dim]
        F = np.eye(dim) + np.einsum("eai,eqaj->eqij", U, self.G)
        tau, J = _tau_batch(dim, F)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = self.G @ np.linalg.inv(F)  # spatial gradients [E, Q, A, dim]
        re = -np.einsum("eqaj,eqcj,eq->eac", g, tau, self.JxW)
        re += RHO * np.einsum("qa,c,eq->eac", self.N, self.body, self.JxW)
        T = self.stress.reshape(-1, dim)[self.conn]
        for e, Nf, normal, dA, Gc in self.faces:
            Ff = np.eye(dim) + np.einsum("ai,qaj->qij", U[e], Gc)
            scale = np.linalg.norm(np.linalg.det(Ff)[:, None] * np.einsum("qji,qj->qi", np.linalg.inv(Ff), normal), axis=1)
            tq = Nf @ T[e]  # [Qf, dim]
            re[e] += np.einsum("qa,qc,q->ac", Nf, tq, scale * dA)
        out = np.zeros((m.nnodes, dim))
        np.add.at(out, self.conn, re)
        out = out.reshape(-1)
        out[self.constrained] = 0.0
        return (out, J.min()) if with_det else out

    def initial(self):
        """u, v of initial_state and a = minv F(u), what mi_explicit_setup with init_acceleration 1 leaves"""
        u, v = initial_state(self.mesh.coords)
        return u, v, self.minv * self.force(u)

    def step(self, u, v, a, dt, noise=None):
        du = dt * v + 0.5 * dt * dt * a
        F = self.force(u + du)
        if noise is not None:
            F = F * (1.0 + 1e-15 * noise.standard_normal(F.shape))
        an = self.minv * F
        return u + du, v + 0.5 * dt * (a + an), an

    def run(self, u, v, a, dt, n, noise=None):
        """the states after steps 1 .. n: a list of (u, v, a)"""
        out = []
        for _ in range(n):
            u, v, a = self.step(u, v, a, dt, noise)
            out.append((u, v, a))
        return out

    def fold_step(self, u, v, a, dt, n):
        """(k, det_before, det_at): the first step k <= n whose force pass sees det F <= 0 at a cell quadrature point, the smallest
        det F of the pass before it and of that pass; k = 0 when no step folds"""
        before = np.inf
        for k in range(1, n + 1):
            du = dt * v + 0.5 * dt * dt * a
            F, jmin = self.force(u + du, with_det=True)
            if not jmin > 0:
                return k, before, jmin
            before = jmin
            an = self.minv * F
            u, v, a = u + du, v + 0.5 * dt * (a + an), an
        return 0, before, before

    # ---- stability
    def tangent(self, u):
        """x -> K_T(u) x on the free dofs (zero on constrained ones): mirror.Operator without its mass term"""
        op = Mi.Operator(self.mesh, u, mu=MU, nu=NU, rho=RHO, alpha1=0.0)
        free = ~self.constrained

        def apply(x):
            y = op(x * free)
            y[~free] = 0.0
            return y
        return apply

    def dense_pencil(self, u):
        """(K_ff, m_f, free): the dense tangent on the free dofs and their lumped masses"""
        apply = self.tangent(u)
        free = np.nonzero(~self.constrained)[0]
        K = np.zeros((len(free), len(free)))
        for j, d in enumerate(free):
            e = np.zeros(self.mesh.n)
            e[d] = 1.0
            K[:, j] = apply(e)[free]
        return 0.5 * (K + K.T), self.mass[free], free

    def lanczos(self, apply, steps=40):
        """the largest Ritz value of `steps` Lanczos steps for K phi = lambda M_L phi in the M_L inner product, from the device's
        start vector, without reorthogonalisation"""
        m = self.mass
        free = ~self.constrained
        steps = min(steps, int(free.sum()))
        q = hash_start(self.mesh.n, self.dim, self.constrained)
        q = q / np.sqrt(np.sum(m * q * q))
        qp, alpha, beta = None, [], []
        for j in range(steps):
            y = apply(q)
            alpha.append(float(q @ y))
            if j + 1 == steps:
                break
            w = self.minv * y - alpha[-1] * q
            if qp is not None:
                w -= beta[-1] * qp
            b = np.sqrt(np.sum(m * w * w))
            if not b > 0:
                break
            beta.append(float(b))
            qp, q = q, w / b
        beta = beta[:len(alpha) - 1]
        T = np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)
        return float(np.linalg.eigvalsh(T)[-1])


def lambda_max_dense(K, mf):
    """the largest eigenvalue of K phi = lambda diag(mf) phi by a dense symmetric eigh"""
    s = 1.0 / np.sqrt(mf)
    return float(np.linalg.eigvalsh(K * s[:, None] * s[None, :])[-1])


_refs, _dts = {}, {}


def reference(name):
    if name not in _refs:
        _refs[name] = Reference(name)
    return _refs[name]


def dt_half_crit(name):
    """1/2 dt_crit of the reference's own 40-step Lanczos at the initial state: the step of the comparisons"""
    if name not in _dts:
        R = reference(name)
        u, _, _ = R.initial()
        _dts[name] = 0.5 * 2.0 / np.sqrt(R.lanczos(R.tangent(u), 40))
    return _dts[name]
