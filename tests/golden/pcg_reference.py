"""Independent numpy reference of the preconditioned conjugate gradient iteration that mi_cg_solve and mi_linear_step run
(cg_run in dealii-adapter_amd/csrc/mi_ctx.cpp), written from the textbook and not from the cg_update_* kernels.

  pcg()               Hestenes-Stiefel PCG (Saad, Iterative Methods for Sparse Linear Systems, algorithm 9.1): every iterate
                      x_k, the recursive-residual norms ||r_k|| (k = 0 .. K), alpha_k and beta_k, over a generic dtype
  first_converged()   the stopping rule of nonlinear_elasticity.cc:1153-1191 as the library states it: the first k >= 0 with
                      ||r_k|| <= tau ||b|| (the linear model: ||r_k|| <= tol_abs)
  predicted_start()   the start vector of "cg_warm_start" 2 / 3: alpha h with alpha = h.b / h.Ah, h = h1 or 2 h1 - h0
  jacobi(), vcycle()  the two preconditioners: 1 / diag(A) and mg_reference.Reference.vcycle
  Problem             one case: mesh, state, mg_reference.Reference (whose A_assembled is the CG's operator), right-hand
                      sides and start vectors, and the cached runs of pcg() that the CPU and the GPU tests share
  sell_matrix_bytes() the size of the sliced-ELL value array of a mesh, which decides between the one-launch solver and
                      the three-launch one (SMALL_CG_MAX_MATRIX_BYTES)

Norms and dots run over all dofs, as on the device, which masks nothing: constrained rows are decoupled diagonal entries, and
right-hand sides and start vectors are zero there, so every iterate is.

Precision: every product runs in the dtype of the call (float64 or np.longdouble); in long double the matrix is multiplied
with np.add.at, as in mg_reference.py.  E_X / E_R below are the float64 run's distances from the long double run per
preconditioner and iteration, measured and asserted by tests/test_mirror_pcg.py; the GPU tolerances are computed from them.
"""
import functools
import math

import numpy as np

import mg_reference as R
import mirror as Mi

SMALL_CG_MAX_MATRIX_BYTES = 1 << 20  # dealii-adapter_amd/csrc/mi_internal.h
CG_BATCH = 16


# ------------------------------------------------------------------ the iteration
class Matrix:
    """a scipy matrix as a product in one dtype"""

    def __init__(self, A, dtype=np.float64):
        self.A, self.dtype, self.n = A.tocsr(), dtype, A.shape[0]
        if dtype != np.float64:
            coo = A.tocoo()
            self.rows, self.cols, self.vals = coo.row, coo.col, coo.data.astype(dtype)

    def __call__(self, x):
        if self.dtype == np.float64:
            return self.A @ x
        y = np.zeros(self.n, self.dtype)
        np.add.at(y, self.rows, self.vals * x[self.cols])
        return y

    def diagonal(self):
        return self.A.diagonal().astype(self.dtype)


def pcg(A, Minv, b, x0, K, dtype=np.float64):
    """K iterations of the preconditioned CG for A x = b from x0.  A, Minv: callables on vectors of `dtype`.
    Returns (xs, rn, alpha, beta): xs[k] = x_k and rn[k] = ||r_k||_2 of the recursively updated residual for k = 0 .. K,
    alpha[k] and beta[k] of iteration k + 1 (beta[k] turns p_k into p_k+1).  Stops early only where the recurrence ends
    (r_k = 0 or p.Ap <= 0); the lists are then shorter."""
    b = np.asarray(b).astype(dtype)
    x = np.asarray(x0).astype(dtype)
    r = b - A(x)
    xs, rn, alpha, beta = [x.copy()], [np.sqrt(r @ r)], [], []
    z = Minv(r)
    p = z.copy()
    rz = r @ z
    for _ in range(K):
        q = A(p)
        pq = p @ q
        if not pq > 0 or rn[-1] == 0:
            break
        a = rz / pq
        x = x + a * p
        r = r - a * q
        xs.append(x.copy())
        rn.append(np.sqrt(r @ r))
        z = Minv(r)
        rz_new = r @ z
        bt = rz_new / rz
        p = z + bt * p
        rz = rz_new
        alpha.append(a)
        beta.append(bt)
    return xs, np.array(rn), np.array(alpha), np.array(beta)


def first_converged(rn, tol_abs):
    """the reported iteration count: the first k >= 0 with ||r_k|| <= tol_abs; None if there is none among rn"""
    hit = np.nonzero(np.asarray(rn) <= tol_abs)[0]
    return int(hit[0]) if len(hit) else None


def distribute(x, constrained):
    """constraints.distribute (:1208): x[constrained] = 0"""
    y = np.array(x)
    y[constrained] = 0
    return y


def predicted_start(A, b, h1, h0=None):
    """alpha h, h = h1 (the same solve one step earlier) or 2 h1 - h0 (two histories), alpha = h.b / h.Ah: the multiple of h with the
    smallest energy-norm error; zero if h.Ah is not positive"""
    h = np.asarray(h1) if h0 is None else 2 * np.asarray(h1) - np.asarray(h0)
    hAh = h @ A(h)
    return (h @ b / hAh if hAh > 0 else 0.0) * h


def jacobi(A, dtype=np.float64):
    dinv = 1 / Matrix(A, dtype).diagonal()
    return lambda r: dinv * r


def vcycle(ref, lmax, dtype=np.float64, **kw):
    """kw: storage / product_matrices of mg_reference.Reference.vcycle (the fp32-stored preconditioner)"""
    return lambda r: ref.vcycle(r, lmax, dtype, **kw)


def margin(rn_k, tol_abs, e_r):
    """True where ||r_k|| is far enough from the tolerance for the test `||r_k|| <= tol` to be the same in every correct
    float64 run: outside [1 / (1 + g), 1 + g] tol with g = max(1e-6, 1e3 e_r)"""
    g = max(1e-6, 1e3 * e_r)
    q = rn_k / tol_abs
    return bool(q < 1 / (1 + g) or q > 1 + g)


# ------------------------------------------------------------------ which solver runs
def sell_nblk64(dim, p, reps):
    """sum of the slice lengths of the sliced-ELL matrix of one slab (mesh.sell_nblk64), from the node lattice alone: a row
    couples the nodes of the cells it lies in, a box of the lattice; rows are sorted into classes of one length and one
    x-width, every class is padded to slices of 64 rows, and a slice is as long as its rows"""
    nn = [p * r + 1 for r in reps[:dim]]
    width = []
    for d in range(dim):
        i = np.arange(nn[d])
        lo = np.where(i % p == 0, np.maximum(i - p, 0), (i // p) * p)
        hi = np.where(i % p == 0, np.minimum(i + p, nn[d] - 1), (i // p) * p + p)
        width.append(hi - lo + 1)
    grids = np.meshgrid(*width, indexing="ij")
    length = np.prod(grids, axis=0).reshape(-1)
    classes = {}
    for ln, wx in zip(length, grids[0].reshape(-1)):
        classes[(int(ln), int(wx))] = classes.get((int(ln), int(wx)), 0) + 1
    return sum(-(-cnt // 64) * ln for (ln, _), cnt in classes.items())


def sell_matrix_bytes(dim, p, reps):
    return sell_nblk64(dim, p, reps) * 64 * dim * dim * 8


# ------------------------------------------------------------------ the cases of tests/test_gpu_pcg_reference.py
# (here, so that tests/test_mirror_pcg.py measures the reference's own rounding on the same inputs without a GPU)
# meshes beside those of mg_reference.CASES, same description
MESHES = dict(R.CASES)
MESHES.update({
    "q2_432_distorted": dict(dim=3, p=2, reps=(4, 3, 2), kind="distorted", roles=R.ROLES_A),
    # the one-launch solver: the largest 2D and 3D Q2 meshes of their family under SMALL_CG_MAX_MATRIX_BYTES and the next above
    "2d_q2_small": dict(dim=2, p=2, reps=(39, 12), kind="distorted", roles=R.ROLES_2D),
    "2d_q2_above": dict(dim=2, p=2, reps=(40, 12), kind="distorted", roles=R.ROLES_2D),
    "q2_small": dict(dim=3, p=2, reps=(3, 2, 1), kind="graded", roles=R.ROLES_A),
    "q2_above": dict(dim=3, p=2, reps=(3, 2, 2), kind="graded", roles=R.ROLES_A),
})
SMALL = {"2d_q2_small": "2d_q2_above", "q2_small": "q2_above"}  # (under the limit: the next size, above it)
JACOBI_CASES = ["2d_q2_186", "q2_432_distorted", "2d_q2_small", "2d_q2_above", "q2_small", "q2_above", "q2_543_mf_fine",
                "q3_532_rule5", "q2_4412_3slabs_z", "q2_1244_2slabs_x", "q2_4416_induced"]
VCYCLE_CASES = ["q2_654", "q2_543_mf_fine", "q3_532_rule5", "2d_q2_186", "q2_4412_3slabs_z", "q2_1244_2slabs_x",
                "q2_4416_induced"]
CASES_OF = dict(jacobi=JACOBI_CASES, vcycle=VCYCLE_CASES)
# (right-hand side, start vector) of the runs that the CPU test measures and the GPU test repeats; the GPU test adds the
# assembly's own residual from x0 = 0, taken from the device (the mirror's assembly is a dense Python loop), under the same
# tolerances
INPUTS = [("smooth", "zero"), ("smooth", "random"), ("rough", "zero")]

K_VCYCLE = (1, 2, 3, 5, 8)
K_JACOBI = (1, 2, 3, 15, 16, 17, 32, 33)  # both sides of the polls after CG_BATCH and 2 CG_BATCH iterations
K_SMALL = (1, 2, 17, 33)
K_MAX = dict(jacobi=34, vcycle=14)  # how far the rounding tables reach: every converged run of the tables below ends earlier

# tau per (case, preconditioner): relative tolerances of the converged runs on the smooth right-hand side from x0 = 0, chosen
# on the CPU (tests/test_mirror_pcg.py asserts for each that no ||r_k|| / (tau ||b||), k <= its, lies within the margin).
# Jacobi: one that converges inside a batch, one on its % 16 == 0 and one on its % 16 == 1, by choosing tau between
# ||r_its|| and ||r_its-1|| of the reference (TAU_AT: the iteration count asked for; the tau follows from the run)
TAU_AT = dict(jacobi=(9, 16, 17), vcycle=(4, 7))
TAU = {
    ("2d_q2_186", "jacobi"): (0.18, 0.018, 0.012),
    ("q2_432_distorted", "jacobi"): (0.51, 0.097, 0.08),
    ("2d_q2_small", "jacobi"): (0.16, 0.018, 0.013),
    ("2d_q2_above", "jacobi"): (0.16, 0.018, 0.012),
    ("q2_small", "jacobi"): (0.33, 0.095, 0.07),
    ("q2_above", "jacobi"): (0.51, 0.16, 0.13),
    ("q2_543_mf_fine", "jacobi"): (0.56, 0.16, 0.13),
    ("q3_532_rule5", "jacobi"): (0.69, 0.24, 0.21),
    ("q2_4412_3slabs_z", "jacobi"): (0.33, 0.064, 0.049),
    ("q2_1244_2slabs_x", "jacobi"): (0.31, 0.05, 0.041),
    ("q2_4416_induced", "jacobi"): (0.31, 0.049, 0.038),
    ("q2_654", "vcycle"): (0.00032, 2.6e-07),
    ("q2_543_mf_fine", "vcycle"): (0.036, 0.0018),
    ("q3_532_rule5", "vcycle"): (0.015, 0.00025),
    ("2d_q2_186", "vcycle"): (7.4e-05, 2.1e-08),
    ("q2_4412_3slabs_z", "vcycle"): (0.00029, 1.7e-07),
    ("q2_1244_2slabs_x", "vcycle"): (0.00018, 9.8e-08),
    ("q2_4416_induced", "vcycle"): (0.00031, 1.5e-07),
}


def geometric_tau(rn, bnorm, its, rounded=True):
    """a tolerance that the run rn meets first at iteration `its`: the geometric mean of ||r_its|| and the smallest residual
    before it, over ||b||; rounded to two digits for the committed table (so that the figure can be read and written down),
    unrounded where a test takes it from a run of its own (two residuals may lie closer than two digits tell apart)"""
    lo, hi = rn[its], rn[:its].min()
    assert lo < hi, "the residual norm does not fall below its earlier values at iteration %d" % its
    t = math.sqrt(lo * hi) / bnorm
    return float("%.1e" % t) if rounded else float(t)


class Problem:
    """one case on the CPU: mesh, state, reference hierarchy, inputs, and the cached runs"""

    def __init__(self, name):
        self.name = name
        c = MESHES[name]
        lo, hi, perturb = R.geometry(c["kind"], c["dim"], c["reps"], seed=sum(c["reps"]))
        self.lo, self.hi, self.perturb = lo, hi, perturb
        self.m = Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, c["roles"], perturb=perturb)
        self.u, self.du = R.case_state(self.m, seed=len(name))
        self.free = ~self.m.constrained
        self._ref = self._A = self._lmax = None
        self._runs = {}

    @property
    def ref(self):
        """the hierarchy (cases that run the V-cycle)"""
        if self._ref is None:
            c = MESHES[self.name]
            self._ref = R.Reference(self.m, self.u + self.du, coarsest=c.get("coarsest", 4), dense=c.get("dense", 1),
                                    nq0=c.get("nq0"), fold0=c.get("fold0", False), alpha1=R.A1)
            self._A = self._ref.A_assembled
        return self._ref

    @property
    def A(self):
        """the CG's operator: the tangent under the assembly's rule, whatever the smoother's product integrates with"""
        if self._A is None:
            self._A = R.operator_matrix(Mi.Operator(self.m, self.u + self.du, alpha1=R.A1))
        return self._A

    def lmax_cpu(self):
        """1.15 lambda_true per smoothed level: what stands in for the device's lmax wherever no device is at hand"""
        if self._lmax is None:
            self._lmax = tuple(self.ref.true_lmax())
        return self._lmax

    def rhs(self, what):
        """"smooth": a smooth field with random coefficients; "rough": white noise; both zero on constrained dofs and scaled to
        the size of a residual of the assembly (1e2)"""
        m, rng = self.m, np.random.default_rng(11 + len(self.name))
        if what == "rough":
            b = rng.standard_normal(m.n)
        else:
            s = (m.coords - m.coords.min(0)) / np.ptp(m.coords, axis=0).max()
            b = np.zeros((m.nnodes, m.dim))
            for _ in range(4):
                k, ph, amp = rng.uniform(0.5, 3.0, m.dim), rng.uniform(0, 2 * np.pi), rng.standard_normal(m.dim)
                b += np.sin(s @ k * np.pi + ph)[:, None] * amp
            b = b.reshape(-1)
        return 1e2 * b / np.abs(b).max() * self.free

    def x0(self, what):
        """"zero", or "random": white noise on the free dofs of the size of a solution (so that A x0 weighs as b does)"""
        if what == "zero":
            return np.zeros(self.m.n)
        x = np.random.default_rng(5 + len(self.name)).standard_normal(self.m.n) * self.free
        return x * (np.abs(self.rhs("smooth")).max() / np.abs(self.A @ x).max())

    def preconditioner(self, pre, lmax=None, dtype=np.float64):
        if pre == "jacobi":
            return jacobi(self.A, dtype)
        return vcycle(self.ref, tuple(lmax), dtype)

    def run(self, pre, b, x0, K, lmax=None, dtype=np.float64, key=None):
        """pcg() on this case, cached under `key` (+ preconditioner, lmax, K, dtype) when one is given"""
        k = None if key is None else (key, pre, None if lmax is None else tuple(lmax), K, dtype)
        if k is None or k not in self._runs:
            out = pcg(Matrix(self.A, dtype), self.preconditioner(pre, lmax, dtype), b, x0, K, dtype)
            if k is None:
                return out
            self._runs[k] = out
        return self._runs[k]


@functools.lru_cache(maxsize=None)
def problem(name):
    return Problem(name)


# ------------------------------------------------------------------ the reference's own rounding
# E_X[pre][k], E_R[pre][k]: worst max |x_k - x_k^ld| / max |x_k^ld| and | ||r_k|| - ||r_k||^ld | / ||r_k||^ld of the float64 run
# against the long double run over CASES_OF x INPUTS: the running maximum over k of the measurement, rounded up in the second
# digit as mg_reference.E_REF is (a later iteration is never held to less than an earlier one); measured and asserted by
# tests/test_mirror_pcg.py::test_reference_rounding_is_the_committed_table (which prints the table to paste here).
# V-cycle runs take 1.15 lambda_true for the device's lmax.
E_X = {
    "jacobi": [
        1.0e-16, 7.4e-16, 1.1e-15, 1.1e-15, 1.8e-15, 2.7e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15,
        3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15, 3.4e-15,
        5.0e-15, 1.2e-14, 2.1e-14, 4.4e-14, 8.7e-14, 1.9e-13, 2.9e-13, 6.5e-13, 1.8e-12, 3.6e-12,
        7.2e-12, 2.2e-11, 5.3e-11, 1.6e-10, 3.6e-10,
    ],
    "vcycle": [
        1.0e-16, 1.3e-15, 2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15,
        2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15, 2.0e-15,
    ],
}
E_R = {
    "jacobi": [
        1.9e-16, 6.3e-16, 1.5e-15, 1.5e-15, 1.5e-15, 1.5e-15, 1.7e-15, 1.7e-15, 1.7e-15, 1.7e-15,
        2.2e-15, 2.2e-15, 2.2e-15, 3.1e-15, 3.1e-15, 3.1e-15, 4.8e-15, 1.2e-13, 1.8e-13, 1.8e-13,
        7.7e-13, 7.7e-13, 9.3e-13, 1.2e-11, 1.4e-11, 1.3e-10, 1.3e-10, 3.2e-10, 7.9e-10, 6.0e-09,
        6.0e-09, 4.6e-08, 4.6e-08, 2.8e-07, 6.9e-07,
    ],
    "vcycle": [
        1.9e-16, 1.6e-15, 3.3e-15, 8.4e-15, 8.4e-15, 1.3e-14, 1.5e-14, 1.7e-14, 3.6e-14, 9.0e-14,
        1.6e-13, 2.1e-13, 2.1e-13, 2.1e-13, 2.1e-13,
    ],
}


def measure_rounding(name, pre, what, start):
    """(E_x(k), E_r(k)) for k = 0 .. K_MAX of one run: float64 against long double"""
    pr = problem(name)
    lmax = pr.lmax_cpu() if pre == "vcycle" else None
    b, x0, K = pr.rhs(what), pr.x0(start), K_MAX[pre]
    xs, rn, _, _ = pr.run(pre, b, x0, K, lmax, key=(what, start))
    xl, rl, _, _ = pr.run(pre, b, x0, K, lmax, np.longdouble)
    assert len(rn) == len(rl) == K + 1
    ex = [float(np.abs(xs[k] - xl[k]).max() / max(np.abs(xl[k]).max(), np.finfo(float).tiny)) for k in range(K + 1)]
    er = [float(abs(rn[k] - rl[k]) / rl[k]) for k in range(K + 1)]
    return np.array(ex), np.array(er)


def _tol(table, k):
    return min(1e-6, 10.0 ** math.ceil(math.log10(64 * max(table[k], 1e-16))))


def tol_x(pre, k):
    """min(1e-6, 64 x the reference's own rounding at iteration k, rounded up to a power of ten)"""
    return _tol(E_X[pre], k)


def tol_r(pre, k):
    return _tol(E_R[pre], k)
