"""Numpy reference of the linear model's multigrid V-cycle (tuning key "linear_precond" 1): the cycle, the transfers and the
Chebyshev smoother of mg_reference.py over levels that carry the LINEAR stepping matrix

  A_l = M_l + theta^2 dt^2 K_l  after MatrixTools::apply_boundary_values with zero values,

each the dense mirror.Linear of its own mesh: the fine mesh as given, and the unperturbed Q1 boxes that
mg_reference.hierarchy() lists.  D_l = the dim x dim node blocks of A_l.  No state is transferred: A is constant.
vcycle(), lambda_true() and true_lmax() are those of mg_reference.Reference.
"""
import numpy as np
import scipy.sparse as sp

import mg_reference as R
import mirror as Mi

DT, THETA = 0.02, 0.5  # every case: four times the shipped time step, where the Jacobi count has grown and the cycle's has not
# the reference's own rounding: worst relmax between the float64 and the long double cycle over CASES (random right-hand side),
# measured and asserted by tests/test_mirror_linear_multigrid.py: 3.19e-15 on q3_532 (distorted Q3 cells), 3.5e-16 .. 7.3e-16 on
# the other five.  Rounded up with room for another CPU's summation order in numpy's float64 products (the figure of
# mg_reference.E_REF was seen to move by a third between two machines).  The tolerance of the GPU tests rests on it.
E_LIN = 5.0e-15


class LinearReference(R.Reference):
    """The hierarchy of one linear problem.  mesh: the fine Mi.Mesh; body: the body force of the fine level's Mi.Linear (kept as
    .linear for the step tests; no level matrix depends on it)."""

    def __init__(self, mesh, dt=DT, theta=THETA, coarsest=4, dense=1, body=None, **material):
        m = mesh
        dim = self.dim = m.dim
        self.shape = R.hierarchy(dim, m.p, m.reps, coarsest, dense)
        self.meshes, self.A, self.D, self.T = [m], [], [], []
        for l, lv in enumerate(self.shape):
            if l:
                mf = self.meshes[-1]
                mc = Mi.Mesh(dim, 1, lv["reps"], m.lo, m.hi, m.roles)
                self.T.append(R.Transfer(dim, mf.nn, mc.nn, mf.constrained, mc.constrained))
                self.meshes.append(mc)
            lin = Mi.Linear(self.meshes[l], body=(body if body is not None and l == 0 else (0.0,) * dim), dt=dt, theta=theta,
                            **material)
            if l == 0:
                self.linear = lin
            A = sp.csr_matrix(lin.system_matrix())
            A.eliminate_zeros()
            A.sort_indices()
            self.A.append(A)
            self.D.append(R.node_blocks(A, dim))
        self.A_assembled = self.A[0]
        self._cache = {}


# ------------------------------------------------------------------ the cases of tests/test_gpu_linear_multigrid.py
# (here, so that tests/test_mirror_linear_multigrid.py measures the reference's own rounding on the same inputs without a GPU)
CASES = {
    "q3_532": dict(dim=3, p=3, reps=(5, 3, 2), kind="distorted", roles=R.ROLES_A),  # 3 levels, exact coarsest
    "q3_212": dict(dim=3, p=3, reps=(2, 1, 2), kind="distorted", roles=R.ROLES_A),  # 2 levels
    "q3_432": dict(dim=3, p=3, reps=(4, 3, 2), kind="graded", roles=R.ROLES_B),
    "q2_644": dict(dim=3, p=2, reps=(6, 4, 4), kind="graded", roles=R.ROLES_A),
    "q1_987": dict(dim=3, p=1, reps=(9, 8, 7), kind="cube", roles=R.ROLES_B),
    "2d_q2_186": dict(dim=2, p=2, reps=(18, 6), kind="cube", roles=R.ROLES_2D),  # 5 levels, smoothed coarse levels
}
BODY = (0.3, -9.81, 2.0)

_refs = {}


def case_geometry(name):
    c = CASES[name]
    return R.geometry(c["kind"], c["dim"], c["reps"], seed=sum(c["reps"]))


def reference(name):
    """the case's LinearReference (default material, theta = 0.5, dt = 0.02; the fine Mi.Linear with the body force BODY),
    built once per process: a mirror build takes seconds"""
    if name not in _refs:
        c = CASES[name]
        lo, hi, perturb = case_geometry(name)
        m = Mi.Mesh(c["dim"], c["p"], c["reps"], lo, hi, c["roles"], perturb=perturb)
        _refs[name] = LinearReference(m, body=BODY[:c["dim"]])
    return _refs[name]
