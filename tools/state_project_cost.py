"""What mi_state_project and the consistent-mass product cost, beside a residual pass of the same context.

Jobs (unit cube, boxes): 60^3 -> 30^3 Q2 and 40^3 -> 20^3 Q3, both with sub = 2 (the exact nested pair).  The fine context carries a
smooth state in its six vectors; the coarse one receives its projection (Context.project_state_from).

Per job, one JSON line:
  project_ms        the whole call as a caller sees it, median (minimum) of 5 after a warm-up: the load pass (points, evaluation
                    on src, contraction, chunk by chunk), the diagonal, the Jacobi-PCG on six columns, one product for dst_sq, one
                    device copy of the six vectors
  its, res          the solve's iteration count and worst residual; n_points of the composite rule
  iteration_ms      one CG iteration of six columns on the FINE context -- the product (mass_apply_cells, eight colour launches),
                    the column dots and the two fused updates: the difference of two Context.mass_solve calls stopped after 12
                    and after 2 iterations, over 10 (uploads and read-backs are the same in both and cancel), median of 5
  product_bytes     what one six-column product must move at least: x read and y written once per column, the connectivity,
                    the cell vertices and the constraint mask once; iteration_gbs is that over iteration_ms, a LOWER bound of
                    what the product kernel reaches (the iteration holds the column algebra too)
  residual_ms       Context.assemble_residual of the fine context, the yardstick, median of 5
  its_small         the iteration counts of the same solve on 6^3 / 4^3 cells next to those of the fine context (its_fine)

The generic form of the product on 3D Q2 / Q3: the same tool on the experiments build with its hook,
    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_MASS_GENERIC=1 python tools/state_project_cost.py
(`form` in the output says which library and hook the line was made with).

The kernels alone:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/state_project_cost.py --child DEGREE FINE

    python tools/state_project_cost.py [--quick]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
JOBS = [(2, 60), (3, 40)]
if "--quick" in sys.argv:
    JOBS = [(2, 8), (3, 6)]
SIX = [M.V_U, M.V_U_OLD, M.V_V, M.V_V_OLD, M.V_A, M.V_A_OLD]


def context(p, n):
    return M.Context(dim=3, degree=p, reps=(n, n, n), lo=(0, 0, 0), hi=(1, 1, 1), mu=0.5e6, nu=0.4, rho=1000.0, delta_t=0.005)


def smooth_state(G):
    X = G.coords
    free = ~G.constrained
    out = []
    for k in range(6):
        f = np.stack([np.sin((k + 1) * X[:, 0] + c) * np.cos(2 * X[:, 1]) * (1 + X[:, 2]) for c in range(3)], axis=1).reshape(-1)
        out.append(1e-3 * f * free)
    return np.array(out)


def timed(fn, reps=5, warm=1):
    ms = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)


def job(p, n):
    F, Cc = context(p, n), context(p, n // 2)
    state = smooth_state(F)
    for k, v in zip(SIX, state):
        F.set(k, v)
    info = {}

    def project():
        info.update(Cc.project_state_from(F, sub=2))

    project_ms = timed(project)
    its_fine = F.mass_solve(state, masked=True)[1]
    short = timed(lambda: F.mass_solve(state, masked=True, max_it=2, check=False))
    longer = timed(lambda: F.mass_solve(state, masked=True, max_it=12, check=False))
    iteration_ms = round((longer[0] - short[0]) / 10.0, 4)
    residual_ms = timed(F.assemble_residual)
    npc = (p + 1) ** 3
    product_bytes = 6 * 2 * F.n * 8 + F.ncells * (npc * 4 + 24 * 8) + F.nnodes
    S = context(p, 6 if p == 2 else 4)
    its_small = S.mass_solve(smooth_state(S), masked=True)[1]
    form = "generic" if os.environ.get("MI_MASS_GENERIC", "0") not in ("", "0") and "_exp" in M.LIB_PATH else "sum-factorised"
    out = dict(form=form, degree=p, fine_cells=n, coarse_cells=n // 2, fine_dofs=F.n, coarse_dofs=Cc.n, project_ms=project_ms, its=info["its"],
               res=info["res"], n_points=info["n_points"], iteration_ms=iteration_ms, product_bytes=product_bytes,
               iteration_gbs=round(product_bytes / (iteration_ms * 1e6), 1) if iteration_ms > 0 else None,
               residual_ms=residual_ms, its_fine=its_fine, its_small=its_small)
    for G in (F, Cc, S):
        G.close()
    return out


def child(p, n):
    F, Cc = context(p, n), context(p, n // 2)
    for k, v in zip(SIX, smooth_state(F)):
        F.set(k, v)
    Cc.project_state_from(F, sub=2)
    F.assemble_residual()


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    else:
        for p, n in JOBS:
            print(json.dumps(job(p, n)), flush=True)
