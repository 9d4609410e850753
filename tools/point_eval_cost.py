"""What mi_state_transfer and mi_evaluate_points cost beside a time step, in one process; and a child mode for a kernel trace.

Jobs (unit cube, boxes): 30^3 Q2 -> 59^3 Q2 (the bench mesh) and 20^3 Q3 -> 40^3 Q3.  The coarse context takes two Newmark steps under
the bench's traction, the fine one receives its state (Context.transfer_state_from), 1,000 random probes are evaluated on it
(six vectors, values only / with gradients), and it takes Newmark steps of its own, timed the same way.

HIP events (torch.cuda.Event on the default stream) around each call, 10 repetitions after 2 warm-ups, the median (minimum): the
whole call as a caller sees it.  A transfer is field_at_points over dst's nodes, finish_sum, one device copy of the six vectors and
six zero_constrained; it reads back one scalar.  An evaluation uploads the points and reads the answers back.  The kernels alone:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/point_eval_cost.py --child DEGREE COARSE FINE

Bytes of a transfer, as the kernel must move them at least: dst's node coordinates read, src's six vectors read once, the six
values and the cell id of every dst node written.  `transfer_gbs` is that over the call's median time: a lower bound of what
field_at_points achieves (the call holds the copy and the masks too; the trace separates them).

    python tools/point_eval_cost.py [--quick]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
JOBS = [(2, 30, 59), (3, 20, 40)]
if "--quick" in sys.argv:
    JOBS = [(2, 6, 11), (3, 4, 8)]
TRACTION = (0.0, -2e3, 0.0)
SIX = [M.V_U, M.V_U_OLD, M.V_V, M.V_V_OLD, M.V_A, M.V_A_OLD]


def context(p, n):
    G = M.Context(dim=3, degree=p, reps=(n, n, n), lo=(0, 0, 0), hi=(1, 1, 1), mu=0.5e6, nu=0.4, rho=1000.0, delta_t=0.005)
    G.set_tuning("cg_warm_start", 2)
    return G


def step(G, k):
    G.set_interface_traction(tuple(min(1.0, (k + 1) / 10.0) * t for t in TRACTION))
    G.newmark_step(tol_lin=1e-6, max_it_mult=1.0)


def timed(fn, reps=10, warm=2):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def job(p, coarse, fine, child=False):
    S, D = context(p, coarse), context(p, fine)
    for k in range(2):
        step(S, k)
    if child:
        for _ in range(12):
            D.transfer_state_from(S)
        pts = np.random.default_rng(1).uniform(0.0, 1.0, (1000, 3))
        for _ in range(12):
            D.evaluate(SIX, pts)
        return dict(degree=p, coarse=coarse, fine=fine, n_dofs=D.n)
    t_x = timed(lambda i: D.transfer_state_from(S))
    err = float(np.abs(D.evaluate(M.V_U, S.coords)[0].reshape(-1) - S.get(M.V_U)).max() / np.abs(S.get(M.V_U)).max())
    pts = np.random.default_rng(1).uniform(0.0, 1.0, (1000, 3))
    t_p = timed(lambda i: D.evaluate(SIX, pts))
    t_g = timed(lambda i: D.evaluate(SIX, pts, gradients=True))
    t_s = timed(lambda i: step(D, 2 + i), reps=5, warm=2)
    nbytes = 8 * (D.nnodes * 3 + 6 * S.n + 6 * D.n + D.nnodes)
    out = dict(degree=p, coarse_cells_per_side=coarse, fine_cells_per_side=fine, src_dofs=S.n, dst_dofs=D.n, transfer_ms=t_x[0],
               transfer_ms_min=t_x[1], transfer_bytes=nbytes, transfer_gbs=round(nbytes / t_x[0] / 1e6, 1), probes=1000,
               probes_ms=t_p[0], probes_ms_min=t_p[1], probes_gradients_ms=t_g[0], probes_gradients_ms_min=t_g[1],
               newmark_step_ms=t_s[0], newmark_step_ms_min=t_s[1], dst_field_at_src_nodes_relmax=err)
    S.close()
    D.close()
    return out


if "--child" in sys.argv:
    k = sys.argv.index("--child")
    print(json.dumps(job(int(sys.argv[k + 1]), int(sys.argv[k + 2]), int(sys.argv[k + 3]), child=True)), flush=True)
    sys.exit(0)

for p, coarse, fine in JOBS:
    print(json.dumps(job(p, coarse, fine)), flush=True)
