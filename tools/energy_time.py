"""ms per mi_energy call beside ms per mi_assemble_residual on the same context, in one process.

HIP events (torch.cuda.Event on the default stream) around each call, 20 repetitions after 3 warm-ups, the median; both
calls end with a synchronisation of the context's stream and a read-back of their scalars, so the events bracket the whole
call as a caller sees it.  mi_assemble_residual is the residual-only pass of the same state: the energy pass is its forward
half plus a reduction.  Meshes: 59^3 Q2 ("fine_level" 0 and 1), 40^3 and 24^3 Q3 ("fine_level" 1, "point_pass_q3" 1).

    python tools/energy_time.py [--quick]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
CASES = [(2, 59, 0), (2, 59, 1), (3, 40, 1), (3, 24, 1)]
if "--quick" in sys.argv:
    CASES = [(2, 12, 0), (2, 12, 1), (3, 8, 1)]


def timed(fn, reps=20, warm=3):
    ms = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


for p, n, fine in CASES:
    G = M.Context(dim=3, degree=p, reps=(n, n, n), body_force=(0.3, -9.81, 1.0))
    if p == 3:
        G.set_tuning("point_pass_q3", 1)
    G.set_tuning("fine_level", fine)
    rng = np.random.default_rng(1234)
    G.set(M.V_U, 0.02 / (p * n) * rng.standard_normal(G.n) * (~G.constrained))
    G.set(M.V_V, rng.standard_normal(G.n))
    G.update_acceleration()
    G.assemble()
    e = G.energy()
    t_e, t_e_min = timed(G.energy)
    t_r, t_r_min = timed(G.assemble_residual)
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, fine_level=fine, energy_ms=round(t_e, 4),
                          energy_ms_min=round(t_e_min, 4), residual_ms=round(t_r, 4), residual_ms_min=round(t_r_min, 4),
                          strain=e["strain"], kinetic=e["kinetic"], body=e["body"])), flush=True)
    G.close()
