"""ms per mi_reactions call (models 0 and 1) beside mi_assemble_residual on the same context, in one process; and a child mode
for a kernel trace.

HIP events (torch.cuda.Event on the default stream) around each call, 20 repetitions after 3 warm-ups, the median (minimum): the
whole call as a caller sees it.  mi_reactions is called without the nodal arrays (the struct alone: one read-back of 35 doubles),
and with `forces` (n_dofs doubles to pageable host memory).  The kernels alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/reactions_time.py --child DEGREE CELLS_PER_SIDE

(a fresh process that builds the context, loads a state and calls mi_reactions(0), mi_reactions(1) and mi_assemble_residual
3 + 20 times each).  Meshes: 59^3 Q2 ("fine_level" 0) and 40^3 Q3 ("fine_level" 1, "point_pass_q3" 1), boxes.  The generic kernel
on the same meshes: MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_REACTIONS_GENERIC=1 (experiments build).

    python tools/reactions_time.py [--quick]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
CASES = [(2, 59, 0), (3, 40, 1)]
if "--quick" in sys.argv:
    CASES = [(2, 12, 0), (3, 8, 1)]


def context(p, n, fine):
    G = M.Context(dim=3, degree=p, reps=(n, n, n), body_force=(0.3, -9.81, 1.0))
    if p == 3:
        G.set_tuning("point_pass_q3", 1)
    G.set_tuning("fine_level", fine)
    rng = np.random.default_rng(1234)
    G.set(M.V_U, 0.02 / (p * n) * rng.standard_normal(G.n) * (~G.constrained))
    G.set(M.V_V, rng.standard_normal(G.n))
    G.set(M.V_V_OLD, rng.standard_normal(G.n))
    G.set(M.V_A, 3.0 * rng.standard_normal(G.n))
    G.set_interface_traction((0.0, -1e3, 0.0))
    G.assemble()
    return G


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
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


if "--child" in sys.argv:
    k = sys.argv.index("--child")
    p, n = int(sys.argv[k + 1]), int(sys.argv[k + 2])
    G = context(p, n, 0 if p == 2 else 1)
    for _ in range(23):
        r0 = G.reactions(M.STRESS_NEOHOOKE, forces=False)
    for _ in range(23):
        r1 = G.reactions(M.STRESS_LINEAR, forces=False)
    for _ in range(23):
        G.assemble_residual()
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, reaction=list(r0["reaction"]), reaction_linear=list(r1["reaction"]))),
          flush=True)
    G.close()
    sys.exit(0)

for p, n, fine in CASES:
    G = context(p, n, fine)
    r = G.reactions(forces=False)
    t0 = timed(lambda: G.reactions(M.STRESS_NEOHOOKE, forces=False))
    t1 = timed(lambda: G.reactions(M.STRESS_LINEAR, forces=False))
    tf = timed(lambda: G.reactions(M.STRESS_NEOHOOKE, forces=True))
    tr = timed(G.assemble_residual)
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, fine_level=fine, generic=os.environ.get("MI_REACTIONS_GENERIC", "0"),
                          reactions_ms=t0[0], reactions_ms_min=t0[1], reactions_linear_ms=t1[0], reactions_linear_ms_min=t1[1],
                          reactions_with_forces_ms=tf[0], reactions_with_forces_ms_min=tf[1], residual_ms=tr[0], residual_ms_min=tr[1],
                          reaction=list(r["reaction"]), internal_abs=r["internal_abs"])), flush=True)
    G.close()
