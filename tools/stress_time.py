"""ms per mi_stress_field call beside mi_energy and mi_assemble_residual on the same context, in one process; and a child
mode for a kernel trace.

HIP events (torch.cuda.Event on the default stream) around each call, 20 repetitions after 3 warm-ups, the median (minimum):
the whole call as a caller sees it -- for mi_stress_field that includes the read-back of the three global arrays
(n_nodes x 8 doubles to pageable host memory), which dominates the kernels at 5 M DoFs.  The kernels alone:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/stress_time.py --child DEGREE CELLS_PER_SIDE

(a fresh process that builds the context, loads a state and calls mi_stress_field 3 + 20 times).  Meshes: 59^3 Q2
("fine_level" 0), 40^3 and 24^3 Q3 ("fine_level" 1, "point_pass_q3" 1), boxes, model 0.  The generic kernel on the same meshes:
MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_STRESS_GENERIC=1 (experiments build).

    python tools/stress_time.py [--quick]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
CASES = [(2, 59, 0), (3, 40, 1), (3, 24, 1)]
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
        s = G.stress_field()
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, max_von_mises=float(s[1].max()))), flush=True)
    G.close()
    sys.exit(0)

for p, n, fine in CASES:
    G = context(p, n, fine)
    G.update_acceleration()
    G.assemble()
    s = G.stress_field()
    t_s = timed(G.stress_field)
    t_e = timed(G.energy)
    t_r = timed(G.assemble_residual)
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, fine_level=fine, generic=os.environ.get("MI_STRESS_GENERIC", "0"),
                          stress_ms=t_s[0], stress_ms_min=t_s[1], energy_ms=t_e[0], energy_ms_min=t_e[1], residual_ms=t_r[0],
                          residual_ms_min=t_r[1], max_von_mises=float(s[1].max()), volume=float(s[2].sum()))), flush=True)
    G.close()
