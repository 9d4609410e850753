"""ms per mi_stress_error call, with and without the per-cell arrays, beside mi_stress_field on the same context, in one process;
and a child mode for a kernel trace.

HIP events (torch.cuda.Event on the default stream) around each call, 20 repetitions after 3 warm-ups, the median (minimum):
the whole call as a caller sees it.  mi_stress_error reads back five scalars and, where wanted, two doubles per cell;
mi_stress_field reads back eight doubles per node.  The kernels alone:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/stress_error_time.py --child DEGREE CELLS_PER_SIDE

(a fresh process that builds the context, loads a state and calls mi_stress_error 3 + 20 times; pass 1 of every call is
mi_stress_field's kernels, so one trace holds both).  Meshes: 59^3 Q2 ("fine_level" 0), 40^3 and 24^3 Q3 ("fine_level" 1,
"point_pass_q3" 1), boxes, model 0.  The generic kernel of pass 2 on the same meshes:
MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_STRESS_ERROR_GENERIC=1 (experiments build).

    python tools/stress_error_time.py [--quick]
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
        r = G.stress_error(cells=False)
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, error=r["error"], norm=r["norm"], relative=r["relative"])), flush=True)
    G.close()
    sys.exit(0)

for p, n, fine in CASES:
    G = context(p, n, fine)
    r = G.stress_error()
    t_a = timed(G.stress_error)
    t_s = timed(lambda: G.stress_error(cells=False))
    t_f = timed(G.stress_field)
    print(json.dumps(dict(degree=p, cells_per_side=n, n_dofs=G.n, n_cells=G.ncells, fine_level=fine,
                          generic=os.environ.get("MI_STRESS_ERROR_GENERIC", "0"), stress_error_ms=t_a[0], stress_error_ms_min=t_a[1],
                          stress_error_scalars_ms=t_s[0], stress_error_scalars_ms_min=t_s[1], stress_field_ms=t_f[0],
                          stress_field_ms_min=t_f[1], error=r["error"], norm=r["norm"], relative=r["relative"],
                          max_cell=r["max_cell"])), flush=True)
    G.close()
