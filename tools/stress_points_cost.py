"""What a stress gauge costs beside a time step: mi_evaluate_stress at 1,000 probes (raw and recovered), the same points through
mi_evaluate_points, one mi_stress_field under "stress_projection" 0 and 1 (with the solve's iteration count), and one Newmark
step of the same context.

Jobs (unit cube, boxes): 59^3 Q2 (the bench mesh) and 40^3 Q3.  The context takes two Newmark steps under the bench's traction, so
the stress is that of a loaded state.  HIP events (torch.cuda.Event on the default stream) around each call -- the whole call as a
caller sees it, upload of the points and read-back of the answers included --, five repetitions after one warm-up, the calls
alternated within a repetition (raw, recovered, points, field key 0, field key 1, step; so drift of the clocks falls on all
alike), the median (minimum) of each.  One JSON line per job.

    python tools/stress_points_cost.py [--quick]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
JOBS = [(2, 59), (3, 40)]
if "--quick" in sys.argv:
    JOBS = [(2, 11), (3, 8)]
TRACTION = (0.0, -2e3, 0.0)
REPS, WARM = 5, 1


def step(G, k):
    G.set_interface_traction(tuple(min(1.0, (k + 1) / 10.0) * t for t in TRACTION))
    G.newmark_step(tol_lin=1e-6, max_it_mult=1.0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def job(p, n):
    G = M.Context(dim=3, degree=p, reps=(n, n, n), lo=(0, 0, 0), hi=(1, 1, 1), mu=0.5e6, nu=0.4, rho=1000.0, delta_t=0.005)
    G.set_tuning("cg_warm_start", 2)
    for k in range(2):
        step(G, k)
    pts = np.random.default_rng(1).uniform(0.0, 1.0, (1000, 3))
    its = []

    def field(key):
        G.set_tuning("stress_projection", key)
        G.stress_field()
        if key:
            its.append(G.get_tuning("stress_projection_its"))
        G.set_tuning("stress_projection", 0)

    calls = [("stress_raw_ms", lambda: G.evaluate_stress(pts, kind=M.STRESS_AT_RAW)),
             ("stress_recovered_ms", lambda: G.evaluate_stress(pts, kind=M.STRESS_AT_RECOVERED)),
             ("stress_raw_principal_ms", lambda: G.evaluate_stress(pts, kind=M.STRESS_AT_RAW, principal=True, directions=True)),
             ("points_ms", lambda: G.evaluate(M.V_U, pts)),
             ("points_gradients_ms", lambda: G.evaluate(M.V_U, pts, gradients=True)),
             ("stress_field_lumped_ms", lambda: field(0)),
             ("stress_field_consistent_ms", lambda: field(1))]
    ms = {k: [] for k, _ in calls}
    ms["newmark_step_ms"] = []
    for r in range(WARM + REPS):
        for k, fn in calls:
            t = event_ms(fn)
            if r >= WARM:
                ms[k].append(t)
        t = event_ms(lambda: step(G, 2 + r))
        if r >= WARM:
            ms["newmark_step_ms"].append(t)
    out = dict(degree=p, cells_per_side=n, n_dofs=G.n, probes=len(pts), repetitions=REPS,
               stress_projection_its=sorted(set(its)))
    for k, v in ms.items():
        out[k] = round(float(np.median(v)), 4)
        out[k.replace("_ms", "_ms_min")] = round(float(np.min(v)), 4)
    G.close()
    return out


for p, n in JOBS:
    print(json.dumps(job(p, n)), flush=True)
