"""What an explicit step costs beside the implicit one: ms per step of explicit_run(200), one mi_assemble_residual (the yardstick
of the force pass) and one Newmark step on the same context, the stability limit dt_crit of explicit_stable_dt and the substeps
a time step of 0.005 needs at the safety factor 0.8.

Jobs (unit cube, boxes): 59^3 Q2 (the bench mesh) and 40^3 Q3, each with "fine_level" 0 and 1.  The context takes two Newmark steps
under the bench's traction, so the state is a loaded one.  HIP events (torch.cuda.Event on the default stream) around each call --
the whole call as a caller sees it --, five repetitions after one warm-up, the calls alternated within a repetition (residual,
Newmark step, explicit run; so drift of the clocks falls on all alike), the median (minimum, maximum) of each.  One JSON line per
job.  --job i runs job i alone (so that a script can give every job a time limit of its own), --quick takes small meshes,
--steps n the steps per explicit run, --point-pass-q3 sets "point_pass_q3" 1 on the Q3 matrix-free level (the force pass is then
mf_point_pass_q3 in one launch instead of the generic pass colour by colour).

--ab: instead of the above, the A/B of the force-only instances of the one-launch point passes: explicit_run(steps) under
"explicit_force_only" 1 and 0 alternated, seven pairs after one warm-up pair, the median of each form, the spread (max - min) of
each and the median of the pair differences.

    python tools/explicit_step_cost.py [--quick] [--job i] [--steps n] [--point-pass-q3] [--ab]
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import _pkg  # noqa: E402

M = _pkg()
JOBS = [(2, 59, 0), (2, 59, 1), (3, 40, 0), (3, 40, 1)]
if "--quick" in sys.argv:
    JOBS = [(2, 11, 0), (2, 11, 1), (3, 8, 0), (3, 8, 1)]
if "--job" in sys.argv:
    JOBS = [JOBS[int(sys.argv[sys.argv.index("--job") + 1])]]
STEPS = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 200
POINT_PASS_Q3 = "--point-pass-q3" in sys.argv
TRACTION = (0.0, -2e3, 0.0)
REPS, WARM = 5, 1
DT, SAFETY = 0.005, 0.8


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


def ab(G, p, n, fine_level, dt_crit):
    n_sub = max(1, math.ceil(DT / (SAFETY * dt_crit)))
    G.explicit_setup(DT / n_sub, init_acceleration=True)
    ms = {1: [], 0: []}
    for r in range(1 + 7):
        for key in (1, 0):
            G.set_tuning("explicit_force_only", key)
            t = event_ms(lambda: G.explicit_run(STEPS))
            if r >= 1:
                ms[key].append(t / STEPS)
    d = np.array(ms[0]) - np.array(ms[1])
    out = dict(ab="explicit_force_only", degree=p, cells_per_side=n, fine_level=fine_level, point_pass_q3=G.get_tuning("point_pass_q3_active"),
               n_dofs=G.n, pairs=7, steps_per_run=STEPS)
    for key, name in ((1, "force_only"), (0, "zero_vector")):
        out[name + "_step_ms"] = round(float(np.median(ms[key])), 5)
        out[name + "_spread_ms"] = round(float(np.max(ms[key]) - np.min(ms[key])), 5)
    out["zero_minus_force_only_ms"] = round(float(np.median(d)), 5)
    out["zero_minus_force_only_min_max_ms"] = [round(float(d.min()), 5), round(float(d.max()), 5)]
    G.close()
    return out


def job(p, n, fine_level):
    G = M.Context(dim=3, degree=p, reps=(n, n, n), lo=(0, 0, 0), hi=(1, 1, 1), mu=0.5e6, nu=0.4, rho=1000.0, delta_t=DT)
    G.set_tuning("cg_warm_start", 2)
    if fine_level:
        G.set_tuning("fine_level", 1)
        G.set_tuning("mf_diag_lag", 1)
        if p == 3 and POINT_PASS_Q3:
            G.set_tuning("point_pass_q3", 1)
    for k in range(2):
        step(G, k)
    lam, dt_crit = G.explicit_stable_dt()
    if "--ab" in sys.argv:
        return ab(G, p, n, fine_level, dt_crit)
    stable_ms = event_ms(G.explicit_stable_dt)
    n_sub = max(1, math.ceil(DT / (SAFETY * dt_crit)))
    G.explicit_setup(DT / n_sub, init_acceleration=False)  # continues from the Newmark state
    ms = dict(assemble_residual_ms=[], newmark_step_ms=[], explicit_run_ms=[])
    for r in range(WARM + REPS):
        t = [event_ms(G.assemble_residual), event_ms(lambda: step(G, 2 + r)), event_ms(lambda: G.explicit_run(STEPS))]
        if r >= WARM:
            for key, v in zip(ms, t):
                ms[key].append(v)
    out = dict(degree=p, cells_per_side=n, fine_level=fine_level, point_pass_q3=G.get_tuning("point_pass_q3_active"), n_dofs=G.n,
               repetitions=REPS, steps_per_run=STEPS, lambda_max=lam, dt_crit=dt_crit, substeps_per_dt=n_sub, safety=SAFETY, dt=DT,
               stable_dt_ms=round(stable_ms, 3))
    for key, v in ms.items():
        out[key] = round(float(np.median(v)), 4)
        out[key.replace("_ms", "_ms_min")] = round(float(np.min(v)), 4)
        out[key.replace("_ms", "_ms_max")] = round(float(np.max(v)), 4)
    out["explicit_step_ms"] = round(out["explicit_run_ms"] / STEPS, 5)
    out["explicit_ms_per_dt"] = round(out["explicit_step_ms"] * n_sub, 3)
    G.close()
    return out


for p, n, f in JOBS:
    print(json.dumps(job(p, n, f)), flush=True)
