"""3D Q3 blocks on the matrix-free fine level, both forms of its assembly in one process, steps alternated: ms per Newmark
step, Newton and CG iterations.

  python tools/q3_point_pass_steps.py [--sizes 24x12x5,24x24x24,40x40x40] [--steps 6] [--keys 0,1]
                                      [--smoother-points 5] [--out FILE]

For every size two contexts of the same block (the reference's defaults: clamped at x = 0, traction on the other faces,
multigrid-PCG above 75 k dofs, the executable's warm start, "fine_level" 1 with "mf_diag_lag" 1 as the executable sets them)
run side by side: "point_pass_q3" 0 (the generic element kernel's residual pass colour by colour, then mf_records_q3) and
"point_pass_q3" 1 (records and residual in one launch of mf_point_pass_q3, then residual_gather).  Step k of one context is
followed by step k of the other, so both see the same state of the machine.  The first step is a warm-up; the others are
timed (wall clock around mi_newmark_step, which returns after the step's last synchronisation).  Printed per size and key,
one JSON line per size: the ms of every timed step, median and mean, Newton iterations and CG iterations per solve of every
timed step; whether the iteration counts of the two keys are identical, and whether EVERY timed step of key 1 was faster
than EVERY timed step of key 0.  --keys 1 runs the new form alone (a profiler run of its steps).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench import _pkg  # noqa: E402

M = _pkg()


def run(reps, steps, keys=(0, 1), points=5):
    ctx = {}
    for key in keys:
        G = M.Context(dim=3, degree=3, reps=reps, hi=tuple(0.1 * r for r in reps))
        G.set_tuning("cg_warm_start", 2)
        G.set_tuning("fine_level", 1)
        G.set_tuning("mf_diag_lag", 1)
        G.set_tuning("smoother_quadrature_q3", points)
        G.set_tuning("point_pass_q3", key)
        if G.get_tuning("point_pass_q3_active") != key:
            raise RuntimeError("point_pass_q3 %d: the assembly would not run the form that was set" % key)
        ctx[key] = G
    rec = {key: dict(ms=[], newton=[], cg=[]) for key in ctx}
    for s in range(steps):
        for key, G in ctx.items():
            G.set_interface_traction((0.0, -1e3 * min(1.0, (s + 1) / 4.0), 0.0))
            t0 = time.perf_counter()
            rc, info = G.newmark_step(tol_lin=1e-6, max_it_mult=1.0)
            dt = 1e3 * (time.perf_counter() - t0)
            if rc != 0 or info.converged != 1:
                raise RuntimeError("step %d of point_pass_q3 %d: rc %d" % (s, key, rc))
            if s == 0:
                continue
            rec[key]["ms"].append(dt)
            rec[key]["newton"].append(info.newton_iterations)
            rec[key]["cg"].append(list(info.lin_its)[:info.newton_iterations])
    n = next(iter(ctx.values())).n
    for G in ctx.values():
        G.close()
    out = dict(reps=list(reps), dofs=n, timed_steps=steps - 1, smoother_points=points)
    for key, r in rec.items():
        out["point_pass_q3_%d" % key] = dict(ms_median=round(statistics.median(r["ms"]), 2), ms_mean=round(statistics.mean(r["ms"]), 2),
                                             ms=[round(x, 2) for x in r["ms"]], newton=r["newton"], cg_per_solve=r["cg"])
    if 0 in rec and 1 in rec:
        a, b = out["point_pass_q3_0"], out["point_pass_q3_1"]
        out["ratio_key0_over_key1"] = round(a["ms_median"] / b["ms_median"], 3)
        out["same_iterations"] = a["newton"] == b["newton"] and a["cg_per_solve"] == b["cg_per_solve"]
        out["every_key1_step_faster"] = max(b["ms"]) < min(a["ms"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="24x12x5,24x24x24,40x40x40")
    ap.add_argument("--steps", type=int, default=6, help="steps per key, the first one untimed (6: five timed)")
    ap.add_argument("--keys", default="0,1", help="values of \"point_pass_q3\" to run")
    ap.add_argument("--smoother-points", type=int, default=5, help="rule of the level's smoother: 5 (125 points), 4 (64 points)")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    lines = []
    for sz in a.sizes.split(","):
        reps = tuple(int(x) for x in sz.split("x"))
        r = run(reps, max(2, a.steps), tuple(int(x) for x in a.keys.split(",")), a.smoother_points)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
