"""Linear model: Jacobi-PCG against multigrid-PCG ("linear_precond" 0 | 1) in one process, steps alternated.

  python tools/linear_precond_steps.py [--cases q3:24x12x5,q3:24x24x24,q3:40x40x40,q1:40x40x40] [--dts 0.005,0.02]
                                       [--steps 6] [--out FILE]

For every case and time step two contexts of the same block (clamped at x = 0, interface on the other faces, theta = 0.5, the
shipped material) are set up side by side: "linear_precond" 0 and 1.  q3: 3D Q3 cells with "linear_operator" 1 (matrix-free
operators); q1: 3D Q1 cells, assembled (BASELINE configuration 2).  Step k of one context is followed by step k of the other
with the same random interface load, so both see the same state of the machine.  The first step is a warm-up; the others are
timed (wall clock around mi_linear_step, which returns after the step's last synchronisation; PCG to the executable's absolute
1e-10).  Printed per case, time step and preconditioner: set-up time (mi_linear_setup, wall clock), median and every ms per
step, CG iterations per step; the ratio Jacobi / multigrid of the medians, and whether EVERY timed multigrid step was faster
than EVERY timed Jacobi step (or the other way round).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench import _pkg  # noqa: E402

M = _pkg()
THETA = 0.5
NAMES = {0: "jacobi", 1: "multigrid"}


def run(element, reps, dt, steps):
    degree = dict(q3=3, q1=1)[element]
    ctx, out = {}, dict(element=element, reps=list(reps), delta_t=dt)
    for pre in (0, 1):
        G = M.Context(dim=3, degree=degree, reps=reps, hi=tuple(0.1 * r for r in reps), delta_t=dt)
        if degree == 3:
            G.set_tuning("linear_operator", 1)
        G.set_tuning("linear_precond", pre)
        t0 = time.perf_counter()
        G.linear_setup(THETA)
        out[NAMES[pre]] = dict(setup_s=round(time.perf_counter() - t0, 3))
        if G.get_tuning("linear_precond_active") != pre or G.get_tuning("linear_operator_active") != int(degree == 3):
            raise RuntimeError("the set-up did not run what was set")
        if pre:
            out[NAMES[pre]]["levels"] = [G.linear_mg_level_describe(l)["n_dofs"] for l in range(G.linear_mg_n_levels())]
        ctx[pre] = G
    out["dofs"], out["timed_steps"] = ctx[0].n, steps - 1
    ids, _ = ctx[0].interface()
    rng = np.random.default_rng(1)
    rec = {pre: dict(ms=[], cg=[]) for pre in ctx}
    for s in range(steps):
        t = 0.5e6 * 1e-4 * rng.standard_normal((len(ids), 3))
        for pre, G in ctx.items():
            G.set_interface_traction(t)
            t0 = time.perf_counter()
            its, _ = G.linear_step(True, 1e-10)
            ms = 1e3 * (time.perf_counter() - t0)
            if s:
                rec[pre]["ms"].append(ms)
                rec[pre]["cg"].append(its)
    for pre, G in ctx.items():
        out[NAMES[pre]].update(ms_median=round(statistics.median(rec[pre]["ms"]), 3), ms=[round(v, 3) for v in rec[pre]["ms"]],
                               cg_per_step=rec[pre]["cg"])
        G.close()
    j, m = out["jacobi"], out["multigrid"]
    out["ratio_step_jacobi_over_multigrid"] = round(j["ms_median"] / m["ms_median"], 3)
    out["every_multigrid_step_faster"] = max(m["ms"]) < min(j["ms"])
    out["every_jacobi_step_faster"] = max(j["ms"]) < min(m["ms"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default="q3:24x12x5,q3:24x24x24,q3:40x40x40,q1:40x40x40")
    ap.add_argument("--dts", default="0.005,0.02")
    ap.add_argument("--steps", type=int, default=6, help="steps per context, the first one untimed")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    lines = []
    for case in a.cases.split(","):
        element, sz = case.split(":")
        for dt in a.dts.split(","):
            lines.append(json.dumps(run(element, tuple(int(v) for v in sz.split("x")), float(dt), max(2, a.steps))))
            print(lines[-1], flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
