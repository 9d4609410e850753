"""3D Q3 blocks, both fine levels in one process, steps alternated: ms per Newmark step, Newton and CG iterations.

  python tools/q3_fine_level_steps.py [--sizes 24x12x5,24x24x24,40x40x40] [--steps 6] [--levels 0,1] [--out FILE]

For every size two contexts of the same block (the reference's defaults: clamped at x = 0, traction on the other faces,
multigrid-PCG above 75 k dofs, the executable's warm start) run side by side: "fine_level" 0 (the assembled tangent and
sell_spmv) and "fine_level" 1 (point records + mf_spmv_q3, "mf_diag_lag" 1 as the executable sets it).  Step k of one
context is followed by step k of the other, so both see the same state of the machine.  The first step is a warm-up; the
others are timed (wall clock around mi_newmark_step, which returns after the step's last synchronisation).  Printed per
size and level: median and mean ms per step, Newton iterations and CG iterations per solve of every timed step, the bytes of
the point records and (assembled) of the tangent's values from its block pattern.  --levels 1 runs the matrix-free level
alone (a profiler run of its steps).
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


def tangent_bytes(reps, p=3):
    """values of the assembled tangent: 9 doubles per coupled node pair (the block pattern of a Q_p lattice)"""
    total = 1
    for n in reps:
        nn = p * n + 1
        s = 0
        for i in range(nn):
            cells = [c for c in (i // p - (1 if i % p == 0 else 0), i // p) if 0 <= c < n]
            lo, hi = min(cells) * p, (max(cells) + 1) * p
            s += hi - lo + 1
        total *= s
    return 72 * total


def run(reps, steps, levels=(0, 1)):
    ctx = {}
    for fl in levels:
        G = M.Context(dim=3, degree=3, reps=reps, hi=tuple(0.1 * r for r in reps))
        G.set_tuning("cg_warm_start", 2)
        if fl:
            G.set_tuning("fine_level", 1)
            G.set_tuning("mf_diag_lag", 1)
        ctx[fl] = G
    ncells = reps[0] * reps[1] * reps[2]
    rec = {fl: dict(ms=[], newton=[], cg=[]) for fl in ctx}
    for s in range(steps):
        for fl, G in ctx.items():
            G.set_interface_traction((0.0, -1e3 * min(1.0, (s + 1) / 4.0), 0.0))
            t0 = time.perf_counter()
            rc, info = G.newmark_step(tol_lin=1e-6, max_it_mult=1.0)
            dt = 1e3 * (time.perf_counter() - t0)
            if rc != 0 or info.converged != 1:
                raise RuntimeError("step %d of fine_level %d: rc %d" % (s, fl, rc))
            if s == 0:
                continue
            rec[fl]["ms"].append(dt)
            rec[fl]["newton"].append(info.newton_iterations)
            rec[fl]["cg"].append(list(info.lin_its)[:info.newton_iterations])
    n = next(iter(ctx.values())).n
    for G in ctx.values():
        G.close()
    out = dict(reps=list(reps), dofs=n, timed_steps=steps - 1)
    for fl, r in rec.items():
        key = "matrix_free" if fl else "assembled"
        out[key] = dict(ms_median=round(statistics.median(r["ms"]), 2), ms_mean=round(statistics.mean(r["ms"]), 2),
                        ms=[round(x, 2) for x in r["ms"]], newton=r["newton"], cg_per_solve=r["cg"])
    if 1 in ctx:
        out["matrix_free"]["record_bytes"] = ncells * 11 * 128 * 8
    if 0 in ctx:
        out["assembled"]["tangent_bytes"] = tangent_bytes(reps)
    if len(ctx) == 2:
        out["ratio_assembled_over_matrix_free"] = round(out["assembled"]["ms_median"] / out["matrix_free"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="24x12x5,24x24x24,40x40x40")
    ap.add_argument("--steps", type=int, default=6, help="steps per level, the first one untimed (>= 6: five timed)")
    ap.add_argument("--levels", default="0,1", help="fine levels to run: 0 assembled, 1 matrix-free")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    lines = []
    for sz in a.sizes.split(","):
        reps = tuple(int(x) for x in sz.split("x"))
        r = run(reps, max(2, a.steps), tuple(int(x) for x in a.levels.split(",")))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
