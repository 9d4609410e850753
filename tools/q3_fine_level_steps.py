"""3D Q3 blocks, both fine levels in one process, steps alternated: ms per Newmark step, Newton and CG iterations.

  python tools/q3_fine_level_steps.py [--sizes 24x12x5,24x24x24,40x40x40] [--steps 6] [--levels 0,1]
                                      [--smoother-points 5,4] [--out FILE]

For every size two contexts of the same block (the reference's defaults: clamped at x = 0, traction on the other faces,
multigrid-PCG above 75 k dofs, the executable's warm start) run side by side: "fine_level" 0 (the assembled tangent and
sell_spmv) and "fine_level" 1 (point records + mf_spmv_q3, "mf_diag_lag" 1 as the executable sets it).  Step k of one
context is followed by step k of the other, so both see the same state of the machine.  The first step is a warm-up; the
others are timed (wall clock around mi_newmark_step, which returns after the step's last synchronisation).  Printed per
size and level: median and mean ms per step, Newton iterations and CG iterations per solve of every timed step, the bytes of
the point records and (assembled) of the tangent's values from its block pattern.  --levels 1 runs the matrix-free level
alone (a profiler run of its steps).
--smoother-points 5,4: one matrix-free context per rule of the multigrid smoother's fine-level operator
("smoother_quadrature_q3": 5 the assembly's 125 points, 4 the element's full-order 64 points on records of its own), their
steps alternated in the same way; the same statistics per rule ("matrix_free" for 5, "matrix_free_q4" for 4), the bytes of
the second record array, and whether EVERY timed step of rule 4 was faster than EVERY timed step of rule 5.
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


def run(reps, steps, levels=(0, 1), points=(5,)):
    # a context per (fine level, smoother rule): (0, 5) assembled, (1, 5) / (1, 4) matrix-free
    ctx = {}
    for fl, q in [(fl, q) for fl in levels for q in (points if fl else (5,))]:
        G = M.Context(dim=3, degree=3, reps=reps, hi=tuple(0.1 * r for r in reps))
        G.set_tuning("cg_warm_start", 2)
        if fl:
            G.set_tuning("fine_level", 1)
            G.set_tuning("mf_diag_lag", 1)
            G.set_tuning("smoother_quadrature_q3", q)
        ctx[(fl, q)] = G
    ncells = reps[0] * reps[1] * reps[2]
    rec = {fl: dict(ms=[], newton=[], cg=[]) for fl in ctx}
    for s in range(steps):
        for fl, G in ctx.items():
            G.set_interface_traction((0.0, -1e3 * min(1.0, (s + 1) / 4.0), 0.0))
            t0 = time.perf_counter()
            rc, info = G.newmark_step(tol_lin=1e-6, max_it_mult=1.0)
            dt = 1e3 * (time.perf_counter() - t0)
            if rc != 0 or info.converged != 1:
                raise RuntimeError("step %d of fine_level %s: rc %d" % (s, fl, rc))
            if fl[0] and G.get_tuning("smoother_quadrature_q3_active") != fl[1]:
                raise RuntimeError("fine_level %s: the smoother did not run the rule that was set" % (fl,))
            if s == 0:
                continue
            rec[fl]["ms"].append(dt)
            rec[fl]["newton"].append(info.newton_iterations)
            rec[fl]["cg"].append(list(info.lin_its)[:info.newton_iterations])
    n = next(iter(ctx.values())).n
    for G in ctx.values():
        G.close()
    out = dict(reps=list(reps), dofs=n, timed_steps=steps - 1)
    name = {(0, 5): "assembled", (1, 5): "matrix_free", (1, 4): "matrix_free_q4"}
    for fl, r in rec.items():
        key = name[fl]
        out[key] = dict(ms_median=round(statistics.median(r["ms"]), 2), ms_mean=round(statistics.mean(r["ms"]), 2),
                        ms=[round(x, 2) for x in r["ms"]], newton=r["newton"], cg_per_solve=r["cg"])
    for key in ("matrix_free", "matrix_free_q4"):
        if key in out:
            out[key]["record_bytes"] = ncells * 11 * 128 * 8
    if "matrix_free_q4" in out:
        out["matrix_free_q4"]["smoother_record_bytes"] = ncells * 11 * 64 * 8
    if "assembled" in out:
        out["assembled"]["tangent_bytes"] = tangent_bytes(reps)
    if "assembled" in out and "matrix_free" in out:
        out["ratio_assembled_over_matrix_free"] = round(out["assembled"]["ms_median"] / out["matrix_free"]["ms_median"], 3)
    if "matrix_free" in out and "matrix_free_q4" in out:
        out["ratio_q5_over_q4"] = round(out["matrix_free"]["ms_median"] / out["matrix_free_q4"]["ms_median"], 3)
        out["every_q4_step_faster"] = max(out["matrix_free_q4"]["ms"]) < min(out["matrix_free"]["ms"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="24x12x5,24x24x24,40x40x40")
    ap.add_argument("--steps", type=int, default=6, help="steps per level, the first one untimed (>= 6: five timed)")
    ap.add_argument("--levels", default="0,1", help="fine levels to run: 0 assembled, 1 matrix-free")
    ap.add_argument("--smoother-points", default="5", help="rules of the matrix-free level's smoother: 5 (125 points), 4 (64 points)")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    lines = []
    for sz in a.sizes.split(","):
        reps = tuple(int(x) for x in sz.split("x"))
        r = run(reps, max(2, a.steps), tuple(int(x) for x in a.levels.split(",")), tuple(int(x) for x in a.smoother_points.split(",")))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
