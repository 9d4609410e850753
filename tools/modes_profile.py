"""Modal analysis (mi_linear_modes) on a large block: wall time per iteration, and its split from a rocprofv3 kernel trace.

  python tools/modes_profile.py time   [--cells 40] [--modes 8] [--its 4,12] [--precond 1]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/modes_profile.py trace [--its 8] [--precond 1] [--steps 2]
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python tools/modes_profile.py trace --its 3 --steps 0
  python tools/modes_profile.py reduce DIR [--its 8] [--modes 8]

The block: 3D Q3, cells x cells x cells of 0.1, clamped at x = 0, "linear_operator" 1, dt = 0.02, theta = 0.5, the shipped material.
  time    mi_linear_modes with max_it = a and max_it = b (both stop unconverged, which is what is wanted here): the difference
          over b - a is the wall time of one iteration (host clock around calls that end synchronised); a warm-up call first
  trace   one call with max_it = --its for the profiler to wrap, then --steps multigrid-PCG steps of the linear model, whose
          dot_partials + finish_sum launches on the same vector length are what one scalar product cost before block_gram
  reduce  the kernel trace in time order, cut into the phases of an iteration at the block kernels: preconditioner
          (block_residual_finish .. projection), products (.. the Gram matrices), block algebra (every block_* kernel).  The
          closing polish (m products after the last block_residual) is counted with the preconditioner: 1 / (2 its) of the
          products.  With a counter file: FETCH_SIZE per block_gram dispatch against (ma + mb) n 8 bytes
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

THETA, DT = 0.5, 0.02


def context(cells, precond):
    from bench import _pkg
    M = _pkg()
    G = M.Context(dim=3, degree=3, reps=(cells,) * 3, hi=(0.1 * cells,) * 3, delta_t=DT)
    G.set_tuning("linear_operator", 1)
    G.set_tuning("linear_precond", precond)
    t0 = time.perf_counter()
    G.linear_setup(THETA)
    if G.get_tuning("linear_precond_active") != precond or G.get_tuning("linear_operator_active") != 1:
        raise RuntimeError("the set-up did not run what was set")
    return M, G, time.perf_counter() - t0


def modes(M, G, k, its):
    t0 = time.perf_counter()
    try:
        out = G.linear_modes(k, tol=1e-8, max_it=its, want_modes=False)
    except M.MiError as e:
        if e.code != M.MI_ENOCONV_LIN:
            raise
        out = e.partial
    return time.perf_counter() - t0, out


def cmd_time(a):
    M, G, setup = context(a.cells, a.precond)
    lo, hi = (int(v) for v in a.its.split(","))
    modes(M, G, a.modes, 1)
    t = {its: min(modes(M, G, a.modes, its)[0] for _ in range(2)) for its in (lo, hi)}
    out = modes(M, G, a.modes, hi)[1]
    print(json.dumps(dict(cells=a.cells, dofs=G.n, n_modes=a.modes, precond=a.precond, setup_s=round(setup, 3),
                          seconds={str(k): round(v, 4) for k, v in t.items()},
                          ms_per_iteration=round(1e3 * (t[hi] - t[lo]) / (hi - lo), 3), lam=list(out["lam"]),
                          residual_after=dict(its=out["its"], worst=float(out["residual"].max())))))


def cmd_trace(a):
    M, G, _ = context(a.cells, a.precond)
    dt, out = modes(M, G, a.modes, int(str(a.its).split(",")[-1]))
    print(json.dumps(dict(dofs=G.n, its=out["its"], seconds=round(dt, 4))))
    k = len(G.interface()[0])
    rng = np.random.default_rng(1)
    for _ in range(a.steps):
        G.set_interface_traction(50.0 * rng.standard_normal((k, 3)))
        print("step: %d CG iterations" % G.linear_step(True, 1e-10)[0])


def _rows(d, pattern):
    for f in glob.glob(os.path.join(d, "**", pattern), recursive=True):
        with open(f) as fh:
            yield from csv.DictReader(fh)


def cmd_reduce(a):
    m = a.modes + max(2, a.modes // 4)
    rows = sorted(_rows(a.dir, "*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    phase, ns, per = "products", dict(precond=0, products=0, block=0, other=0), {}
    seen_modes = False
    for r in rows:
        name = r["Kernel_Name"]
        dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        short = name.split("(")[0].replace("void ", "").replace("mi::", "")
        key = short + (" grid %s" % r.get("Grid_Size_X", r.get("Grid_Size", "?")) if "block_gram" in short else "")
        cnt, tot = per.get(key, (0, 0))
        per[key] = (cnt + 1, tot + dur)
        if "block_" in name:
            seen_modes = True
            ns["block"] += dur
            if "block_residual_finish" in name:
                phase = "precond"
            elif "block_combine" in name and phase == "precond":
                phase = "products"
            elif "block_gram" in name and "finish" not in name and phase == "products":
                phase = "rr"
        elif "cg_" in name or "linear_rhs" in name or "linear_update" in name:
            phase = "steps"  # the linear steps behind the call
            ns["other"] += dur
        elif seen_modes or "hash" in name:
            ns[phase if phase in ns else "other"] += dur
    print("per iteration (kernel time, %d iterations): %s" % (a.its, {k: "%.3f ms" % (v / a.its / 1e6) for k, v in ns.items()}))
    for key in sorted(per):
        if any(s in key for s in ("block_", "dot_partials", "finish_sum", "reduce_to_totals")):
            print("  %-60s calls %5d  mean %10.1f us" % (key, per[key][0], per[key][1] / per[key][0] / 1e3))
    g = [(k, v) for k, v in per.items() if k.startswith("block_gram grid")]
    dp, fs = per.get("dot_partials"), per.get("finish_sum")
    if g and dp:
        big = max(g, key=lambda kv: int(kv[0].split()[-1]))
        one = dp[1] / dp[0] + (fs[1] / fs[0] if fs else 0.0)
        print("3 m x 3 m Gram (%s): %.1f us + finish; %d scalar products of dot_partials%s: %d x %.1f us = %.1f us" %
              (big[0], big[1][1] / big[1][0] / 1e3, 9 * m * m, " + finish_sum" if fs else "", 9 * m * m, one / 1e3,
               9 * m * m * one / 1e3))
    for r in _rows(a.dir, "*counter_collection.csv"):
        if "block_gram" in r.get("Kernel_Name", "") and "finish" not in r["Kernel_Name"] and r.get("Counter_Name") == "FETCH_SIZE":
            print("  FETCH_SIZE %s of block_gram grid %s" % (r["Counter_Value"], r.get("Grid_Size_X", r.get("Grid_Size", "?"))))
        if "block_residual<" in r.get("Kernel_Name", "") and r.get("Counter_Name") == "FETCH_SIZE":
            print("  FETCH_SIZE %s of block_residual (reads 2 m n 8 bytes + the mask)" % r["Counter_Value"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["time", "trace", "reduce"])
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--cells", type=int, default=40)
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--its", default="4,12")
    ap.add_argument("--precond", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()
    if a.cmd == "reduce":
        a.its = int(str(a.its).split(",")[-1])
    dict(time=cmd_time, trace=cmd_trace, reduce=cmd_reduce)[a.cmd](a)
