"""Modal analysis of the tangent (mi_tangent_modes) on a large block: wall time per iteration, and its split from a rocprofv3
kernel trace.

  python tools/tangent_modes_cost.py time   [--degree 2] [--cells 59] [--fine-level 0] [--modes 8] [--its 4,12] [--precond 1]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/tangent_modes_cost.py trace [--its 8] [...]
  python tools/tangent_modes_cost.py reduce DIR [--its 8]
  python tools/tangent_modes_cost.py product [--degree 2] [--cells 59]

The block: cells x cells x cells of 0.1, clamped at x = 0, the shipped material and time step, stretched by u_x = 0.02 X.  The runs
DESIGN.md section 19 asks for: --degree 2 --cells 59 with --fine-level 0 and 1, --degree 3 --cells 40 --fine-level 1; 8 modes, V-cycle.
  time    mi_tangent_modes with max_it = a and max_it = b (both stop unconverged, which is what is wanted here): the difference
          over b - a is the wall time of one iteration (host clock around calls that end synchronised); a warm-up call first.
          Every call also assembles and refreshes the hierarchy: that part cancels in the difference and is printed on its own
  product sell_spmm on 3 and on 10 columns against as many launches of sell_spmv on the same matrix in the same process, five
          alternated repetitions of ten products each (device events).  Keeping criterion: the slowest block measurement is
          shorter than the fastest 3-fold single measurement
  trace   one call with max_it = --its for the profiler to wrap
  reduce  the kernel trace in time order, cut into the phases of an iteration at the block kernels: block_residual opens the
          preconditioner (V-cycles or the diagonal), the next block_gram the projection, the first mass_apply the products; every
          block_* kernel is block algebra, every mass_* kernel a mass image, whatever the phase.  Assembly and hierarchy refresh
          before the first block kernel are listed as set-up.  Per iteration = total / (--its + 1): the closing polish is one
          more round of products
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


def context(a):
    from bench import _pkg
    M = _pkg()
    G = M.Context(dim=3, degree=a.degree, reps=(a.cells,) * 3, hi=(0.1 * a.cells,) * 3)
    if a.fine_level:
        G.set_tuning("fine_level", 1)
    G.set_tuning("precond", a.precond)
    u = np.zeros((G.nnodes, 3))
    u[:, 0] = 0.02 * G.coords[:, 0]
    G.set(M.V_U, u.reshape(-1))
    return M, G


def modes(M, G, k, its):
    t0 = time.perf_counter()
    try:
        out = G.tangent_modes(k, tol=1e-8, max_it=its, want_modes=False)
    except M.MiError as e:
        if e.code != M.MI_ENOCONV_LIN:
            raise
        out = e.partial
    return time.perf_counter() - t0, out


def cmd_time(a):
    M, G = context(a)
    lo, hi = (int(v) for v in a.its.split(","))
    modes(M, G, a.modes, 1)
    t_lo, _ = modes(M, G, a.modes, lo)
    t_hi, out = modes(M, G, a.modes, hi)
    per = (t_hi - t_lo) / (hi - lo)
    print(json.dumps(dict(n_dofs=G.n, degree=a.degree, cells=a.cells, fine_level=a.fine_level, precond=a.precond, modes=a.modes,
                          ms_per_iteration=1e3 * per, ms_outside_iterations=1e3 * (t_lo - lo * per), lam=list(out["lam"]),
                          residual=list(out["residual"]))))


def cmd_product(a):
    """sell_spmm on NV columns against NV launches of sell_spmv, five alternated repetitions each, and the block of m = 10 columns"""
    a.precond = 0  # (no hierarchy: the product alone)
    M, G = context(a)
    G.assemble()
    out = dict(n_dofs=G.n, nnz=G.nnz, degree=a.degree, cells=a.cells, spmv_lds_launches=G.get_tuning("spmv_lds_launches"))
    for nv in (3, 10):
        before = G.get_tuning("spmm_launches")
        blk, one = G.bench_spmm(nv, reps=10, rounds=5)
        out["nv_%d" % nv] = dict(ms_block=list(blk), ms_single=list(one), slowest_block=blk.max(), fastest_single=one.min(),
                                 single_spread=one.max() / one.min() - 1.0, ratio=one.min() / blk.max(),
                                 keep=bool(blk.max() < one.min()), block_launches=G.get_tuning("spmm_launches") - before)
    print(json.dumps(out))


def cmd_trace(a):
    M, G = context(a)
    modes(M, G, a.modes, a.its)


def phase_split(names_and_ns):
    """{phase: ns} of kernel records (name, duration in ns) in time order"""
    out = {"set-up": 0, "preconditioner": 0, "projection": 0, "products": 0, "mass images": 0, "block algebra": 0}
    phase = "set-up"
    for name, ns in names_and_ns:
        if "block_residual" in name:
            phase = "preconditioner"
        elif "block_gram" in name and phase == "preconditioner":
            phase = "projection"
        elif "mass_apply" in name and phase != "set-up":
            phase = "products"
        elif "block_hash_init" in name:
            phase = "products"
        if "block_" in name:
            out["block algebra"] += ns
        elif "mass_" in name and phase != "set-up":
            out["mass images"] += ns
        else:
            out[phase if phase != "projection" else "block algebra"] += ns
    return out


def cmd_reduce(a):
    rows = []
    for f in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    split = phase_split((n, d) for _, n, d in rows)
    rounds = a.its + 1
    print(json.dumps({k: dict(ms_total=v / 1e6, ms_per_iteration=(v / 1e6 / rounds if k != "set-up" else None)) for k, v in split.items()},
                     indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["time", "trace", "reduce", "product"])
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--cells", type=int, default=59)
    ap.add_argument("--fine-level", type=int, default=0)
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--its", default=None)
    ap.add_argument("--precond", type=int, default=1)
    a = ap.parse_args()
    if a.cmd == "product":
        cmd_product(a)
    elif a.cmd == "time":
        a.its = a.its or "4,12"
        cmd_time(a)
    else:
        a.its = int(a.its or 8)
        cmd_trace(a) if a.cmd == "trace" else cmd_reduce(a)
