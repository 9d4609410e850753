"""Linear model on 3D Q3 or Q2 blocks, assembled and matrix-free operators in one process, steps alternated.

  python tools/linear_operator_steps.py [--degree 3] [--sizes 24x12x5,24x24x24,40x40x40] [--steps 6] [--products 5]
                                        [--precond 0] [--dt 0.005] [--out FILE]

For every size two contexts of the same block (clamped at x = 0, interface on the other faces, theta = 0.5, the shipped
material and time step) are set up side by side: "linear_operator" 0 (K, M and the stepping matrix assembled in the tangent's
sliced-ELL layout, the products on sell_spmv) and the matrix-free form (nothing assembled: --degree 3 "linear_operator" 1,
mf_linear_q3 + the slot gathers; --degree 2 "linear_operator" 2, mf_linear_q2 + the slot gathers).  --precond 1: both with the
model's multigrid V-cycle ("linear_precond" 1) instead of the Jacobi diagonal; --dt: the time step.
Step k of one context is followed by step k of the other with the same random interface load, so both see the same state
of the machine.  The first step is a warm-up; the others are timed (wall clock around mi_linear_step, which returns after
the step's last synchronisation; Jacobi-PCG to the executable's absolute 1e-10).  Printed per size and mode: set-up time
(mi_linear_setup, wall clock), free device memory after the set-up (hipMemGetInfo; the two contexts are created one after
the other, so the difference of consecutive readings is what a mode keeps), median and every ms per step, CG iterations
per step, and the microseconds per product of K, M and the stepping matrix from device stamps (mi_linear_apply with
profiling on times the product alone, class "spmv": the kernel and its gather, or the sliced-ELL launch); the ratios
assembled / matrix-free; and whether EVERY timed matrix-free step was faster than EVERY timed assembled one.
"""
import argparse
import ctypes as C
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
NAMES = {0: "assembled", 1: "matrix_free"}


def free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def run(reps, steps, products, degree=3, precond=0, dt=0.005):
    ctx, out = {}, dict(reps=list(reps), degree=degree, linear_precond=precond, delta_t=dt)
    M.lib()
    for mode in (0, 1):
        G = M.Context(dim=3, degree=degree, reps=reps, hi=tuple(0.1 * r for r in reps), delta_t=dt)
        before = free_bytes()
        G.set_tuning("linear_operator", (2 if degree == 2 else 1) if mode else 0)
        G.set_tuning("linear_precond", precond)
        t0 = time.perf_counter()
        G.linear_setup(THETA)
        out[NAMES[mode]] = dict(setup_s=round(time.perf_counter() - t0, 3), free_bytes_after_setup=free_bytes(),
                                setup_bytes=before - free_bytes())
        if G.get_tuning("linear_operator_active") != ((2 if degree == 2 else 1) if mode else 0):
            raise RuntimeError("the set-up did not run the operator that was set")
        ctx[mode] = G
    out["dofs"], out["timed_steps"] = ctx[0].n, steps - 1
    ids, _ = ctx[0].interface()
    rng = np.random.default_rng(1)
    rec = {mode: dict(ms=[], cg=[]) for mode in ctx}
    for s in range(steps):
        t = 0.5e6 * 1e-4 * rng.standard_normal((len(ids), 3))
        for mode, G in ctx.items():
            G.set_interface_traction(t)
            t0 = time.perf_counter()
            its, _ = G.linear_step(True, 1e-10)
            dt = 1e3 * (time.perf_counter() - t0)
            if s:
                rec[mode]["ms"].append(dt)
                rec[mode]["cg"].append(its)
    x = rng.standard_normal(ctx[0].n)
    for mode, G in ctx.items():
        r = out[NAMES[mode]]
        r.update(ms_median=round(statistics.median(rec[mode]["ms"]), 3), ms=[round(v, 3) for v in rec[mode]["ms"]],
                 cg_per_step=rec[mode]["cg"])
        G.set_profiling(True)
        r["us_per_product"] = {}
        for which, name in enumerate(("K", "M", "A")):
            G.linear_apply(which, x)  # warm-up
            G.reset_timings()
            for _ in range(products):
                G.linear_apply(which, x)
            ms, count = G.timings()["spmv"]
            r["us_per_product"][name] = round(1e3 * ms / count, 2)
        G.close()
    a, m = out["assembled"], out["matrix_free"]
    out["ratio_step_assembled_over_matrix_free"] = round(a["ms_median"] / m["ms_median"], 3)
    out["ratio_product_assembled_over_matrix_free"] = {k: round(a["us_per_product"][k] / m["us_per_product"][k], 3)
                                                       for k in ("K", "M", "A")}
    out["every_matrix_free_step_faster"] = max(m["ms"]) < min(a["ms"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="24x12x5,24x24x24,40x40x40")
    ap.add_argument("--degree", type=int, default=3, choices=(2, 3), help="3: mf_linear_q3 | 2: mf_linear_q2")
    ap.add_argument("--precond", type=int, default=0, choices=(0, 1), help="\"linear_precond\" of both contexts")
    ap.add_argument("--dt", type=float, default=0.005, help="time step of both contexts")
    ap.add_argument("--steps", type=int, default=6, help="steps per mode, the first one untimed")
    ap.add_argument("--products", type=int, default=5, help="timed products per operator")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    lines = []
    for sz in a.sizes.split(","):
        lines.append(json.dumps(run(tuple(int(v) for v in sz.split("x")), max(2, a.steps), max(1, a.products), a.degree, a.precond,
                                    a.dt)))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
