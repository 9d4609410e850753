#!/usr/bin/env python3
"""Driver of tests/test_gpu_energy_rccl.py: mi_energy through the library's RCCL branch.  N rank THREADS (one slab per rank,
the RCCL test double of run_ranks.py, whose loader this uses unchanged) set the same global state and ask for the energies;
the undecomposed context answers the same question.  Prints one JSON line."""
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import run_ranks  # noqa: E402


def main():
    world = int(sys.argv[1])
    dim, p = int(sys.argv[2]), int(sys.argv[3])
    reps = tuple(int(v) for v in sys.argv[4].split(","))
    M = run_ranks.load()
    common = dict(dim=dim, degree=p, reps=reps, hi=tuple(0.1 * r for r in reps), face_role=[1, 7, 7, 7, 8, 7], mu=0.7e6, nu=0.3,
                  rho=870.0, body_force=(0.3, -9.81, 1.0))
    uid = M.comm_unique_id()
    results, errors = [None] * world, []
    state = {}

    def ask(G):
        if not state:
            rng = np.random.default_rng(3)
            state["u"] = 0.002 * rng.standard_normal(G.n) * ~G.constrained
            state["v"] = rng.standard_normal(G.n)
        G.set(M.V_U, state["u"])
        G.set(M.V_V, state["v"])
        e = G.energy()
        return [e["strain"], e["kinetic"], e["body"]]

    single = M.Context(**common)
    ref = ask(single)
    single.close()

    def rank_main(r):
        try:
            G = M.Context(rank=r, world=world, unique_id=uid, **common)
            results[r] = ask(G)
            G.close()
        except BaseException as e:  # noqa: BLE001 -- reported to the parent test
            errors.append("rank %d: %r" % (r, e))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    if errors or any(t.is_alive() for t in threads):
        print(json.dumps({"ok": False, "errors": errors, "hung": [t.is_alive() for t in threads]}), flush=True)
        os._exit(1)
    # scale of the body potential, a signed sum: rho |b| max|u| volume
    bscale = 870.0 * float(np.linalg.norm(common["body_force"][:dim])) * float(np.abs(state["u"]).max()) * float(np.prod(common["hi"]))
    print(json.dumps({"ok": True, "single": ref, "ranks": results, "body_scale": bscale}))


if __name__ == "__main__":
    main()
