"""Cross-check of the two sum-factorised mass kernels (mass_apply_q2, mass_apply_q3) against mass_apply_cells on 3D Q2 / Q3
meshes (experiments build).

MI_MASS_GENERIC=1 makes launch_mass_apply take the generic kernel on 3D Q2 / Q3 as well; the hook exists in
libmi_elasticity_exp.so only and is read once per process, so the two forms run in two processes:

    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so python tools/mass_generic_check.py > fast.json
    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_MASS_GENERIC=1 python tools/mass_generic_check.py > generic.json
    python tools/mass_generic_check.py fast.json generic.json      # asserts 1e-13 relmax, product and solve, masked and not
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MESHES = [(2, (3, 2, 3)), (2, (1, 1, 1)), (2, (6, 5, 4)), (3, (3, 2, 3)), (3, (1, 1, 1))]

if len(sys.argv) == 3:
    a, b = (json.load(open(f)) for f in sys.argv[1:])
    for x, y in zip(a, b):
        assert x["key"] == y["key"]
        err = []
        for k in ("y", "ym", "xs"):
            u, v = np.array(x[k]), np.array(y[k])
            err.append(float(np.abs(u - v).max() / np.abs(v).max()))
        print(x["key"], "product %.2e masked product %.2e solve %.2e" % tuple(err))
        assert max(err[:2]) <= 1e-13 and err[2] <= 1e-10  # (the solve: both stop at tol 1e-12 times kappa_2 <= 5e2)
    sys.exit(0)

from bench import _pkg  # noqa: E402

M = _pkg()
out = []
for p, reps in MESHES:
    for perturbed in (False, True):
        rng = np.random.default_rng(10 * p + sum(reps) + int(perturbed))
        nv = int(np.prod([r + 1 for r in reps]))
        perturb = 0.005 * rng.standard_normal((nv, 3)) if perturbed else None
        G = M.Context(dim=3, degree=p, reps=reps, hi=tuple(0.1 * r for r in reps), perturb=perturb)
        x = rng.standard_normal((6, G.n))
        out.append(dict(key="Q%d %s %s" % (p, "x".join(map(str, reps)), "perturbed" if perturbed else "box"),
                        y=G.mass_apply(x).tolist(), ym=G.mass_apply(x, masked=True).tolist(),
                        xs=G.mass_solve(x[:2], masked=True)[0].tolist()))
        G.close()
print(json.dumps(out))
