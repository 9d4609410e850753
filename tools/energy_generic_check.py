"""Cross-check of the two sum-factorised energy kernels against energy_cells on 3D Q2 / Q3 meshes (experiments build).

MI_ENERGY_GENERIC=1 makes launch_energy take the generic kernel on 3D Q2 / Q3 as well; the hook exists in
libmi_elasticity_exp.so only and is read once per process, so the two forms run in two processes:

    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so python tools/energy_generic_check.py > fast.json
    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_ENERGY_GENERIC=1 python tools/energy_generic_check.py > generic.json
    python tools/energy_generic_check.py fast.json generic.json      # asserts 1e-12 (strain, kinetic; body: of its scale)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RHO, BODY = 870.0, (0.3, -9.81, 1.0)
MESHES = [(2, (2, 2, 2)), (2, (3, 2, 2)), (3, (2, 2, 2)), (3, (3, 2, 3))]

if len(sys.argv) == 3:
    a, b = (json.load(open(f)) for f in sys.argv[1:])
    for x, y in zip(a, b):
        assert x["key"] == y["key"]
        err = [abs(x["strain"] - y["strain"]) / y["strain"], abs(x["kinetic"] - y["kinetic"]) / y["kinetic"],
               abs(x["body"] - y["body"]) / x["body_scale"]]
        print(x["key"], "strain %.2e kinetic %.2e body %.2e" % tuple(err))
        assert max(err) <= 1e-12
    sys.exit(0)

from bench import _pkg  # noqa: E402

M = _pkg()
out = []
for p, reps in MESHES:
    for perturbed in (False, True):
        rng = np.random.default_rng(10 * p + sum(reps) + int(perturbed))
        nv = int(np.prod([r + 1 for r in reps]))
        perturb = 0.01 * rng.uniform(-1, 1, (nv, 3)) if perturbed else None
        hi = tuple(0.1 * r for r in reps)
        G = M.Context(dim=3, degree=p, reps=reps, hi=hi, mu=0.7e6, nu=0.3, rho=RHO, body_force=BODY, perturb=perturb)
        u = 0.0005 * rng.standard_normal(G.n) * ~G.constrained
        G.set(M.V_U, u)
        G.set(M.V_V, rng.standard_normal(G.n))
        e = G.energy()
        e.update(key="Q%d %s %s" % (p, "x".join(map(str, reps)), "perturbed" if perturbed else "box"),
                 body_scale=RHO * float(np.linalg.norm(BODY)) * float(np.abs(u).max()) * float(np.prod(hi)))
        out.append(e)
        G.close()
print(json.dumps(out))
