"""Cross-check of the two sum-factorised stress kernels against stress_cells on 3D Q2 / Q3 meshes (experiments build).

MI_STRESS_GENERIC=1 makes launch_stress take the generic kernel on 3D Q2 / Q3 as well; the hook exists in
libmi_elasticity_exp.so only and is read once per process, so the two forms run in two processes:

    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so python tools/stress_generic_check.py fast.npz
    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_STRESS_GENERIC=1 python tools/stress_generic_check.py generic.npz
    python tools/stress_generic_check.py fast.npz generic.npz      # asserts 1e-12 (sigma: of max|sigma|; von Mises, weight: relative)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MESHES = [(2, (2, 2, 2)), (2, (3, 2, 2)), (3, (2, 2, 2)), (3, (3, 2, 3))]

if len(sys.argv) == 3:
    a, b = (np.load(f) for f in sys.argv[1:])
    for key in sorted(k[:-6] for k in a.files if k.endswith(":sigma")):
        smax = np.abs(b[key + ":sigma"]).max()
        err = [np.abs(a[key + ":sigma"] - b[key + ":sigma"]).max() / smax,
               np.abs(a[key + ":vm"] / b[key + ":vm"] - 1).max(), np.abs(a[key + ":w"] / b[key + ":w"] - 1).max()]
        print(key, "sigma %.2e von Mises %.2e weight %.2e" % tuple(err))
        assert max(err) <= 1e-12
    sys.exit(0)

from bench import _pkg  # noqa: E402

M = _pkg()
out = {}
for p, reps in MESHES:
    for perturbed in (False, True):
        rng = np.random.default_rng(10 * p + sum(reps) + int(perturbed))
        nv = int(np.prod([r + 1 for r in reps]))
        perturb = 0.01 * rng.uniform(-1, 1, (nv, 3)) if perturbed else None
        G = M.Context(dim=3, degree=p, reps=reps, hi=tuple(0.1 * r for r in reps), mu=0.7e6, nu=0.3, rho=870.0, perturb=perturb)
        G.set(M.V_U, 0.0005 * rng.standard_normal(G.n) * ~G.constrained)
        key = "Q%d %s %s" % (p, "x".join(map(str, reps)), "perturbed" if perturbed else "box")
        out[key + ":sigma"], out[key + ":vm"], out[key + ":w"] = G.stress_field()
        G.close()
np.savez(sys.argv[1], **out)
