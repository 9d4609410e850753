"""Cross-check of the two sum-factorised stress error kernels against stress_error_cells on 3D Q2 / Q3 meshes (experiments build).

MI_STRESS_ERROR_GENERIC=1 makes launch_stress_error take the generic kernel on 3D Q2 / Q3 as well (pass 1, mi_stress_field's
kernels, stays as it is: both runs read the same nodal field); the hook exists in libmi_elasticity_exp.so only and is read once
per process, so the two forms run in two processes:

    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so python tools/stress_error_generic_check.py fast.npz
    MI_LIB=dealii-adapter_amd/libmi_elasticity_exp.so MI_STRESS_ERROR_GENERIC=1 python tools/stress_error_generic_check.py generic.npz
    python tools/stress_error_generic_check.py fast.npz generic.npz   # asserts 1e-12 (cells: of sqrt(eta_K^2 + n_K^2); totals: relative)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MESHES = [(2, (2, 2, 2)), (2, (3, 2, 2)), (3, (2, 2, 2)), (3, (3, 2, 3))]

if len(sys.argv) == 3:
    a, b = (np.load(f) for f in sys.argv[1:])
    for key in sorted(k[:-4] for k in a.files if k.endswith(":eta")):
        scale = np.sqrt(b[key + ":eta"] ** 2 + b[key + ":n"] ** 2)
        err = [(np.abs(a[key + ":eta"] - b[key + ":eta"]) / scale).max(), (np.abs(a[key + ":n"] - b[key + ":n"]) / scale).max(),
               np.abs(a[key + ":tot"] / b[key + ":tot"] - 1).max()]
        print(key, "eta_K %.2e n_K %.2e totals %.2e" % tuple(err))
        assert max(err) <= 1e-12 and a[key + ":max"] == b[key + ":max"]
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
        r = G.stress_error()
        out[key + ":eta"], out[key + ":n"], out[key + ":max"] = r["eta_cell"], r["norm_cell"], r["max_cell"]
        out[key + ":tot"] = np.array([r["error"], r["norm"], r["relative"]])
        G.close()
np.savez(sys.argv[1], **out)
