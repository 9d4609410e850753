"""GPU: the executable's switch MI_MODES=k on the shipped 3D linear case (FSI3 flap, Q3).

With MI_MODES=4 the run prints lambda, omega and the frequency of the four lowest modes before its first step and writes
<Output folder>/modes.json; its eigenvalues meet Context.linear_modes on the same mesh, material and time step to 1e-6 relative
(both are converged to 1e-8 of lambda_4 in the residual, and an eigenvalue's error is quadratic in it).  Both run with the
multigrid preconditioner (MI_LINEAR_PRECOND=1 / "linear_precond" 1): at the shipped time step sigma = 1 / (theta dt)^2 = 1.6e5 lies
two decades above lambda_1, where the Jacobi-preconditioned iteration takes hundreds of steps.

Without the variable nothing of it exists: no modes.json, no word of it in the log, and every file the run writes -- the
displacement log and the output folder -- is byte for byte what the run with the variable writes next to its modes.json.
"""
import json
import os
import re

import numpy as np
import pytest

from conftest import load_pkg
from test_host_gpu import _prm, _run_case

M = load_pkg()
pytestmark = pytest.mark.gpu

NAME = "fsi3_linear_3d_shipped"


def _files(d):
    out = {"displacement.log": open(d / "displacement.log", "rb").read()}
    for f in sorted(os.listdir(d / "out")):
        out["out/" + f] = open(d / "out" / f, "rb").read()
    return out


def test_executable_reports_the_lowest_modes(tmp_path):
    (tmp_path / "plain").mkdir()
    (tmp_path / "modes").mkdir()
    env = {"MI_LINEAR_PRECOND": "1"}
    out0, rows0 = _run_case(NAME, "elasticity3d", tmp_path / "plain", env=env)
    out1, rows1 = _run_case(NAME, "elasticity3d", tmp_path / "modes", env=dict(env, MI_MODES="4"))
    assert "MI_MODES ignored" not in out1 and "Vibration modes" in out1 and "Vibration modes" not in out0
    hz_log = [float(v) for v in re.findall(r"frequency = (\S+) Hz", out1)]
    js = json.loads(open(tmp_path / "modes" / "out" / "modes.json").read())
    assert sorted(js) == ["converged", "frequency_hz", "iterations", "lambda", "residual"]
    lam = np.array(js["lambda"])
    assert js["converged"] is True and len(lam) == 4 and js["iterations"] >= 1 and max(js["residual"]) <= 1e-8
    assert np.allclose(js["frequency_hz"], np.sqrt(lam) / (2 * np.pi), rtol=1e-14)
    assert len(hz_log) == 4 and np.allclose(hz_log, js["frequency_hz"], rtol=1e-4)  # (printed with 6 digits)
    # the same mesh through the Python wrapper: linear_elasticity.cc's FSI3 flap
    get = _prm(NAME)
    G = M.Context(dim=3, degree=int(get("Polynomial degree")), reps=(18, 3, 1), lo=(0.24899, 0.19, -0.005), hi=(0.6, 0.21, 0.005),
                  face_role=[M.FACE_CLAMPED, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_ZCLAMP, M.FACE_ZCLAMP],
                  mu=float(get("Shear modulus")), nu=float(get("Poisson's ratio")), rho=float(get("rho")),
                  delta_t=float(get("Time step size")))
    G.set_tuning("linear_precond", 1)
    G.linear_setup(0.5)
    ref = G.linear_modes(4, tol=1e-8, max_it=1000, want_modes=False)
    G.close()
    print("lambda %s, frequencies %s Hz, %d iterations (wrapper: %d)" % (lam, js["frequency_hz"], js["iterations"], ref["its"]))
    assert np.all(lam > 0) and np.abs(lam - ref["lam"]).max() <= 1e-6 * ref["lam"].max()
    assert np.all(np.abs(lam - ref["lam"]) <= 1e-6 * ref["lam"])
    # without the variable: the same files, bit for bit, and no modes.json
    f0, f1 = _files(tmp_path / "plain"), _files(tmp_path / "modes")
    assert "out/modes.json" not in f0 and "out/modes.json" in f1
    del f1["out/modes.json"]
    assert sorted(f0) == sorted(f1)
    for name in f0:
        assert f0[name] == f1[name], name
    assert len(rows0) == len(rows1) >= 3
