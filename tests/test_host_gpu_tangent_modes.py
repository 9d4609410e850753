"""GPU: the nonlinear executable's switch MI_TANGENT_MODES=k on a shipped small case (2D FSI3 flap, Q2, explicit coupling, four
windows of a ramped load).

With MI_TANGENT_MODES=3 the run prints lambda, omega and the frequency of the three lowest modes of the tangent after its last
time step and writes tangent_modes.json beside the displacement log.  Its eigenvalues meet Context.tangent_modes on a context
stepped through the same four loads with the parameter file's tolerances to 1e-6 relative: both are converged to 1e-8 of
lambda_3 in the residual (an eigenvalue's error is quadratic in it), and the two final states agree to the linear solver's
1e-12.  Both run the analysis with the V-cycle: the executable's report switches "precond" to 1 for its call and back (with the
diagonal this flap needs 2670 iterations, with the V-cycle 70).

Without the variable nothing of it exists: no tangent_modes.json, no word of it in the output, and every file the run writes --
the displacement log, probe and reaction logs, the output folder -- is byte for byte what the run with the variable writes.
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

NAME = "fsi3_neo_2d_explicit"


def _files(d):
    out = {f: open(d / f, "rb").read() for f in ("displacement.log", "probes.log", "reactions.log", "tangent_modes.json")
           if os.path.exists(d / f)}
    for f in sorted(os.listdir(d / "out")):
        out["out/" + f] = open(d / "out" / f, "rb").read()
    return out


def test_executable_reports_the_tangent_modes(tmp_path):
    (tmp_path / "plain").mkdir()
    (tmp_path / "modes").mkdir()
    out0, rows0 = _run_case(NAME, "elasticity", tmp_path / "plain")
    out1, rows1 = _run_case(NAME, "elasticity", tmp_path / "modes", env={"MI_TANGENT_MODES": "3"})
    assert "MI_TANGENT_MODES ignored" not in out1 and "Tangent modes" in out1 and "Tangent modes" not in out0
    hz_log = [float(v) for v in re.findall(r"frequency = (\S+) Hz", out1)]
    js = json.loads(open(tmp_path / "modes" / "tangent_modes.json").read())
    assert sorted(js) == ["converged", "frequency_hz", "iterations", "lambda", "residual", "stable", "time"]
    lam = np.array(js["lambda"])
    assert js["converged"] is True and len(lam) == 3 and js["iterations"] >= 1 and max(js["residual"]) <= 1e-8
    assert js["stable"] == [True] * 3 and np.all(lam > 0) and np.all(np.diff(lam) > 0)
    assert np.allclose(js["frequency_hz"], np.sqrt(lam) / (2 * np.pi), rtol=1e-14)
    assert len(hz_log) == 3 and np.allclose(hz_log, js["frequency_hz"], rtol=5e-4)  # (the stream prints 4 digits here)
    # the same mesh and load history through the Python wrapper: nonlinear_elasticity.cc's FSI3 flap in the plane
    get = _prm(NAME)
    dt = float(get("Time step size"))
    assert abs(js["time"] - 4 * dt) < 1e-12
    G = M.Context(dim=2, degree=int(get("Polynomial degree")), reps=(18, 3), lo=(0.24899, 0.19), hi=(0.6, 0.21),
                  face_role=[M.FACE_CLAMPED, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_ZCLAMP, M.FACE_ZCLAMP],
                  mu=float(get("Shear modulus")), nu=float(get("Poisson's ratio")), rho=float(get("rho")), delta_t=dt)
    for k in range(4):
        G.set_interface_traction((0.0, -40.0 * min(1.0, (k + 1) / 4.0)))
        rc, info = G.newmark_step(tol_lin=float(get("Residual")), max_it_mult=float(get("Max iteration multiplier")))
        assert rc == 0 and info.converged == 1
    G.set_tuning("precond", 1)  # as the executable's report does for its call
    ref = G.tangent_modes(3, tol=1e-8, max_it=1000, want_modes=False)
    G.close()
    print("lambda %s, frequencies %s Hz, %d iterations (wrapper: %s, %d)" % (lam, js["frequency_hz"], js["iterations"], ref["lam"], ref["its"]))
    assert np.all(np.abs(lam - ref["lam"]) <= 1e-6 * np.abs(ref["lam"]))
    # without the variable: the same files, bit for bit, and no tangent_modes.json; the same output up to the report
    f0, f1 = _files(tmp_path / "plain"), _files(tmp_path / "modes")
    assert "tangent_modes.json" not in f0 and "tangent_modes.json" in f1
    del f1["tangent_modes.json"]
    assert sorted(f0) == sorted(f1) and "displacement.log" in f0
    for name in f0:
        assert f0[name] == f1[name], name
    assert len(rows0) == len(rows1) == 4
