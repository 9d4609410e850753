"""GPU: the nonlinear executable's switch MI_EXPLICIT=1 on the shipped small 3D case block_neo_3d_q2 (3 x 2 x 2 Q2 cells, two
windows of a ramped traction).

With the variable every time step of the parameter file becomes n_sub = ceil(dt / (0.8 dt_crit)) explicit central-difference steps
of dt / n_sub (mi_explicit_run), dt_crit from mi_explicit_stable_dt before the first step.  A Python Context driven through the
same calls -- stable_dt at the start, set-up with init_acceleration 1 at the first step and 0 afterwards, the traction set once per
time step -- gives the displacement log and the explicit_* keys of steps.jsonl to 1e-12 of the largest entry, and n_sub is what
ceil(dt / (0.8 dt_crit)) of explicit_stable_dt gives.  Without the variable steps.jsonl has none of the keys.
"""
import json
import math

import numpy as np
import pytest

from conftest import load_pkg
from test_host_gpu import _prm, _run_case

M = load_pkg()
pytestmark = pytest.mark.gpu

NAME = "block_neo_3d_q2"


def test_executable_steps_explicitly(tmp_path):
    (tmp_path / "explicit").mkdir()
    out, rows = _run_case(NAME, "elasticity3d", tmp_path / "explicit", env={"MI_EXPLICIT": "1"})
    steps = [json.loads(l) for l in open(tmp_path / "explicit" / "out" / "steps.jsonl")]
    assert len(rows) == 2 and len(steps) == 2 and "explicit:" in out
    get = _prm(NAME)
    dt = float(get("Time step size"))
    G = M.Context(dim=3, degree=int(get("Polynomial degree")), reps=(3, 2, 2), lo=(0, 0, 0), hi=(0.3, 0.2, 0.2),
                  mu=float(get("Shear modulus")), nu=float(get("Poisson's ratio")), rho=float(get("rho")), delta_t=dt)
    ids, _ = G.interface()
    _, dt_crit = G.explicit_stable_dt()
    n_sub = max(1, math.ceil(dt / (0.8 * dt_crit)))
    for k in range(2):
        G.set_interface_traction((0.0, -2000.0 * min(1.0, (k + 1) / 10.0), 0.0))
        G.explicit_setup(dt / n_sub, init_acceleration=(k == 0))
        info = G.explicit_run(n_sub)
        u = G.get_interface_displacement().reshape(-1)
        s = steps[k]
        assert s["explicit_substeps"] == n_sub == info["steps_done"]
        assert abs(s["explicit_dt"] - dt / n_sub) <= 1e-12 * dt
        assert abs(s["kinetic_lumped"] - info["kinetic_lumped"]) <= 1e-12 * abs(info["kinetic_lumped"])
        err = np.abs(rows[k][1:] - u).max() / np.abs(u).max()
        print("window %d: %d substeps of %.4e, displacement log against the Python context %.2e" % (k, n_sub, dt / n_sub, err))
        assert np.abs(u).max() > 0 and err <= 1e-12
    G.close()


def test_without_the_variable_nothing_of_it_exists(tmp_path):
    out, rows = _run_case(NAME, "elasticity3d", tmp_path)
    steps = [json.loads(l) for l in open(tmp_path / "out" / "steps.jsonl")]
    assert "explicit" not in out and all(not any(key.startswith("explicit") or key == "kinetic_lumped" for key in s) for s in steps)
