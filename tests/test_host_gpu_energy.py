"""GPU: the executable's step log carries the energy diagnostics.

Every line of <Output folder>/steps.jsonl has "strain_energy", "kinetic_energy" and "body_potential" (one mi_energy per
solved step, after mi_newmark_finish_step).  They are held to tests/golden/energy_reference.py evaluated on the CPU oracle's
displacement and velocity after the same steps of the same coupling script.  Tolerance: 1e-7 relative, ten times the 1e-8 at
which test_host_gpu.py holds the interface displacements of this case -- the energies are quadratic in the state, so a
relative error e of the state shows as about 2 e.
"""
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_host_gpu import TOL, _prm, _run_case, _scenario_desc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import energy_reference as E  # noqa: E402
import mirror as Mi  # noqa: E402

pytestmark = pytest.mark.gpu


def test_step_log_carries_the_energies(tmp_path):
    name = "fsi3_neo_2d_explicit"
    _run_case(name, "elasticity", tmp_path)
    steps = [json.loads(l) for l in open(tmp_path / "out" / "steps.jsonl")]
    assert len(steps) == 4
    get = _prm(name)
    desc = _scenario_desc(get, 2)
    P = O.Problem(desc)
    mesh = Mi.Mesh(2, desc.degree, tuple(desc.reps)[:2], tuple(desc.lo)[:2], tuple(desc.hi)[:2], list(desc.face_role)[:4])
    assert mesh.n == P.n and np.array_equal(mesh.constrained, np.asarray(P.constrained, bool))
    body = tuple(desc.body_force)[:2]
    vol = E.volume(mesh)
    for k, s in enumerate(steps):
        P.set_interface_traction((0.0, -40.0 * min(1.0, (k + 1) / 4.0)))
        rc, _ = P.newmark_step(O.SOLVER_CG_SSOR, tol_lin=1e-12, max_it_mult=2.0)
        assert rc == 0
        u, v = P.vec(O.V_U).copy(), P.vec(O.V_V).copy()
        strain, kinetic, pot, det = E.energies(mesh, u, v, desc.mu, desc.nu, desc.rho, body)
        assert det > 0
        got = [s[key] for key in ("strain_energy", "kinetic_energy", "body_potential")]
        assert all(np.isfinite(g) for g in got)
        print("step %d: strain %.6e (rel %.1e) kinetic %.6e (rel %.1e) body %.6e" % (
            k + 1, got[0], abs(got[0] - strain) / strain, got[1], abs(got[1] - kinetic) / kinetic, got[2]))
        assert strain > 0 and kinetic > 0
        assert abs(got[0] - strain) <= 10 * TOL * strain
        assert abs(got[1] - kinetic) <= 10 * TOL * kinetic
        assert abs(got[2] - pot) <= 10 * TOL * desc.rho * np.linalg.norm(body) * np.abs(u).max() * vol
