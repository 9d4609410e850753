"""CPU anchor of tests/golden/modes_reference.py: the conditions under which the assertions of tests/test_gpu_linear_modes.py are
derived hold on the cases it runs.  No device, no library; K and M are mirror.Linear's.

Per case (dense eigh of K_ff, M_ff):
  * the rigid cluster has the size the boundary conditions leave (0 with a clamped face; 3 in the plane, 6 in space) and its
    eigenvalues are zero to 1e-9 of lambda_n_modes, the first elastic one is not
  * the smallest gap among the first n_modes + 3 eigenvalues outside the rigid cluster is >= 1e-3 of lambda_n_modes: every
    wanted eigenvalue is told apart from its neighbours at tolerance 1e-8 with five decades to spare
  * eps lambda_max / lambda_n_modes <= 1e-10: the rounding of one evaluation of K x - lambda M x, relative to the scale of the
    stopping rule lambda_n_modes |M x|, is two decades below tol = 1e-8 -- what the factor 2 in the GPU test's re-evaluation
    of the stopping rule covers
Measured here: gap 2.0e-3 (q2_432g), >= 6e-3 elsewhere; lambda_max / lambda_n_modes <= 5.5e3.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import modes_reference as MR  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name", list(MR.CASES))
def test_reference_pencil_is_well_conditioned(name):
    c = MR.CASES[name]
    mesh = MR.case_mesh(name)
    lin = Mi.Linear(mesh, dt=MR.DT, theta=MR.THETA)
    Kf, Mf, free = MR.free_pencil(lin.K, lin.M, mesh.constrained)
    w, V = MR.eigh_free(Kf, Mf)
    n_modes, n_rigid = c["n_modes"], MR.rigid_count(name)
    m = n_modes + max(2, n_modes // 4)
    assert m <= len(free) and 3 * m <= 60
    top = w[n_modes - 1]
    gap, spread = MR.condition(w, n_modes, n_rigid)
    print("%s: %d free dofs, lambda_1 %.4g, lambda_n %.4g, rigid %d, gap %.2e, lambda_max / lambda_n %.3g" %
          (name, len(free), w[n_rigid], top, n_rigid, gap, spread))
    assert n_rigid < n_modes
    assert np.all(np.abs(w[:n_rigid]) <= 1e-9 * top) and w[n_rigid] > 1e-4 * top
    assert gap >= 1e-3
    assert EPS * spread <= 1e-10
    assert np.all(MR.gaps(w, n_modes, n_rigid) >= 1e-3 * top)
    assert np.abs(V.T @ Mf @ V - np.eye(len(free))).max() <= 1e-10
