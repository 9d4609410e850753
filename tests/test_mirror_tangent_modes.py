"""CPU anchor of tests/golden/tangent_modes_reference.py: what the modal analysis of the tangent (mi_tangent_modes) computes, and
the conditions under which the assertions of tests/test_gpu_tangent_modes.py are derived, on the cases it runs.  No device, no
library: K_T = mirror.Solid.assemble - alpha_1 rho M, dense eigh on the free pencil.

  * 3D box meshes: the free-free block of K_T(0) equals mirror.Linear.K to 1e-13 of its largest entry, and the eigenvalues equal
    the linear model's within the dense solver's own error 2 n eps lambda_max plus Weyl's bound for the matrix difference
  * 2D: K_T(0) is NOT the linear K (the 2 x 2 neo-Hookean formulation against plane strain): the difference is recorded
  * a stretched beam raises lambda_0, the compressed strip has lambda_0 < 0
  * A_ff = (K_T + alpha_1 rho M)_ff is positive definite on every case and state (Cholesky): lambda_min > -alpha_1
  * K_T x formed as A x - alpha_1 rho M x: its measured error (float64 against long double) lies within
    tangent_modes_reference.floor(), and that bound is <= 1e-9 of the stopping rule's scale on every case:
    a decade below tol = 1e-8 (the long rows of Q3 and Q4 make it 6e-10; what is measured is 5e-13)
  * clusters and gaps: no cluster is cut by n_modes, every cluster is >= 1e-3 lambda_top away from its neighbours, and the dense
    reference's own error n eps (lambda_max + alpha_1) is <= 1e-4 of the smallest gap.  The square beam has double modes

Measured here (printed by the tests):
  q2_311 zero     lambda 27.392 27.392 548.37 814.35 814.35     stretch 284.29 284.29 1354.5 2730.3 2730.3
  2d_q2_61 zero   lambda_0 1.3525   stretch 59.967   compress -4941.1
  |K_T(0) - K_lin| / max |K_lin| on the free dofs: 3D <= 3e-15, 2d_q2_61 5.3e-2
"""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import tangent_modes_cases as TC  # noqa: E402
import tangent_modes_reference as TR  # noqa: E402

EPS = np.finfo(np.float64).eps
_pencils, _eigs = {}, {}


def _pencil(name, kind):
    if (name, kind) not in _pencils:
        _pencils[name, kind] = TR.mirror_pencil(name, kind)
    return _pencils[name, kind]


def _eig(name, kind):
    if (name, kind) not in _eigs:
        _, Mf, Kf, _ = _pencil(name, kind)
        _eigs[name, kind] = TR.eigh_free(0.5 * (Kf + Kf.T), Mf)
    return _eigs[name, kind]


@pytest.mark.parametrize("name", ["q2_311", "q1_422"])
def test_unloaded_tangent_is_the_linear_model_in_3d(name):
    mesh = TC.case_mesh(name)
    _, Mf, Kf, free = _pencil(name, "zero")
    lin = Mi.Linear(mesh)
    Kl, Ml, _ = TR.free_pencil(lin.K, lin.M, mesh.constrained)
    dk = np.abs(Kf - Kl).max() / np.abs(Kl).max()
    dm = np.abs(Mf - Ml).max() / np.abs(Ml).max()
    w, wl = _eig(name, "zero")[0], TR.eigh_free(Kl, Ml)[0]
    k = TC.CASES[name]["n_modes"]
    bound = 2 * len(free) * EPS * w[-1] + np.linalg.norm(Kf - Kl, 2) / np.linalg.eigvalsh(Mf)[0]
    print("%s: |K_T(0) - K| / max |K| %.2e, mass %.2e, lambda %s, linear %s, bound %.2e" % (name, dk, dm, w[:k], wl[:k], bound))
    assert dk <= 1e-13 and dm <= 1e-13
    assert np.all(np.abs(w[:k] - wl[:k]) <= bound)


def test_unloaded_tangent_in_2d_differs_from_plane_strain():
    name = "2d_q2_61"
    mesh = TC.case_mesh(name)
    Kf = _pencil(name, "zero")[2]
    Kl = TR.free_pencil(Mi.Linear(mesh).K, np.eye(mesh.n), mesh.constrained)[0]
    d = np.abs(Kf - Kl).max() / np.abs(Kl).max()
    print("%s: |K_T(0) - K| / max |K| %.3e" % (name, d))
    assert 1e-2 < d < 1e-1


def test_load_moves_the_spectrum():
    beam = {kind: _eig("q2_311", kind)[0][:4] for kind in ("zero", "stretch")}
    strip = {kind: _eig("2d_q2_61", kind)[0][0] for kind in ("zero", "stretch", "compress")}
    print("q2_311: zero %s, stretch %s; 2d_q2_61 lambda_0: %s" % (beam["zero"], beam["stretch"], strip))
    # the figures this feature was motivated with, to their printed digits
    assert np.allclose(beam["zero"], [27.392, 27.392, 548.37, 814.35], rtol=2e-5)
    assert np.allclose(beam["stretch"], [284.29, 284.29, 1354.5, 2730.3], rtol=4e-5)
    assert beam["stretch"][0] > 10 * beam["zero"][0]
    assert abs(strip["zero"] - 1.35) < 5e-3 and abs(strip["stretch"] - 60.0) < 0.05 and abs(strip["compress"] + 4941) < 1.0
    assert strip["compress"] < 0 and -strip["compress"] < TC.ALPHA1


@pytest.mark.parametrize("name,kind", TC.RUNS, ids=["%s-%s" % r for r in TC.RUNS])
def test_conditions_of_the_device_test(name, kind):
    c = TC.CASES[name]
    Af, Mf, Kf, free = _pencil(name, kind)
    w, V = _eig(name, kind)
    k = c["n_modes"]
    m = k + max(2, k // 4)
    assert m <= len(free) and 3 * m <= 60
    sla.cholesky(0.5 * (Af + Af.T))  # raises where A_ff is not positive definite
    assert w[0] > -TC.ALPHA1
    top = np.abs(w[:k]).max()
    # the floor of K_T x as a difference, on the wanted eigenvectors
    X = V[:, :k]
    bound = TR.floor(Af, Mf, X, top)
    ld = np.longdouble
    exact = (Af.astype(ld) @ X.astype(ld) - ld(TC.ALPHA1) * (Mf.astype(ld) @ X.astype(ld))).astype(np.float64)
    formed = Af @ X - TC.ALPHA1 * (Mf @ X)
    measured = np.linalg.norm(formed - exact, axis=0) / (top * np.linalg.norm(Mf @ X, axis=0))
    # clusters and gaps
    gap, of = TR.gaps(w, k)
    e_ref = len(free) * EPS * (w[-1] + TC.ALPHA1)
    print("%s %s: %d free dofs, lambda %s, clusters %s, min gap / top %.2e, lambda_max / top %.3g, floor measured %.2e bound %.2e, "
          "eps alpha_1 / top %.2e, e_ref / gap %.2e" % (name, kind, len(free), w[:k], TR.clusters(w, k), gap.min() / top, w[-1] / top,
                                                       measured.max(), bound.max(), EPS * TC.ALPHA1 / top, e_ref / gap.min()))
    assert np.all(measured <= bound) and np.all(bound <= 1e-9)
    assert all(b <= k for a, b in TR.clusters(w, k))  # n_modes cuts no cluster
    assert np.all(gap >= 1e-3 * top)
    assert e_ref <= 1e-4 * gap.min()
    assert np.abs(V.T @ Mf @ V - np.eye(len(free))).max() <= 1e-9
    if name == "q2_311":
        assert TR.clusters(w, k) == [(0, 2), (2, 3), (3, 5)]
