"""CPU anchor of tests/golden/stress_reference.py, the numpy reference the device's nodal stress recovery is held to
(test_gpu_stress_field.py).  No device, no library:

  (1) tau of mirror.material equals (dPsi/dF) F^T by central differences of energy_reference.psi, 2D and 3D; step 1e-5 and
      gate 1e-6 as the derivative identity of test_mirror_energy.py (truncation ~eps^2)
  (2) a homogeneous deformation u = (F0 - I) X is reproduced exactly by Q_p on box and perturbed meshes (X(xi) is d-linear), so
      EVERY node has sigma_i = tau(F0)/det F0 (model 0) or lambda tr(eps0) I + 2 mu eps0 (model 1), to 1e-12 of max|sigma|: a
      known answer that does not depend on the projection
  (3) sum_i W_i = volume and sum_i W_i sigma_i = sum over cells and points of sigma JxW, both to 1e-13 (the stress sums: of their
      largest component; they are signed sums of a few thousand terms, the shape functions sum to one)
  (4) 3D boxes: for u -> eps u the distance between model 0 and model 1 falls as eps^2 (lambda = kappa - 2 mu / 3 in 3D, and both
      rules integrate N_i times the linear stress exactly on boxes): ratio in [50, 200] for a factor 10 in eps
  (5) conditioning of the reference itself: the same sums carried in np.longdouble lie within 1e-13 max|sigma| of the float64
      reference on every case of the GPU file -- a condition on the INPUTS that keeps the device's 1e-12 meaningful
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import energy_reference as E  # noqa: E402
import mirror as Mi  # noqa: E402
import stress_cases as SC  # noqa: E402
import stress_reference as S  # noqa: E402

MU, NU = SC.MU, SC.NU
F0 = {2: np.array([[1.08, 0.05], [-0.03, 0.94]]),
      3: np.array([[1.08, 0.05, -0.02], [-0.03, 0.94, 0.04], [0.01, -0.06, 1.03]])}


def _flat(dim, s):
    return np.array([s[d, e] for d, e in S.PAIRS[dim]])


@pytest.mark.parametrize("dim", [2, 3])
def test_tau_is_the_derivative_of_psi(dim):
    rng = np.random.default_rng(dim)
    eps = 1e-5
    for _ in range(10):
        F = np.eye(dim) + 0.3 * rng.uniform(-1, 1, (dim, dim))
        assert np.linalg.det(F) > 0.1
        P = np.zeros((dim, dim))
        for i in range(dim):
            for j in range(dim):
                dF = np.zeros((dim, dim))
                dF[i, j] = eps
                P[i, j] = (E.psi(dim, MU, NU, F + dF) - E.psi(dim, MU, NU, F - dF)) / (2 * eps)
        tau = Mi.material(dim, MU, NU, F)[0]
        assert np.abs(P @ F.T - tau).max() <= 1e-6 * np.abs(tau).max()


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1], SC.GENERIC_MESHES[2]])
def test_homogeneous_deformation_is_a_known_answer(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    H = F0[dim] - np.eye(dim)
    u = (m.coords @ H.T).reshape(-1)
    for model in (S.NEOHOOKE, S.LINEAR):
        want = _flat(dim, S.point_stress(dim, MU, NU, H, model)[0])
        sigma, vm, _, det = S.nodal_stress(m, u, MU, NU, model)
        if model == S.NEOHOOKE:
            assert abs(det - np.linalg.det(F0[dim])) <= 1e-12
        assert np.abs(sigma - want[None, :]).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(vm - S.von_mises(dim, want[None, :])[0]).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[1], SC.Q3_MESHES[0], SC.GENERIC_MESHES[3]])
def test_weights_sum_to_the_volume_and_carry_the_mean_stress(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    vol = E.volume(c["mesh"])
    for model in (S.NEOHOOKE, S.LINEAR):
        sigma, _, W, _ = SC.ref(c, model)
        assert W.min() > 0
        assert abs(W.sum() - vol) <= 1e-13 * vol
        mean = S.mean_stress(c["mesh"], c["u"], MU, NU, model)
        assert np.abs((W[:, None] * sigma).sum(axis=0) - mean).max() <= 1e-13 * np.abs(mean).max()


@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0]])
def test_models_agree_to_second_order(mesh):
    c = SC.case(*mesh, False)
    dist = []
    for eps in (1e-3, 1e-4):
        s0 = S.nodal_stress(c["mesh"], eps * c["u"], MU, NU, S.NEOHOOKE)[0]
        s1 = S.nodal_stress(c["mesh"], eps * c["u"], MU, NU, S.LINEAR)[0]
        dist.append(np.abs(s0 - s1).max())
    assert 50 <= dist[0] / dist[1] <= 200, dist


@pytest.mark.parametrize("mesh,perturbed,model", SC.REFERENCE_CASES + SC.TEAM_CASES)
def test_reference_is_well_conditioned(mesh, perturbed, model):
    c = SC.case(*mesh, perturbed)
    sigma, vm, W, det = SC.ref(c, model)
    assert det >= 0.4 and W.min() > 0
    ld = S.nodal_stress(c["mesh"], c["u"], MU, NU, model, dtype=np.longdouble, pts=SC.points(c, model))
    smax = np.abs(sigma).max()
    print("sigma %.2e  von Mises %.2e  W %.2e (of max|sigma|, of itself, of itself)" % (
        np.abs(ld[0] - sigma).max() / smax, np.abs((ld[1] - vm) / vm).max(), np.abs((ld[2] - W) / W).max()))
    assert np.abs(ld[0] - sigma).max() <= 1e-13 * smax
