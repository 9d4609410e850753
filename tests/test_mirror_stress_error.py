"""CPU anchor of tests/golden/stress_error_reference.py, the numpy reference the device's stress error indicator
(mi_stress_error) is held to by test_gpu_stress_error.py.  No device, no library:

  (1) a homogeneous deformation u = A x is reproduced exactly by Q_p on box and perturbed meshes, the raw stress is the same
      tensor at every point and the lumped projection returns it at every node: eta <= 1e-13 n, both models
  (2) model 1: n^2 = u^T K u with K of mirror.Linear (the same rule), to 1e-12 -- m is the complementary energy density
  (3) conditioning of the reference itself: the sums carried in np.longdouble (sigma* included) lie within 1e-14 of
      sqrt(eta_K^2 + n_K^2) of the float64 reference, per cell, on every case of the GPU file
  (4) decay: on a smooth field, interpolated at the nodes, halving h divides eta by a factor inside [0.75 2^p, 1.25 2^p]:
      2D Q1 8^2 -> 16^2, Q2 6^2 -> 12^2, Q3 4^2 -> 8^2, and 3D Q2 2^3 -> 4^3, both models (the recovered field is
      superconvergent on these boxes: one order more than the raw stress's h^p)
  (5) effectivity: at the finer mesh of each 2D pair, model 1, eta / true error lies within [0.3, 2], the true error being
      the same norm of sigma_exact - sigma_h with sigma_exact from the field's analytic gradient.  The field is the nodal
      interpolant, not a Galerkin solution: an indicator, no guaranteed bound
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import stress_cases as SC  # noqa: E402
import stress_error_cases as EC  # noqa: E402
import stress_error_reference as R  # noqa: E402
import stress_reference as S  # noqa: E402

MU, NU = SC.MU, SC.NU
A0 = {2: np.array([[0.08, 0.05], [-0.03, -0.06]]),
      3: np.array([[0.08, 0.05, -0.02], [-0.03, -0.06, 0.04], [0.01, -0.06, 0.03]])}
AMP = 0.01


# ------------------------------------------------------------------ (1)
@pytest.mark.parametrize("model", [S.NEOHOOKE, S.LINEAR])
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [(2, 1, (3, 2)), (2, 3, (3, 2)), (3, 2, (2, 2, 2)), (3, 3, (2, 2, 2))])
def test_homogeneous_deformation_has_no_error(mesh, perturbed, model):
    c = SC.case(*mesh, perturbed)
    m = c["mesh"]
    u = (m.coords @ A0[m.dim].T).reshape(-1)
    r = R.stress_error(m, u, MU, NU, model)
    print("eta %.2e of n = %.4e" % (r["error"] / r["norm"], r["norm"]))
    assert r["norm"] > 0 and r["error"] <= 1e-13 * r["norm"]
    assert r["relative"] <= 1e-13


def test_zero_state_gives_zeros():
    c = SC.case(2, 2, (3, 2), True)
    r = R.stress_error(c["mesh"], np.zeros(c["mesh"].n), MU, NU, S.LINEAR)
    assert r["error"] == 0 and r["norm"] == 0 and r["relative"] == 0 and r["max_cell"] == 0
    assert not np.isnan(r["eta_cell"]).any()


# ------------------------------------------------------------------ (2)
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [(2, 1, (3, 2)), (2, 3, (3, 2)), (3, 1, (2, 2, 2)), (3, 2, (3, 2, 2))])
def test_norm_is_the_strain_energy_of_the_linear_model(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    L = Mi.Linear(c["mesh"], mu=MU, nu=NU)
    want = c["u"] @ L.K @ c["u"]
    got = EC.ref(c, S.LINEAR)["norm"] ** 2
    print("n^2 %.12e  u^T K u %.12e" % (got, want))
    assert abs(got - want) <= 1e-12 * want


# ------------------------------------------------------------------ (3)
@pytest.mark.parametrize("mesh,perturbed,model", EC.ALL_CASES)
def test_reference_is_well_conditioned(mesh, perturbed, model):
    c = EC.case(*mesh, perturbed)
    r = EC.ref(c, model)
    ld = R.stress_error(c["mesh"], c["u"], MU, NU, model, dtype=np.longdouble, pts=EC.points(c, model))
    scale = np.sqrt(ld["eta2_cell"] + ld["n2_cell"])
    assert scale.min() > 0
    ee, en = np.abs(ld["eta_cell"] - r["eta_cell"]) / scale, np.abs(ld["norm_cell"] - r["norm_cell"]) / scale
    print("eta_K %.2e  n_K %.2e of sqrt(eta_K^2 + n_K^2); smallest eta_K / scale %.3f" % (ee.max(), en.max(),
                                                                                       float((r["eta_cell"] / scale).min())))
    assert ee.max() <= 1e-14 and en.max() <= 1e-14
    assert abs(ld["error"] - r["error"]) <= 1e-14 * np.sqrt(ld["error"] ** 2 + ld["norm"] ** 2)
    assert ld["max_cell"] == r["max_cell"]


# ------------------------------------------------------------------ (4), (5)
def _field(dim, X):
    x, y = X[:, 0], X[:, 1]
    if dim == 2:
        return AMP * np.stack([np.sin(2 * x) * np.cos(2 * y + 0.3), np.cos(2 * x + 0.2) * np.sin(3 * y)], axis=1)
    z = X[:, 2]
    return AMP * np.stack([np.sin(2 * x) * np.cos(2 * y + 0.3) * np.cos(z), np.cos(2 * x + 0.2) * np.sin(3 * y) * np.sin(z + 0.1),
                           np.sin(x + y) * np.cos(2 * z)], axis=1)


def _gradient_2d(x, y):
    return AMP * np.array([[2 * np.cos(2 * x) * np.cos(2 * y + 0.3), -2 * np.sin(2 * x) * np.sin(2 * y + 0.3)],
                           [-2 * np.sin(2 * x + 0.2) * np.sin(3 * y), 3 * np.cos(2 * x + 0.2) * np.cos(3 * y)]])


_smooth = {}


def _smooth_run(dim, p, n, model):
    key = (dim, p, n, model)
    if key not in _smooth:
        m = Mi.Mesh(dim, p, (n,) * dim, (0.0,) * dim, (1.0,) * dim, [0] * (2 * dim))
        u = _field(dim, m.coords).reshape(-1)
        pts = S.points(m, u, MU, NU, model)
        _smooth[key] = (m, pts, R.stress_error(m, u, MU, NU, model, pts=pts))
    return _smooth[key]


@pytest.mark.parametrize("model", [S.NEOHOOKE, S.LINEAR])
@pytest.mark.parametrize("dim,p,n", [(2, 1, 8), (2, 2, 6), (2, 3, 4), (3, 2, 2)])
def test_eta_decays_with_h(dim, p, n, model):
    coarse, fine = _smooth_run(dim, p, n, model)[2]["error"], _smooth_run(dim, p, 2 * n, model)[2]["error"]
    print("%dD Q%d model %d: eta %.4e -> %.4e, factor %.3f (2^p = %d)" % (dim, p, model, coarse, fine, coarse / fine, 2 ** p))
    assert 0.75 * 2 ** p <= coarse / fine <= 1.25 * 2 ** p


@pytest.mark.parametrize("p,n", [(1, 16), (2, 12), (3, 8)])
def test_effectivity_against_the_exact_stress(p, n):
    m, pts, r = _smooth_run(2, p, n, S.LINEAR)
    rule = S._rule(2, p, p + 1)
    true2 = 0.0
    for k, (conn, N, s, JxW, _) in enumerate(pts):
        verts = m.cells[k // len(rule)][1]
        x = Mi.q1_map(2, verts, rule[k % len(rule)][0])
        exact = S.point_stress(2, MU, NU, _gradient_2d(x[0], x[1]), S.LINEAR)[0]
        true2 += R.metric(2, MU, NU, np.array([exact[d, e] for d, e in S.PAIRS[2]]) - s) * JxW
    ratio = r["error"] / np.sqrt(true2)
    print("2D Q%d %d^2: eta %.4e, true error %.4e, effectivity %.3f" % (p, n, r["error"], np.sqrt(true2), ratio))
    assert 0.3 <= ratio <= 2.0
