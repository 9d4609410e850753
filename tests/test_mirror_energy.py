"""CPU anchor of tests/golden/energy_reference.py, the numpy reference the device's energy diagnostics are held to
(test_gpu_energy.py).  No device, no library:

  (a) psi() equals the oracle's Psi (orc_material, written from compressible_neo_hook_material.h:30-35, 62-72) on random F
  (b) the strain energy is the potential of the mirror's residual: dW/du . d by central differences equals -rhs . d with rhs
      from mirror.Solid.assemble at zero acceleration, body force and traction.  The difference quotient's error is
      truncation, ~eps^2 (3e-8 at eps = 1e-5, 3e-10 at 1e-6 on these meshes): gate 1e-6 at eps = 1e-5
  (c) kinetic = 1/2 v^T M v with mirror.Linear's consistent mass, and the linear strain energy 1/2 u^T K u equals the
      integral of lambda/2 tr(eps)^2 + mu eps : eps point by point
  (d) a rigid translation stores nothing: |strain| <= 1e-12 mu volume
"""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import energy_reference as E  # noqa: E402
import mirror as Mi  # noqa: E402

MU, NU, RHO = 0.7e6, 0.3, 870.0
ROLES = {2: [1, 7, 0, 7], 3: [1, 7, 0, 7, 8, 0]}
_cache = {}


def _mesh(dim, perturbed=True):
    """Q2 3 x 2 x 2 (3D) or 3 x 2 (2D), vertices moved by 0.1 h"""
    key = (dim, perturbed)
    if key not in _cache:
        reps = (3, 2, 2)[:dim]
        hi = tuple(0.1 * r for r in reps)
        rng = np.random.default_rng(7 + dim)
        nv = int(np.prod([r + 1 for r in reps]))
        perturb = 0.1 * 0.1 * rng.uniform(-1, 1, (nv, dim)) if perturbed else None
        _cache[key] = Mi.Mesh(dim, 2, reps, (0.0,) * dim, hi, ROLES[dim], perturb=perturb)
    return _cache[key]


def _state(m, amp, seed):
    rng = np.random.default_rng(seed)
    u = amp * rng.standard_normal(m.n) * ~m.constrained
    return u, rng.standard_normal(m.n)


@pytest.mark.parametrize("dim", [2, 3])
def test_psi_equals_the_oracle(dim):
    rng = np.random.default_rng(dim)
    for _ in range(20):
        F = np.eye(dim) + 0.3 * rng.uniform(-1, 1, (dim, dim))
        assert np.linalg.det(F) > 0.1
        ref = O.material(dim, MU, NU, F)[0]
        assert abs(E.psi(dim, MU, NU, F) - ref) <= 1e-13 * abs(ref)


@pytest.mark.parametrize("dim", [2, 3])
def test_strain_energy_is_the_potential_of_the_residual(dim):
    m = _mesh(dim)
    u, _ = _state(m, 0.002, 11)
    assert E.energies(m, u, 0 * u, MU, NU, RHO)[3] >= 0.4
    S = Mi.Solid(m, mu=MU, nu=NU, rho=RHO)
    S.u = u
    _, rhs = S.assemble(np.zeros(m.n))
    d = np.random.default_rng(12).standard_normal(m.n) * ~m.constrained
    d *= np.abs(u).max() / np.abs(d).max()
    eps = 1e-5
    Wp = E.energies(m, u + eps * d, 0 * u, MU, NU, RHO)[0]
    Wm = E.energies(m, u - eps * d, 0 * u, MU, NU, RHO)[0]
    dW = (Wp - Wm) / (2 * eps)
    assert abs(dW + rhs @ d) <= 1e-6 * abs(rhs @ d), (dW, rhs @ d)


@pytest.mark.parametrize("dim", [2, 3])
def test_kinetic_and_linear_strain_are_the_quadratic_forms(dim):
    body = (0.3, -9.81, 1.0)[:dim]
    for perturbed in (False, True):
        m = _mesh(dim, perturbed)
        u, v = _state(m, 0.002, 13)
        L = Mi.Linear(m, MU, NU, RHO, body)
        # boxes: QGauss(p + 1) and QGauss(p + 2) both integrate N_a N_b exactly; moved vertices: the linear model's own rule
        _, kin, pot, _ = E.energies(m, u, v, MU, NU, RHO, body, nq=None if not perturbed else 3)
        ls, lk, lb = E.linear_energies(L, u, v)
        assert abs(kin - lk) <= 1e-13 * lk
        assert abs(pot - lb) <= 1e-13 * RHO * np.linalg.norm(body) * np.abs(u).max() * E.volume(m)
        assert abs(ls - E.linear_strain_pointwise(m, u, MU, NU)) <= 1e-13 * ls


@pytest.mark.parametrize("dim", [2, 3])
def test_rigid_translation_stores_nothing(dim):
    m = _mesh(dim)
    u = np.tile(np.array([0.013, -0.021, 0.008])[:dim], m.nnodes)
    strain, _, _, det = E.energies(m, u, 0 * u, MU, NU, RHO)
    assert abs(det - 1) < 1e-12
    assert abs(strain) <= 1e-12 * MU * E.volume(m)
