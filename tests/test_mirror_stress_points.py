"""CPU anchor of tests/golden/stress_points_reference.py, the numpy reference mi_evaluate_stress, mi_principal_stress and the
consistent stress recovery are held to (test_gpu_stress_points.py, test_gpu_stress_consistent.py).  No device, no library:

  (1) an affine field u = A X + b has the same gradient at every point of every mesh, box or perturbed (X(xi) is d-linear), so
      raw() gives ONE tensor everywhere: material(I + A) / det (model 0) or Hooke's law (model 1) in closed form, to 1e-12 of
      max|sigma|; interpolate() of that constant nodal field gives it back
  (2) raw() at the rule's points pushed through sum N_i sigma JxW / W_i is stress_reference.nodal_stress, to 1e-13 of max|sigma|
      (the same sums from the same point values in another order)
  (3) consistent(): M sigma* = b has the residual of a dense solve; sum_i b_i = sum_i (M sigma*)_i = the mean stress integral
      (the basis sums to one); on a state whose raw stress lies in the nodal space -- the affine field -- it equals the lumped field
  (4) the Jacobi mirror's eigenpairs: values against numpy.linalg.eigvalsh to 16 eps |sigma|_F, vectors measured against the
      tensor alone.  The worst figures of the mirror on the GPU test's tensors are printed; test_gpu_stress_points.py gates the
      device at 8 x SP.MIRROR_EIG_RES / SP.MIRROR_EIG_ORTH, which this test holds to be upper bounds of what it measures:
          measured   residual 1.61 (3D) 0.86 (2D)   trace 1.64 (3D) 0.93 (2D)   orthonormality 6.00 (3D) 1.00 (2D)
          recorded   MIRROR_EIG_RES 1.65 (residual and trace)   MIRROR_EIG_ORTH 6.0
      in units of eps |sigma|_F (orthonormality: eps)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import point_eval_cases as PC  # noqa: E402
import stress_cases as SC  # noqa: E402
import stress_points_reference as SP  # noqa: E402
import stress_reference as S  # noqa: E402

MU, NU = SC.MU, SC.NU
MESHES = [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1], SC.GENERIC_MESHES[4]]


def _flat(dim, s):
    return np.array([s[d, e] for d, e in S.PAIRS[dim]])


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_affine_field_has_one_tensor_everywhere(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    A = 0.05 * PC.Affine(dim, np.random.default_rng(4)).A
    u = (m.coords @ A.T + 0.01).reshape(-1)
    ic, ixi = PC.interior_pairs(m, 20, np.random.default_rng(1))
    bc, bxi = PC.boundary_pairs(m)
    cells, xi = np.concatenate([ic, bc]), np.concatenate([ixi, bxi])
    for model in (S.NEOHOOKE, S.LINEAR):
        want = _flat(dim, S.point_stress(dim, MU, NU, A, model)[0])
        got, det = SP.raw(m, u, MU, NU, model, cells, xi)
        err = np.abs(got - want[None, :]).max() / np.abs(want).max()
        back = SP.interpolate(m, np.tile(want, (m.nnodes, 1)), cells, xi)
        print("model %d: raw %.2e, interpolated %.2e of max|sigma|" % (model, err, np.abs(back - want).max() / np.abs(want).max()))
        assert err <= 1e-12 and np.abs(back - want[None, :]).max() <= 1e-12 * np.abs(want).max()
        if model == S.NEOHOOKE:
            assert np.abs(det - np.linalg.det(np.eye(dim) + A)).max() <= 1e-12


@pytest.mark.parametrize("model", [S.NEOHOOKE, S.LINEAR])
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_raw_at_the_rule_projects_to_the_nodal_reference(mesh, perturbed, model):
    c = SC.case(*mesh, perturbed)
    m = c["mesh"]
    ref = SC.ref(c, model)
    cells, xi, N, JxW = SP.quadrature_pairs(m, model)
    got = SP.lumped(m, cells, SP.raw(m, c["u"], MU, NU, model, cells, xi)[0], N, JxW)
    err = np.abs(got - ref[0]).max() / np.abs(ref[0]).max()
    print("lumped from raw(): %.2e of max|sigma|" % err)
    assert err <= 1e-13
    assert np.abs(SP.load(m, cells, np.zeros((len(cells), 1)), N, JxW)[1] / ref[2] - 1).max() <= 1e-13


@pytest.mark.parametrize("model", [S.NEOHOOKE, S.LINEAR])
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.GENERIC_MESHES[2]])
def test_consistent_projection_reference(mesh, model):
    c = SC.case(*mesh, True)
    m, dim = c["mesh"], c["dim"]
    sig, b, W, Md = SP.consistent(m, c["u"], MU, NU, model)
    assert np.abs(Md @ sig - b).max() <= 64 * SP.EPS * np.linalg.cond(Md) * np.abs(b).max()
    if model == S.NEOHOOKE:  # (the lumped weight is the mass's row sum where both are on the same rule)
        assert np.abs(Md.sum(axis=1) / W - 1).max() <= 1e-12
    mean = S.mean_stress(m, c["u"], MU, NU, model)
    assert np.abs(b.sum(axis=0) - mean).max() <= 1e-12 * np.abs(mean).max()
    # a stress that lies in the nodal space is reproduced: consistent = lumped = the constant
    A = 0.05 * PC.Affine(dim, np.random.default_rng(4)).A
    u = (m.coords @ A.T).reshape(-1)
    want = _flat(dim, S.point_stress(dim, MU, NU, A, model)[0])
    got = SP.consistent(m, u, MU, NU, model)[0]
    kappa = np.linalg.cond(Md)
    print("kappa_2(M) %.1f, constant field %.2e of max|sigma|" % (kappa, np.abs(got - want).max() / np.abs(want).max()))
    assert np.abs(got - want[None, :]).max() <= 64 * SP.EPS * kappa * np.abs(want).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_jacobi_mirror_eigenpairs(dim):
    T = SP.eig_tensors(dim)
    lam, dirs = SP.principal(dim, T)
    for a, l in zip(T, lam):
        full = SP.full_tensor(dim, a)
        assert np.abs(l - np.linalg.eigvalsh(full)[::-1]).max() <= 16 * SP.EPS * np.linalg.norm(full)
    res, orth, tr, ordered, signed = SP.eig_figures(dim, T, lam, dirs)
    print("%dD mirror on %d tensors: residual %.2f, trace %.2f eps |sigma|_F, orthonormality %.2f eps" % (dim, len(T), res, tr, orth))
    assert ordered and signed
    assert res <= SP.MIRROR_EIG_RES and tr <= SP.MIRROR_EIG_RES and orth <= SP.MIRROR_EIG_ORTH
    again = SP.principal(dim, T)
    assert again[0].tobytes() == lam.tobytes() and again[1].tobytes() == dirs.tobytes()
    # the degenerate ones get the basis of the statements: the coordinate axes
    for a in T[64:67]:
        l, V = SP.principal(dim, a[None, :])
        assert np.array_equal(V[0], np.eye(dim)) and np.array_equal(l[0], a[:dim])
