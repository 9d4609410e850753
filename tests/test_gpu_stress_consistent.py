"""GPU: the consistent stress recovery (tuning "stress_projection" 1: M sigma*_k = b_k with the consistent mass, in place of the
lumped b_i / W_i) against tests/golden/stress_points_reference.consistent, the dense numpy solve anchored by
test_mirror_stress_points.py.

Cases: one box and one perturbed mesh of tests/golden/stress_cases.py per kernel form (stress_q3 / mass_apply_q3, stress_q2 /
mass_apply_q2, stress_cells / mass_apply_cells in 2D and 3D), both models, the random admissible state.

Bounds.  sigma* against the dense solve: kappa_2(M) (1e-13 + 64 eps) max|sigma*| per entry -- the form of test_gpu_mass.py's bound
with the solve's fixed tolerance 1e-13 for the residual, 64 eps for the dense solve's own.  Model 0: eta(key 1) <= eta(key 0)
(1 + 1e-10), derived, not measured: M, b and mi_stress_error's eta share QGauss(p + 2) and the metric m(.) is constant, so the
consistent sigma* minimises eta over ALL nodal fields, the lumped one among them.  Everything else is bits.
"""
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import point_eval_cases as PC  # noqa: E402
import point_eval_reference as PE  # noqa: E402
import stress_cases as SC  # noqa: E402
import stress_points_reference as SP  # noqa: E402
import stress_reference as S  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

MU, NU, RHO = SC.MU, SC.NU, SC.RHO
CASES = [(SC.Q3_MESHES[0], False), (SC.Q3_MESHES[1], True), (SC.Q2_MESHES[0], False), (SC.Q2_MESHES[1], True),
         (SC.GENERIC_MESHES[1], False), (SC.GENERIC_MESHES[2], True), (SC.GENERIC_MESHES[4], False), (SC.GENERIC_MESHES[5], True)]
MODELS = (M.STRESS_NEOHOOKE, M.STRESS_LINEAR)


def _context(c, **kw):
    fr = list(c["roles"]) + [0] * (6 - len(c["roles"]))
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=(0.0,) * c["dim"], hi=c["hi"], face_role=fr, mu=MU, nu=NU,
                  rho=RHO, perturb=c["perturb"], **kw)
    assert G.n == c["mesh"].n and np.array_equal(G.constrained, c["mesh"].constrained)
    return G


def _loaded(c, **kw):
    G = _context(c, **kw)
    G.set(M.V_U, c["u"])
    return G


def _bits(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got)


@pytest.mark.parametrize("mesh,perturbed", CASES)
def test_consistent_projection_against_the_dense_solve(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    G = _loaded(c)
    assert G.get_tuning("stress_projection") == 0 and G.get_tuning("stress_projection_its") == 0
    lumped = {model: G.stress_field(model) for model in MODELS}
    eta0 = G.stress_error()["error"]
    assert G.get_tuning("stress_projection_its") == 0
    G.set_tuning("stress_projection", 1)
    assert G.get_tuning("stress_projection") == 1
    for model in MODELS:
        ref, _, W, Md = SP.consistent(m, c["u"], MU, NU, model)
        ev = np.linalg.eigvalsh(Md)
        bound = ev[-1] / ev[0] * (1e-13 + 64 * SP.EPS)
        sigma, vm, w = G.stress_field(model)
        its = G.get_tuning("stress_projection_its")
        err = np.abs(sigma - ref).max() / np.abs(ref).max()
        moved = np.abs(sigma - lumped[model][0]).max() / np.abs(ref).max()
        print("model %d: kappa_2 %.1f, %d iterations, |sigma* - dense| %.2e of max|sigma*| = %.3f of the bound; lumped is %.1e away" %
              (model, ev[-1] / ev[0], its, err, err / bound, moved))
        assert its > 0
        assert err <= bound
        assert moved > 1e-6  # (the random state's stress is not in the nodal space: the two projections differ)
        assert np.abs(vm - S.von_mises(dim, sigma)).max() <= 1e-12 * np.abs(ref).max()  # von Mises of the solved tensor
        assert w.tobytes() == lumped[model][2].tobytes()  # weight stays W_i
        assert _bits(G.stress_field(model)) == _bits((sigma, vm, w))
    # the error indicator and the interpolation read the same nodal array
    eta1 = G.stress_error()["error"]
    print("eta: lumped %.6e, consistent %.6e" % (eta0, eta1))
    assert eta1 <= eta0 * (1 + 1e-10)
    sigma = G.stress_field()[0]
    cells, xi = PC.interior_pairs(m, 33, np.random.default_rng(21))
    r = G.evaluate_stress(PE.points(m, cells, xi), kind=M.STRESS_AT_RECOVERED)
    assert np.abs(r["sigma"] - SP.interpolate(m, sigma, cells, xi)).max() <= 1e-12 * np.abs(sigma).max()
    G.close()


@pytest.mark.parametrize("mesh,perturbed", [CASES[1], CASES[3], CASES[5]])
def test_key_back_to_zero_gives_the_bits_of_a_context_that_never_saw_it(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m = c["mesh"]
    X = PE.points(m, *PC.interior_pairs(m, 33, np.random.default_rng(22)))
    G, H = _loaded(c), _loaded(c)
    G.set_tuning("stress_projection", 1)
    for model in MODELS:
        G.stress_field(model)
    G.stress_error()
    assert G.get_tuning("stress_projection_its") > 0
    G.set_tuning("stress_projection", 0)
    assert G.get_tuning("stress_projection") == 0 and G.get_tuning("stress_projection_its") == 0
    for model in MODELS:
        assert _bits(G.stress_field(model)) == _bits(H.stress_field(model))
        eg, eh = G.stress_error(model), H.stress_error(model)
        assert all(np.array_equal(eg[k], eh[k]) for k in eg)
        rg = G.evaluate_stress(X, model=model, kind=M.STRESS_AT_RECOVERED)
        rh = H.evaluate_stress(X, model=model, kind=M.STRESS_AT_RECOVERED)
        assert rg["sigma"].tobytes() == rh["sigma"].tobytes() and rg["von_mises"].tobytes() == rh["von_mises"].tobytes()
    G.close()
    H.close()


def test_setter_is_refused_on_a_team_and_bad_values():
    c = SC.case(*SC.TEAM_MESHES[0], True)
    T = _loaded(c, slabs=2)
    assert T.comm_info()[0] == 2
    want = T.stress_field()
    with pytest.raises(M.MiError) as err:
        T.set_tuning("stress_projection", 1)
    assert err.value.code == M.MI_EINVAL and "undecomposed" in str(err.value)
    assert T.get_tuning("stress_projection") == 0
    T.set_tuning("stress_projection", 0)
    assert _bits(T.stress_field()) == _bits(want)
    T.close()
    G = _loaded(SC.case(*SC.GENERIC_MESHES[0], False))
    for bad in (-1, 2):
        with pytest.raises(M.MiError):
            G.set_tuning("stress_projection", bad)
    assert G.get_tuning("stress_projection") == 0
    G.close()


@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1]])
def test_the_solve_leaves_a_following_step_alone(mesh):
    c = SC.case(*mesh, True)
    G, H = _context(c), _context(c)
    for Y in (G, H):
        Y.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        Y.newmark_step(tol_lin=1e-10)
    vecs = [G.get(w) for w in range(10)]
    G.set_tuning("stress_projection", 1)
    for model in MODELS:
        G.stress_field(model)
    G.stress_error()
    assert G.get_tuning("stress_projection_its") > 0
    for w in range(10):
        assert np.array_equal(vecs[w], G.get(w)), w
    _, ig = G.newmark_step(tol_lin=1e-10)
    _, ih = H.newmark_step(tol_lin=1e-10)
    assert bytes(ig) == bytes(ih)
    for w in range(10):
        assert np.array_equal(G.get(w), H.get(w)), w
    G.close()
    H.close()
    G, H = _context(c), _context(c)  # the linear model
    for Y in (G, H):
        Y.linear_setup(0.5)
        Y.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        Y.linear_step(1, 1e-12)
    G.set_tuning("stress_projection", 1)
    G.stress_field(M.STRESS_LINEAR)
    assert G.linear_step(1, 1e-12) == H.linear_step(1, 1e-12)
    for w in range(10):
        assert np.array_equal(G.get(w), H.get(w)), w
    G.close()
    H.close()
