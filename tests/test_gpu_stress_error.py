"""GPU: the stress error indicator (mi_stress_error) against tests/golden/stress_error_reference.py, the numpy reference anchored
by test_mirror_stress_error.py.  Cases, material, roles and states: tests/golden/stress_cases.py through stress_error_cases.py.

Tolerances: eta_K and n_K per cell 1e-12 of sqrt(eta_K^2 + n_K^2); eta, n and `relative` 1e-12 of themselves -- the project's
gate for its numpy references; test_mirror_stress_error.py shows the reference's own sums to be good to 1e-14 of that scale on
every case here.  max_cell is exact.  Modes of one context and repeated calls: the same bytes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import stress_cases as SC  # noqa: E402
import stress_error_cases as EC  # noqa: E402
import stress_error_reference as R  # noqa: E402
import stress_reference as S  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

MU, NU, RHO = SC.MU, SC.NU, SC.RHO
BODY = (0.3, -9.81, 1.0)
TOL = 1e-12
COUNTERS = ["count_scalar_allreduce", "count_scalar_allreduce_cg", "count_vector_allreduce", "count_halo_exchange",
            "count_cg_host_sync", "count_cg_iterations", "count_cg_solves", "count_mg_refresh"]
A0 = {2: np.array([[0.08, 0.05], [-0.03, -0.06]]),
      3: np.array([[0.08, 0.05, -0.02], [-0.03, -0.06, 0.04], [0.01, -0.06, 0.03]])}
KEYS = ["error", "norm", "relative", "max_cell_error", "max_cell"]


def _context(c, **kw):
    fr = list(c["roles"]) + [0] * (6 - len(c["roles"]))
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=(0.0,) * c["dim"], hi=c["hi"], face_role=fr, mu=MU, nu=NU,
                  rho=RHO, body_force=BODY, perturb=c["perturb"], **kw)
    assert G.n == c["mesh"].n and np.array_equal(G.constrained, c["mesh"].constrained)
    return G


def _loaded(c, **kw):
    G = _context(c, **kw)
    G.set(M.V_U, c["u"])
    return G


def _check(got, ref, what="", floor=0.0):
    """floor: a lower limit of the per-cell scale as a fraction of the total's, for states that leave cells undeformed (there the
    reference's own numbers are rounding noise of the loaded cells' and the scale means nothing)"""
    scale = np.maximum(np.sqrt(ref["eta2_cell"] + ref["n2_cell"]), floor * np.sqrt(ref["error"] ** 2 + ref["norm"] ** 2))
    assert got["eta_cell"].shape == got["norm_cell"].shape == scale.shape
    ee, en = np.abs(got["eta_cell"] - ref["eta_cell"]) / scale, np.abs(got["norm_cell"] - ref["norm_cell"]) / scale
    et = [abs(got[k] / ref[k] - 1) for k in ("error", "norm", "relative")]
    print("%s eta_K %.2e n_K %.2e of sqrt(eta_K^2 + n_K^2); eta %.2e n %.2e relative %.2e of themselves (gate %.0e); max_cell %d (%d)"
          % (what, ee.max(), en.max(), et[0], et[1], et[2], TOL, got["max_cell"], ref["max_cell"]))
    assert ee.max() <= TOL
    assert en.max() <= TOL
    assert max(et) <= TOL
    assert got["max_cell"] == ref["max_cell"]
    assert got["max_cell_error"] == got["eta_cell"][got["max_cell"]] == got["eta_cell"].max()


def _bits(got):
    return b"".join(np.ascontiguousarray(got[k]).tobytes() for k in KEYS + ["eta_cell", "norm_cell"] if got[k] is not None)


# ------------------------------------------------------------------ 1. against the reference; 2. the two-level sum
@pytest.mark.parametrize("mesh,perturbed,model", EC.ALL_CASES)
def test_stress_error_against_reference(mesh, perturbed, model):
    c = EC.case(*mesh, perturbed)
    ref = EC.ref(c, model)
    G = _loaded(c)
    assert G.ncells == len(c["mesh"].cells)
    got = G.stress_error(model)
    G.close()
    _check(got, ref)


# ------------------------------------------------------------------ 3. known answers
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[2]])
def test_homogeneous_deformation_on_the_device(mesh):
    c = SC.case(*mesh, True)
    G = _context(c)
    G.set(M.V_U, (c["mesh"].coords @ A0[c["dim"]].T).reshape(-1))
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        r = G.stress_error(model)
        print("model %d: eta %.2e of n = %.4e" % (model, r["error"] / r["norm"], r["norm"]))
        assert r["norm"] > 0 and r["error"] <= TOL * r["norm"]
    G.close()


@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1]])
def test_zero_state_gives_zeros(mesh):
    c = SC.case(*mesh, True)
    G = _context(c)
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        r = G.stress_error(model)
        assert all(r[k] == 0 for k in KEYS), r
        assert np.all(r["eta_cell"] == 0) and np.all(r["norm_cell"] == 0)
    G.close()


@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[1], SC.Q3_MESHES[0], SC.GENERIC_MESHES[0]])
def test_a_state_deformed_in_one_corner_cell_puts_max_cell_there(mesh):
    c = SC.case(*mesh, True)
    m = c["mesh"]
    K = len(m.cells) - 1  # the far corner: faces x+, y+ (, z+), none of them clamped
    count = np.zeros(m.nnodes, int)
    for conn, _, _ in m.cells:
        count[conn] += 1
    own = [a for a in m.cells[K][0] if count[a] == 1]  # the nodes no other cell has
    assert own
    u = np.zeros((m.nnodes, m.dim))
    u[own] = 0.002 * np.random.default_rng(7).standard_normal((len(own), m.dim))
    u = u.reshape(-1)
    assert not np.any(u[m.constrained])
    G = _context(c)
    G.set(M.V_U, u)
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        ref = R.stress_error(m, u, MU, NU, model)
        assert ref["max_cell"] == K
        got = G.stress_error(model)
        assert got["max_cell"] == K
        # cells without a deformed node: sigma_h = 0 exactly on the device, ~1e-16 of the corner's stress in numpy, and the
        # root turns that into n_K ~ 1e-15 n.  So the cells are held to 1e-12 of the TOTAL's scale here; at their own
        # scale they are held by test_stress_error_against_reference
        _check(got, ref, floor=1.0)
    G.close()


# ------------------------------------------------------------------ 4. cross-check with the linear model's energy
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[1], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1]])
def test_norm_is_twice_the_linear_strain_energy(mesh):
    c = SC.case(*mesh, True)
    G = _context(c)
    G.linear_setup(0.5)
    G.set(M.V_U, c["u"])
    n2, want = G.stress_error(M.STRESS_LINEAR)["norm"] ** 2, 2 * G.linear_energy()["strain"]
    G.close()
    print("n^2 %.12e  2 x strain energy %.12e" % (n2, want))
    assert abs(n2 - want) <= TOL * want


# ------------------------------------------------------------------ 5. every mode of a context, the same bytes
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[1], SC.Q2_MESHES[1]])
def test_stress_error_is_mode_independent(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    G = _loaded(c)
    s0 = G.stress_error()
    _check(s0, EC.ref(c, S.NEOHOOKE))
    assert _bits(G.stress_error()) == _bits(s0)
    without = G.stress_error(cells=False)
    assert without["eta_cell"] is None and without["norm_cell"] is None
    assert [without[k] for k in KEYS] == [s0[k] for k in KEYS]
    G.set_tuning("fine_level", 1)
    G.assemble()
    assert _bits(G.stress_error()) == _bits(s0)
    if c["p"] == 3:  # the matrix-free linear set-up releases the tangent array (and clears the state vectors)
        G.set_tuning("linear_operator", 1)
        G.linear_setup(0.5)
        assert G.get_tuning("linear_operator_active") == 1
        G.set(M.V_U, c["u"])
        assert _bits(G.stress_error()) == _bits(s0)
    G.close()


# ------------------------------------------------------------------ 6. purity
def _counters(G):
    return [G.get_tuning(k) for k in COUNTERS]


def _field_bits(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got)


@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[0], SC.Q2_MESHES[0], SC.GENERIC_MESHES[1]])
def test_stress_error_changes_nothing(mesh):
    c = SC.case(*mesh, True)
    G, H = _context(c), _context(c)
    for X in (G, H):
        X.set_profiling(True)
        X.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        X.newmark_step(tol_lin=1e-10)  # from rest under load and body force: a state with every vector in use
    norm0, rhs0 = G.assemble(), G.get(M.V_RHS)
    H.assemble()
    vecs = [G.get(w) for w in range(10)]
    fields = [_field_bits(G.stress_field(model)) for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR)]
    counts = {k: v[1] for k, v in G.timings().items()}
    counters = _counters(G)
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        s0 = G.stress_error(model)
        assert _bits(G.stress_error(model)) == _bits(s0)
    assert counters == _counters(G)
    assert counts == {k: v[1] for k, v in G.timings().items()}
    for w in range(10):
        assert np.array_equal(vecs[w], G.get(w)), w
    assert fields == [_field_bits(G.stress_field(model)) for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR)]
    norm1 = G.assemble()
    assert norm1 == norm0 and np.array_equal(G.get(M.V_RHS), rhs0)
    H.assemble()  # the twin never asked for an indicator
    _, ig = G.newmark_step(tol_lin=1e-10)
    _, ih = H.newmark_step(tol_lin=1e-10)
    assert bytes(ig) == bytes(ih)
    assert np.array_equal(G.get(M.V_U), H.get(M.V_U))
    G.close()
    H.close()


# ------------------------------------------------------------------ 7. errors
@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[0], SC.Q2_MESHES[0], SC.GENERIC_MESHES[1]])
def test_folded_cell_is_reported(mesh):
    c = SC.case(*mesh, True)
    s = 2.0
    with np.errstate(invalid="ignore"):
        while min(pt[4] for pt in S.points(c["mesh"], s * c["u"], MU, NU, S.NEOHOOKE)) > 0:
            s *= 2.0
    G = _loaded(c)
    G.set(M.V_U, s * c["u"])
    with pytest.raises(M.MiError) as err:
        G.stress_error(M.STRESS_NEOHOOKE)
    assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    G.set(M.V_U, c["u"])
    _check(G.stress_error(), EC.ref(c, S.NEOHOOKE))
    assert G.assemble() > 0
    G.close()


def test_teams_are_refused():
    c = SC.case(*SC.TEAM_MESHES[0], True)
    T = _loaded(c, slabs=2, cut_axis=0)
    assert T.comm_info()[0] == 2
    with pytest.raises(M.MiError) as err:
        T.stress_error()
    assert err.value.code == M.MI_EINVAL and "one slab only" in str(err.value)
    T.stress_field()  # (the field itself runs on emulated slabs)
    T.close()


def test_argument_errors():
    c = SC.case(*SC.GENERIC_MESHES[0], False)
    G = _loaded(c)
    for model in (-1, 2):
        with pytest.raises(M.MiError) as err:
            G.stress_error(model)
        assert err.value.code == M.MI_EINVAL
    L = M.lib()
    info = M.StressErrorInfo()
    eta = np.zeros(G.ncells)
    dp = eta.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mi_stress_error(G.h, 0, None, dp, dp) == M.MI_EINVAL
    assert L.mi_stress_error(None, 0, C.byref(info), dp, dp) == M.MI_EINVAL
    assert L.mi_stress_error(G.h, 0, C.byref(info), dp, None) == M.MI_OK  # each array optional on its own
    want = G.stress_error()
    assert np.array_equal(eta, want["eta_cell"]) and info.error == want["error"] and info.reserved == 0
    G.close()
