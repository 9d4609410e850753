"""GPU: the nodal stress recovery (mi_stress_field) against tests/golden/stress_reference.py, the numpy reference anchored by
test_mirror_stress.py.  Cases, material, roles and states: tests/golden/stress_cases.py (those of test_gpu_energy.py).

Tolerances: sigma 1e-12 of max|sigma_ref| per entry, von Mises and weight 1e-12 relative -- test_gpu_energy.py's gate for the same
point stage against the same mirror; test_mirror_stress.py shows the reference's own sums to be good to 1e-13 of max|sigma| on
every case here.  Slabs against the undecomposed context 1e-13 of max|sigma| (another summation order: a slab's colours are
those of its local box), the weights 1e-13 relative -- on the cut planes too, where a ghost-layer cell counted twice or not at
all would show as a factor.  Modes of one context and repeated calls: the same bytes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import stress_cases as SC  # noqa: E402
import stress_reference as S  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

MU, NU, RHO = SC.MU, SC.NU, SC.RHO
BODY = (0.3, -9.81, 1.0)
TOL, TOL_TEAM = 1e-12, 1e-13
COUNTERS = ["count_scalar_allreduce", "count_scalar_allreduce_cg", "count_vector_allreduce", "count_halo_exchange",
            "count_cg_host_sync", "count_cg_iterations", "count_cg_solves", "count_mg_refresh"]
F0 = {2: np.array([[1.08, 0.05], [-0.03, 0.94]]),
      3: np.array([[1.08, 0.05, -0.02], [-0.03, 0.94, 0.04], [0.01, -0.06, 1.03]])}


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


def _check(got, ref, tol=TOL, what=""):
    sigma, vm, W = got
    rs, rv, rw = ref[:3]
    smax = np.abs(rs).max()
    es, ev, ew = np.abs(sigma - rs).max() / smax, np.abs((vm - rv) / rv).max(), np.abs((W - rw) / rw).max()
    print("%s sigma %.2e of max|sigma|, von Mises %.2e, weight %.2e relative (gate %.0e)" % (what, es, ev, ew, tol))
    assert es <= tol
    assert ev <= tol
    assert ew <= tol


def _bits(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got)


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("mesh,perturbed,model", SC.REFERENCE_CASES)
def test_stress_against_reference(mesh, perturbed, model):
    c = SC.case(*mesh, perturbed)
    ref = SC.ref(c, model)
    assert ref[3] >= 0.4 and ref[2].min() > 0
    G = _loaded(c)
    got = G.stress_field(model)
    G.close()
    ncomp = c["dim"] * (c["dim"] + 1) // 2
    assert got[0].shape == (c["mesh"].nnodes, ncomp) and got[1].shape == got[2].shape == (c["mesh"].nnodes,)
    _check(got, ref)


# ------------------------------------------------------------------ 2. homogeneous deformation: the known answer
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[2]])
def test_homogeneous_deformation_on_the_device(mesh):
    c = SC.case(*mesh, True)
    dim = c["dim"]
    H = F0[dim] - np.eye(dim)
    G = _context(c)
    G.set(M.V_U, (c["mesh"].coords @ H.T).reshape(-1))
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        s = S.point_stress(dim, MU, NU, H, model)[0]
        want = np.array([s[d, e] for d, e in S.PAIRS[dim]])
        sigma, vm, _ = G.stress_field(model)
        err = np.abs(sigma - want[None, :]).max() / np.abs(want).max()
        evm = np.abs(vm - S.von_mises(dim, want[None, :])[0]).max() / np.abs(want).max()
        print("model %d: sigma %.2e, von Mises %.2e of max|sigma|" % (model, err, evm))
        assert err <= TOL and evm <= TOL
    G.close()


# ------------------------------------------------------------------ 3. every mode of a context, the same bytes
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[1], SC.Q2_MESHES[1]])
def test_stress_is_mode_independent(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    G = _loaded(c)
    s0 = G.stress_field()
    _check(s0, SC.ref(c, S.NEOHOOKE))
    assert _bits(G.stress_field()) == _bits(s0)
    G.set_tuning("fine_level", 1)
    G.assemble()
    assert _bits(G.stress_field()) == _bits(s0)
    if c["p"] == 3:  # the matrix-free linear set-up releases the tangent array (and clears the state vectors)
        G.set_tuning("linear_operator", 1)
        G.linear_setup(0.5)
        assert G.get_tuning("linear_operator_active") == 1
        G.set(M.V_U, c["u"])
        assert _bits(G.stress_field()) == _bits(s0)
    G.close()


# ------------------------------------------------------------------ 4. purity
def _counters(G):
    return [G.get_tuning(k) for k in COUNTERS]


@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[0], SC.Q2_MESHES[0], SC.GENERIC_MESHES[1]])
def test_stress_changes_nothing(mesh):
    c = SC.case(*mesh, True)
    G, H = _context(c), _context(c)
    for X in (G, H):
        X.set_profiling(True)
        X.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        X.newmark_step(tol_lin=1e-10)  # from rest under load and body force: a state with every vector in use
    norm0, rhs0 = G.assemble(), G.get(M.V_RHS)
    H.assemble()
    vecs = [G.get(w) for w in range(10)]
    counts = {k: v[1] for k, v in G.timings().items()}
    counters = _counters(G)
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        s0 = G.stress_field(model)
        assert _bits(G.stress_field(model)) == _bits(s0)
    assert counters == _counters(G)
    assert counts == {k: v[1] for k, v in G.timings().items()}
    for w in range(10):
        assert np.array_equal(vecs[w], G.get(w)), w
    norm1 = G.assemble()
    assert norm1 == norm0 and np.array_equal(G.get(M.V_RHS), rhs0)
    H.assemble()  # the twin never asked for a stress
    _, ig = G.newmark_step(tol_lin=1e-10)
    _, ih = H.newmark_step(tol_lin=1e-10)
    assert bytes(ig) == bytes(ih)
    assert np.array_equal(G.get(M.V_U), H.get(M.V_U))
    G.close()
    H.close()


# ------------------------------------------------------------------ 5. a folded cell is an error return, not a fault
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
        G.stress_field(M.STRESS_NEOHOOKE)
    assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    lin = G.stress_field(M.STRESS_LINEAR)  # no such case in the linear model: s times the field of u
    _check((lin[0] / s, lin[1] / s, lin[2]), SC.ref(c, S.LINEAR))
    G.set(M.V_U, c["u"])
    _check(G.stress_field(), SC.ref(c, S.NEOHOOKE))
    assert G.assemble() > 0
    G.close()


# ------------------------------------------------------------------ 6. emulated teams: every owned node complete, once
def _cut_plane_nodes(c, slabs, cut):
    """nodes on the planes between the slabs: cut 0 = the direction with most cell layers (ties: the last), else cut - 1"""
    reps, p, dim = c["reps"], c["p"], c["dim"]
    ax = cut - 1
    if cut == 0:
        ax = dim - 1
        for d in range(dim - 2, -1, -1):
            if reps[d] > reps[ax]:
                ax = d
    nn = [p * r + 1 for r in reps]
    idx = (np.arange(c["mesh"].nnodes) // int(np.prod(nn[:ax]))) % nn[ax]
    planes = [p * (reps[ax] * r // slabs) for r in range(1, slabs)]
    return np.nonzero(np.isin(idx, planes))[0]


@pytest.mark.parametrize("mesh,slabs,cut", [(SC.TEAM_MESHES[0], 2, 0), (SC.TEAM_MESHES[0], 4, 0), (SC.TEAM_MESHES[0], 2, 1),
                                            (SC.TEAM_MESHES[1], 2, 0), (SC.TEAM_MESHES[1], 4, 0), (SC.TEAM_MESHES[1], 2, 2),
                                            (SC.TEAM_MESHES[2], 2, 0), (SC.TEAM_MESHES[2], 4, 0), (SC.TEAM_MESHES[2], 2, 2)])
def test_stress_on_emulated_teams(mesh, slabs, cut):
    c = SC.case(*mesh, True)
    if "single" not in c:
        G1 = _loaded(c)
        c["single"] = G1.stress_field()
        G1.close()
        _check(c["single"], SC.ref(c, S.NEOHOOKE), what="single")
    one = c["single"]
    T = _loaded(c, slabs=slabs, cut_axis=cut)
    assert T.comm_info()[0] == slabs
    got = T.stress_field()
    lin = T.stress_field(M.STRESS_LINEAR)
    T.close()
    _check(got, SC.ref(c, S.NEOHOOKE), what="slabs")
    _check(got, one, tol=TOL_TEAM, what="slabs against single")
    _check(lin, SC.ref(c, S.LINEAR), what="slabs, linear")
    on_cut = _cut_plane_nodes(c, slabs, cut)
    assert len(on_cut) > 0
    ew = np.abs(got[2][on_cut] / one[2][on_cut] - 1).max()
    print("weights on the cut planes (%d nodes): %.2e relative" % (len(on_cut), ew))
    assert ew <= TOL_TEAM


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors():
    c = SC.case(*SC.GENERIC_MESHES[0], False)
    G = _loaded(c)
    for model in (-1, 2):
        with pytest.raises(M.MiError) as err:
            G.stress_field(model)
        assert err.value.code == M.MI_EINVAL
    L = M.lib()
    w = np.zeros(G.nnodes)
    dp = w.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mi_stress_field(G.h, 0, None, dp, dp) == M.MI_EINVAL
    assert L.mi_stress_field(None, 0, dp, dp, dp) == M.MI_EINVAL
    sigma = np.zeros((G.nnodes, 3))
    assert L.mi_stress_field(G.h, 0, sigma.ctypes.data_as(C.POINTER(C.c_double)), None, None) == M.MI_OK  # optional outputs
    assert np.array_equal(sigma, G.stress_field()[0])
    G.close()
