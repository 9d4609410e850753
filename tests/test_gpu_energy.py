"""GPU: the energy diagnostics (mi_energy, mi_linear_energy) against tests/golden/energy_reference.py, the numpy reference
anchored by test_mirror_energy.py, and against the library's own residual, products and matrices.

Meshes: the smallest at which each kernel form can go wrong, box and vertex-perturbed (0.1 h) each -- energy_q3 on 2 x 2 x 2 and
3 x 2 x 3, energy_q2 on 2 x 2 x 2 and 3 x 2 x 2, energy_cells on 2D p = 1..4 (3 x 2), 3D p = 1 (2 x 2 x 2) and 3D p = 4 (1 x 1 x 2).
State: u = amp randn on the free dofs, v = randn, body force (0.3, -9.81, 1.0); amp is halved from 0.02 until the REFERENCE's
smallest det F is >= 0.4, which is asserted before the device is asked.

Tolerances: strain and kinetic 1e-12 relative (fp64 sums of a few thousand positive terms); the body potential 1e-12 of
rho |b| max|u| volume (a signed sum); slabs against the undecomposed context 1e-13 (another summation order); modes of one
context: the same bits (the kernels read u, v, the mesh tables and cell boxes with the same values in every mode); the
derivative identity 1e-6 at eps = 1e-5 as the CPU anchor (truncation ~eps^2); the linear model 1e-12; the theta = 1/2 balance
1e-6 as test_gpu_properties.py.
"""
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import energy_reference as E  # noqa: E402
import mirror as Mi  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

MU, NU, RHO = 0.7e6, 0.3, 870.0
BODY = (0.3, -9.81, 1.0)
ROLES = [1, 7, 0, 7, 8, 0]  # x- clamped, x+ / y+ interface, z- clamped in z (3D)
TOL, TOL_TEAM = 1e-12, 1e-13
COUNTERS = ["count_scalar_allreduce", "count_scalar_allreduce_cg", "count_vector_allreduce", "count_halo_exchange",
            "count_cg_host_sync", "count_cg_iterations", "count_cg_solves", "count_mg_refresh"]

# (dim, degree, reps): by kernel form
Q3_MESHES = [(3, 3, (2, 2, 2)), (3, 3, (3, 2, 3))]
Q2_MESHES = [(3, 2, (2, 2, 2)), (3, 2, (3, 2, 2))]
GENERIC_MESHES = [(2, 1, (3, 2)), (2, 2, (3, 2)), (2, 3, (3, 2)), (2, 4, (3, 2)), (3, 1, (2, 2, 2)), (3, 4, (1, 1, 2))]
TEAM_MESHES = [(3, 2, (2, 2, 4)), (3, 3, (2, 2, 4)), (2, 2, (6, 2))]

_cases = {}


def _case(dim, p, reps, perturbed):
    """mesh, admissible state and reference energies of a case, built once and left unchanged"""
    key = (dim, p, tuple(reps), perturbed)
    if key in _cases:
        return _cases[key]
    reps = tuple(reps)
    h = 0.1
    hi = tuple(h * r for r in reps)
    rng = np.random.default_rng(100 * dim + 10 * p + sum(reps) + int(perturbed))
    nv = int(np.prod([r + 1 for r in reps]))
    perturb = 0.1 * h * rng.uniform(-1, 1, (nv, dim)) if perturbed else None
    roles = ROLES[:2 * dim]
    m = Mi.Mesh(dim, p, reps, (0.0,) * dim, hi, roles, perturb=perturb)
    u0 = rng.standard_normal(m.n) * ~m.constrained
    v = rng.standard_normal(m.n)
    amp = 0.02 * h / 0.1
    while True:
        ref = E.energies(m, amp * u0, v, MU, NU, RHO, BODY[:dim])
        if ref[3] >= 0.4:
            break
        amp *= 0.5
    c = dict(dim=dim, p=p, reps=reps, hi=hi, perturb=perturb, roles=roles, mesh=m, u=amp * u0, v=v, ref=ref, vol=E.volume(m))
    _cases[key] = c
    return c


def _context(c, body=BODY, **kw):
    fr = list(c["roles"]) + [0] * (6 - len(c["roles"]))
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=(0.0,) * c["dim"], hi=c["hi"], face_role=fr, mu=MU, nu=NU,
                  rho=RHO, body_force=tuple(body), perturb=c["perturb"], **kw)
    assert G.n == c["mesh"].n and np.array_equal(G.constrained, c["mesh"].constrained)
    return G


def _loaded(c, **kw):
    G = _context(c, **kw)
    G.set(M.V_U, c["u"])
    G.set(M.V_V, c["v"])
    return G


def _check(c, e, ref=None, tol=TOL):
    strain, kinetic, body, det = c["ref"] if ref is None else ref
    assert det >= 0.4
    bscale = RHO * np.linalg.norm(BODY[:c["dim"]]) * np.abs(c["u"]).max() * c["vol"]
    print("strain %.17g ref %.17g rel %.2e | kinetic rel %.2e | body err/scale %.2e" % (
        e["strain"], strain, abs(e["strain"] - strain) / strain, abs(e["kinetic"] - kinetic) / kinetic,
        abs(e["body"] - body) / bscale))
    assert abs(e["strain"] - strain) <= tol * strain
    assert abs(e["kinetic"] - kinetic) <= tol * kinetic
    assert abs(e["body"] - body) <= tol * bscale


def _bits(e):
    return np.array([e["strain"], e["kinetic"], e["body"]]).tobytes()


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", Q3_MESHES + Q2_MESHES + GENERIC_MESHES)
def test_energy_against_reference(mesh, perturbed):
    c = _case(*mesh, perturbed)
    G = _loaded(c)
    _check(c, G.energy())
    G.close()


# ------------------------------------------------------------------ 2. every mode of a context, the same bits
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [Q3_MESHES[1], Q2_MESHES[1]])
def test_energy_is_mode_independent(mesh, perturbed):
    c = _case(*mesh, perturbed)
    G = _loaded(c)
    e0 = G.energy()
    _check(c, e0)
    G.set_tuning("fine_level", 1)
    G.assemble()
    e1 = G.energy()
    assert _bits(e1) == _bits(e0)
    if c["p"] == 3:  # the matrix-free linear set-up releases the tangent array (and clears the state vectors)
        G.set_tuning("linear_operator", 1)
        G.linear_setup(0.5)
        assert G.get_tuning("linear_operator_active") == 1
        G.set(M.V_U, c["u"])
        G.set(M.V_V, c["v"])
        assert _bits(G.energy()) == _bits(e0)
    G.close()


# ------------------------------------------------------------------ 3. purity and repeatability
def _counters(G):
    return [G.get_tuning(k) for k in COUNTERS]


@pytest.mark.parametrize("mesh", [Q3_MESHES[0], Q2_MESHES[0], GENERIC_MESHES[1]])
def test_energy_changes_nothing(mesh):
    c = _case(*mesh, True)
    G, H = _context(c), _context(c)
    for X in (G, H):
        X.set_profiling(True)
        X.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        X.newmark_step(tol_lin=1e-10)  # from rest under load and body force: a state with every vector in use
    vecs = [G.get(w) for w in range(10)]
    counts = {k: v[1] for k, v in G.timings().items()}
    counters = _counters(G)
    e0 = G.energy()
    assert _bits(G.energy()) == _bits(e0)
    assert counters == _counters(G)
    assert counts == {k: v[1] for k, v in G.timings().items()}
    for w in range(10):
        assert np.array_equal(vecs[w], G.get(w)), w
    _, ig = G.newmark_step(tol_lin=1e-10)
    _, ih = H.newmark_step(tol_lin=1e-10)  # the twin never asked
    assert bytes(ig) == bytes(ih)
    assert np.array_equal(G.get(M.V_U), H.get(M.V_U))
    G.close()
    H.close()


# ------------------------------------------------------------------ 4. the strain energy is the potential of the device's residual
@pytest.mark.parametrize("mesh", [Q3_MESHES[1], Q2_MESHES[1]])
def test_energy_derivative_is_the_residual(mesh):
    c = _case(*mesh, True)
    G = _loaded(c, body=(0.0, 0.0, 0.0))
    G.assemble()  # zero acceleration, body force and traction
    rhs = G.get(M.V_RHS)
    free = ~c["mesh"].constrained
    d = np.random.default_rng(5).standard_normal(G.n) * free
    d *= np.abs(c["u"]).max() / np.abs(d).max()
    eps = 1e-5
    G.set(M.V_U, c["u"] + eps * d)
    Wp = G.energy()["strain"]
    G.set(M.V_U, c["u"] - eps * d)
    Wm = G.energy()["strain"]
    dW = (Wp - Wm) / (2 * eps)
    print("dW %.12e  -rhs.d %.12e  rel %.2e" % (dW, -(rhs @ d), abs(dW + rhs @ d) / abs(rhs @ d)))
    assert abs(dW + rhs @ d) <= 1e-6 * abs(rhs @ d)
    G.close()


# ------------------------------------------------------------------ 5. rigid translation, zero state
@pytest.mark.parametrize("mesh", [Q3_MESHES[0], Q2_MESHES[0], GENERIC_MESHES[2], GENERIC_MESHES[5]])
def test_rigid_translation_and_zero_state(mesh):
    c = _case(*mesh, True)
    G = _context(c)
    e = G.energy()
    assert e["strain"] == 0.0 and e["kinetic"] == 0.0 and e["body"] == 0.0
    G.set(M.V_U, np.tile(np.array([0.013, -0.021, 0.008])[:c["dim"]], G.nnodes))
    e = G.energy()
    print("rigid translation: strain %.3e (bound %.3e)" % (e["strain"], 1e-12 * MU * c["vol"]))
    assert abs(e["strain"]) <= 1e-12 * MU * c["vol"]
    G.close()


# ------------------------------------------------------------------ 6. a folded cell is an error return, not a fault
@pytest.mark.parametrize("mesh", [Q3_MESHES[0], Q2_MESHES[0], GENERIC_MESHES[1]])
def test_folded_cell_is_reported(mesh):
    c = _case(*mesh, True)
    s = 2.0
    while E.energies(c["mesh"], s * c["u"], c["v"], MU, NU, RHO, BODY[:c["dim"]])[3] >= 0:
        s *= 2.0
    G = _loaded(c)
    G.set(M.V_U, s * c["u"])
    with pytest.raises(M.MiError) as err:
        G.energy()
    assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    G.set(M.V_U, c["u"])
    _check(c, G.energy())
    assert G.assemble() > 0
    G.set(M.V_U, 0 * c["u"])
    G.set(M.V_V, 0 * c["v"])
    rc, info = G.newmark_step(tol_lin=1e-10)
    assert rc == 0 and info.converged == 1
    G.close()


# ------------------------------------------------------------------ 7. emulated teams: every cell counted once
@pytest.mark.parametrize("mesh,slabs,cut", [(TEAM_MESHES[0], 2, 0), (TEAM_MESHES[0], 4, 0), (TEAM_MESHES[1], 2, 0),
                                            (TEAM_MESHES[2], 3, 1)])
def test_energy_on_emulated_teams(mesh, slabs, cut):
    c = _case(*mesh, True)
    G1 = _loaded(c)
    e1 = G1.energy()
    G1.close()
    _check(c, e1)
    T = _loaded(c, slabs=slabs, cut_axis=cut)
    assert T.comm_info()[0] == slabs
    et = T.energy()
    T.close()
    _check(c, et)
    _check(c, et, ref=(e1["strain"], e1["kinetic"], e1["body"], c["ref"][3]), tol=TOL_TEAM)


# ------------------------------------------------------------------ 8. the linear model
L_D, L_V, L_F_OLD = 0, 2, 4


def _linear_reference(G, c, d, v):
    """1/2 d^T K d, 1/2 v^T M v, -d . f from the exported matrices and the body-force vector (F_1 of a step without load)"""
    K, Mm = G.linear_csr(0), G.linear_csr(1)
    G.linear_step(1, 1e-10)
    f = G.get(L_F_OLD)
    return 0.5 * d @ (K @ d), 0.5 * v @ (Mm @ v), -(d @ f), f


def _check_linear(c, e, ref, tol=TOL):
    bscale = RHO * np.linalg.norm(BODY[:c["dim"]]) * np.abs(c["u"]).max() * c["vol"]
    print("linear: strain rel %.2e kinetic rel %.2e body err/scale %.2e" % (
        abs(e["strain"] - ref[0]) / ref[0], abs(e["kinetic"] - ref[1]) / ref[1], abs(e["body"] - ref[2]) / bscale))
    assert abs(e["strain"] - ref[0]) <= tol * ref[0]
    assert abs(e["kinetic"] - ref[1]) <= tol * ref[1]
    assert abs(e["body"] - ref[2]) <= tol * bscale


@pytest.mark.parametrize("mesh", [Q3_MESHES[1], Q2_MESHES[0], GENERIC_MESHES[2]])
def test_linear_energy_assembled(mesh):
    c = _case(*mesh, True)
    G = _context(c)
    with pytest.raises(M.MiError) as err:
        G.linear_energy()
    assert err.value.code == M.MI_EINVAL
    G.linear_setup(0.5)
    ref = _linear_reference(G, c, c["u"], c["v"])
    G.set(L_D, c["u"])
    G.set(L_V, c["v"])
    e = G.linear_energy()
    _check_linear(c, e, ref)
    # ... and the independent reference: mirror.Linear's matrices and body vector
    Lm = Mi.Linear(c["mesh"], MU, NU, RHO, BODY[:c["dim"]])
    _check_linear(c, e, E.linear_energies(Lm, c["u"], c["v"]))
    if c["dim"] == 3:  # two emulated slabs, against the undecomposed context
        T = _context(c, slabs=2)
        T.linear_setup(0.5)
        T.set(L_D, c["u"])
        T.set(L_V, c["v"])
        _check_linear(c, T.linear_energy(), (e["strain"], e["kinetic"], e["body"]))
        T.close()
    G.close()


@pytest.mark.parametrize("perturbed", [False, True])
def test_linear_energy_matrix_free(perturbed):
    c = _case(*Q3_MESHES[1], perturbed)
    out = []
    for op in (0, 1):
        G = _context(c)
        G.set_tuning("linear_operator", op)
        G.linear_setup(0.5)
        assert G.get_tuning("linear_operator_active") == op
        G.set(L_D, c["u"])
        G.set(L_V, c["v"])
        out.append(G.linear_energy())
        G.close()
    _check_linear(c, out[1], (out[0]["strain"], out[0]["kinetic"], out[0]["body"]))


def test_linear_energy_balance_of_the_midpoint_scheme():
    """three steps at theta = 1/2 under a constant load: E_n+1 - E_n = work of the mean load along the displacement increment
    (the balance test_gpu_properties.py checks from exported matrices), with E from mi_linear_energy"""
    c = _case(*Q2_MESHES[1], False)
    G = _context(c, body=(0.0, 0.0, 0.0))
    G.linear_setup(0.5)
    G.set_interface_traction((0.0, -200.0, 0.0))
    d_old, f_prev, energy = np.zeros(G.n), np.zeros(G.n), [0.0]
    for step in range(3):
        G.linear_step(1, 1e-10)
        d, f = G.get(L_D), G.get(L_F_OLD)
        e = G.linear_energy()
        assert e["body"] == 0.0
        Etot = e["strain"] + e["kinetic"]
        work = 0.5 * (f + f_prev) @ (d - d_old)
        print("step %d: dE %.12e work %.12e" % (step, Etot - energy[-1], work))
        assert abs((Etot - energy[-1]) - work) <= 1e-6 * max(abs(work), 1e-30)
        energy.append(Etot)
        d_old, f_prev = d, f
    assert energy[-1] > 0
    G.close()
