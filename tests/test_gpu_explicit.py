"""GPU: the explicit time integrator (mi_explicit_setup, mi_explicit_run, mi_explicit_get_mass, mi_explicit_stable_dt) against the
numpy reference tests/golden/explicit_reference.py, which tests/test_mirror_explicit.py anchors on the CPU.

Cases: explicit_reference.CASES -- 3D Q1-Q4 and 2D Q1-Q4 meshes of cell edge 0.1, each with a clamped face, an interface face with
a non-uniform traction and a body force; |u| about 3e-3, |v| up to 8.  The 3D Q2 and Q3 cases also run with "fine_level" 1, Q3
also with "point_pass_q3" 1: the force pass is whichever pass the keys select.

  1  explicit_mass() to 1e-13 and the acceleration after the set-up to 1e-12 of the reference's
  2  ten steps at dt = 1/2 dt_crit(reference): u, v, a after steps 1, 2, 5, 10 to 1e-12 of each field's maximum, the project's
     tolerance for mirror comparisons (the CPU test measures rounding perturbations of the force to stay below 1e-13)
  3  explicit_run(10) equals ten explicit_run(1) bit for bit; two runs from the same state give the same bytes; steps_done, dt,
     inverted_step as documented; kinetic_lumped = 1/2 sum m v^2 of the returned v within gamma_n = n eps / (1 - n eps)
  4  one step composed from the public pieces -- set(ACC, 0), set(DELTA, du), assemble_residual, get(RHS) and the host formulas --
     to 1e-14 relative (FMA contraction forbids bit equality); and on every context whose force pass is one of the two
     one-launch point passes, the run with the force-only instances ("explicit_force_only" 1, the default) equals (==) the run
     through the zero vector (key 0): a0 of the set-up, the six vectors and the right-hand side after 1 and after 5 more steps
  5  a velocity field that folds a cell at step k of the reference: MI_EINVAL naming step k, steps_done = k - 1, the six vectors
     those of a separate explicit_run(k - 1) bit for bit; a run from a good state afterwards succeeds.  (det F <= 0 is the flag
     every assembly test exercises; nothing faults)
  6  the Ritz value of explicit_stable_dt against dense eigh of the context's own exported matrices (csr() minus alpha_1 rho times
     mass_apply of unit columns, with explicit_mass()): 0.9 lambda_max <= theta <= lambda_max (1 + 1e-12); two calls give the same
     bits; 200 steps at 0.8 dt_crit keep strain + kinetic_lumped + body within a factor of 2 of its start (no traction in that
     run: with one the sum is no invariant)
  7  a context that ran set-up and steps and was set back with mi_vec_set, and a fresh one given the same vectors, return the same
     bits from newmark_step ("precond" 0, "cg_warm_start" 0); state_save / state_restore around a run restores the six vectors
  8  the refusals, each with nothing changed
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import explicit_reference as ER  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ALPHA1 = 1.0 / (0.25 * 0.005**2)
RUNS = []
for _n in ER.CASES:
    RUNS.append((_n, 0, 0))
    if _n in ER.FINE_LEVEL:
        RUNS.append((_n, 1, 0))
    if _n in ER.POINT_PASS_Q3:
        RUNS.append((_n, 1, 1))
IDS = ["%s-%s%s" % (n, "matrix_free" if f else "assembled", "-point_pass" if p else "") for n, f, p in RUNS]
_traj = {}


def _context(name, fine_level=0, point_pass=0, state=True, traction=True, **kw):
    c = ER.CASES[name]
    lo, hi, perturb = ER.geometry(name)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=ER.roles(name), perturb=perturb,
                  mu=ER.MU, nu=ER.NU, rho=ER.RHO, body_force=ER.BODY, **kw)
    if fine_level:
        G.set_tuning("fine_level", 1)
    if point_pass:
        G.set_tuning("point_pass_q3", 1)
        assert G.get_tuning("point_pass_q3_active") == 1
    R = ER.reference(name)
    if traction:
        ids, _ = G.interface()
        assert np.array_equal(ids, R.mesh.interface_nodes)
        G.set_interface_traction(ER.traction(R.mesh.coords[ids]))
    if state:
        u, v = ER.initial_state(R.mesh.coords)
        G.set(M.V_U, u)
        G.set(M.V_V, v)
    return G


def _trajectory(name):
    """the reference's states after steps 1 .. 10 at 1/2 dt_crit; computed once, left unchanged"""
    if name not in _traj:
        R = ER.reference(name)
        u, v, a = R.initial()
        _traj[name] = (a, R.run(u, v, a, ER.dt_half_crit(name), ER.STEPS))
    return _traj[name]


def _six(G):
    return [G.get(w) for w in range(6)]


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name,fine_level,point_pass", RUNS, ids=IDS)
def test_masses_initial_acceleration_and_steps(name, fine_level, point_pass):
    R = ER.reference(name)
    a0, traj = _trajectory(name)
    G = _context(name, fine_level, point_pass)
    dt = ER.dt_half_crit(name)
    G.explicit_setup(dt)
    e_m = _rel(G.explicit_mass(), R.mass)
    e_a = _rel(G.get(M.V_A), a0)
    print("%s: mass %.1e, a0 %.1e" % (name, e_m, e_a))
    assert e_m <= 1e-13 and e_a <= 1e-12
    assert np.array_equal(G.get(M.V_A), G.get(M.V_A_OLD)) and not G.get(M.V_DELTA).any()
    done = 0
    for at in ER.CHECK_AT:
        out = G.explicit_run(at - done)
        assert out["rc"] == 0 and out["steps_done"] == at - done and out["inverted_step"] == -1
        done = at
        errs = [_rel(G.get(w), ref) for w, ref in zip((M.V_U, M.V_V, M.V_A), traj[at - 1])]
        print("%s: step %d  u %.1e v %.1e a %.1e" % (name, at, *errs))
        assert max(errs) <= 1e-12, (at, errs)
    G.close()


@pytest.mark.parametrize("name,fine_level,point_pass", [("q2_311p", 0, 0), ("q2_222", 1, 0), ("q3_211", 1, 1), ("q1_222", 0, 0),
                                                        ("2d_q3_21", 0, 0)])
def test_chaining_and_repeatability(name, fine_level, point_pass):
    R = ER.reference(name)
    G = _context(name, fine_level, point_pass)
    dt = ER.dt_half_crit(name)
    G.explicit_setup(dt)
    G.state_save()
    out = G.explicit_run(10)
    assert (out["rc"], out["steps_done"], out["inverted_step"], out["dt"]) == (0, 10, -1, dt)
    A = _six(G)
    for w in (0, 2, 4):  # the *_OLD vectors equal the new ones, the delta is zero, the right-hand side holds the last force
        assert np.array_equal(A[w], A[w + 1])
    assert not G.get(M.V_DELTA).any()
    assert _rel(np.where(G.constrained, 0.0, 1.0 / G.explicit_mass()) * G.get(M.V_RHS), A[4]) <= 4 * EPS
    mv2 = R.mass * A[2] * A[2]
    n = mv2.size + 2
    assert abs(out["kinetic_lumped"] - 0.5 * mv2.sum()) <= n * EPS / (1 - n * EPS) * 0.5 * np.abs(mv2).sum()
    G.state_restore()
    for _ in range(10):
        one = G.explicit_run(1)
        assert one["steps_done"] == 1
    for a, b in zip(A, _six(G)):
        assert np.array_equal(a, b)
    assert one["kinetic_lumped"] == out["kinetic_lumped"]
    G.state_restore()
    again = G.explicit_run(10)
    for a, b in zip(A, _six(G)):
        assert a.tobytes() == b.tobytes()
    assert again == out
    zero = G.explicit_run(0)  # a no-op that fills info
    assert (zero["steps_done"], zero["inverted_step"], zero["kinetic_lumped"]) == (0, -1, out["kinetic_lumped"])
    for a, b in zip(A, _six(G)):
        assert np.array_equal(a, b)
    G.close()


@pytest.mark.parametrize("name,fine_level,point_pass", RUNS, ids=IDS)
def test_one_step_from_the_public_pieces(name, fine_level, point_pass):
    G, H = _context(name, fine_level, point_pass), _context(name, fine_level, point_pass)
    dt = ER.dt_half_crit(name)
    for X in (G, H):
        X.explicit_setup(dt)
    u, v, a = H.get(M.V_U), H.get(M.V_V), H.get(M.V_A)
    assert np.array_equal(a, G.get(M.V_A))
    du = dt * v + 0.5 * dt * dt * a
    H.set(M.V_A, np.zeros(H.n))
    H.set(M.V_DELTA, du)
    H.assemble_residual()
    F = H.get(M.V_RHS)
    minv = np.where(H.constrained, 0.0, 1.0 / H.explicit_mass())
    an = minv * F
    want = (u + du, v + 0.5 * dt * (a + an), an)
    G.explicit_run(1)
    errs = [_rel(G.get(w), ref) for w, ref in zip((M.V_U, M.V_V, M.V_A), want)]
    print("%s: composed step  u %.1e v %.1e a %.1e" % (name, *errs))
    assert max(errs) <= 1e-14
    G.close()
    H.close()


FORCE_ONLY_RUNS = [(n, f, p) for n, f, p in RUNS if f == 1 and (ER.CASES[n]["p"] == 2 or p == 1)]  # the one-launch point passes


@pytest.mark.parametrize("name,fine_level,point_pass", FORCE_ONLY_RUNS, ids=[IDS[RUNS.index(r)] for r in FORCE_ONLY_RUNS])
def test_force_only_instances_equal_the_zero_vector_form(name, fine_level, point_pass):
    G, Z = _context(name, fine_level, point_pass), _context(name, fine_level, point_pass)
    assert G.get_tuning("explicit_force_only") == 1  # the default
    Z.set_tuning("explicit_force_only", 0)
    assert Z.get_tuning("explicit_force_only") == 0
    dt = ER.dt_half_crit(name)
    for X in (G, Z):
        X.explicit_setup(dt)
    assert np.abs(G.get(M.V_A)).max() > 0
    for n in (0, 1, 5):
        if n:
            a, b = G.explicit_run(n), Z.explicit_run(n)
            assert a == b
        for w in list(range(6)) + [M.V_RHS, M.V_DELTA]:
            assert np.all(G.get(w) == Z.get(w)), (n, w)
    G.close()
    Z.close()


@pytest.mark.parametrize("name,fine_level", [("q2_311p", 0), ("q2_311p", 1), ("q3_211", 1), ("2d_q2_61", 0)])
def test_fold_is_decided_on_the_device(name, fine_level):
    R = ER.reference(name)
    dt = ER.dt_half_crit(name)
    u0, v0 = ER.initial_state(R.mesh.coords)
    vf = ER.fold_velocity(R.mesh.coords, dt)
    k, before, at = R.fold_step(u0, vf, R.minv * R.force(u0), dt, 12)
    assert k >= 3
    G, T = _context(name, fine_level), _context(name, fine_level)
    for X in (G, T):
        X.set(M.V_V, vf)
        X.explicit_setup(dt)
    with pytest.raises(M.MiError) as e:
        G.explicit_run(k + 3)
    part = e.value.partial
    print("%s: reference folds at step %d (det F %.3f -> %.3f); device: %s" % (name, k, before, at, e.value))
    assert e.value.code == M.MI_EINVAL and "inverted element" in str(e.value) and ("at explicit step %d " % k) in str(e.value)
    assert part["steps_done"] == k - 1 and part["inverted_step"] == k
    good = T.explicit_run(k - 1)
    assert good["rc"] == 0 and good["kinetic_lumped"] == part["kinetic_lumped"]
    for a, b in zip(_six(G), _six(T)):
        assert np.array_equal(a, b)
    assert not G.get(M.V_DELTA).any()
    # a good state afterwards: the context steps again
    G.set(M.V_U, u0)
    G.set(M.V_V, v0)
    G.explicit_setup(dt)
    assert G.explicit_run(3)["steps_done"] == 3
    G.close()
    T.close()


def _dense_mass(G):
    n = G.n
    Md = np.zeros((n, n))
    for j0 in range(0, n, 6):
        cols = np.arange(j0, min(j0 + 6, n))
        X = np.zeros((len(cols), n))
        X[np.arange(len(cols)), cols] = 1.0
        Md[:, cols] = G.mass_apply(X).T
    return Md


@pytest.mark.parametrize("name,fine_level", [("q2_311p", 0), ("q2_311p", 1), ("q3_211", 1), ("q1_222", 0), ("2d_q3_21", 0)])
def test_stability_estimate(name, fine_level):
    A = _context(name)  # the exported matrices come from an assembled context at the same state
    A.assemble()
    free = np.nonzero(~A.constrained)[0]
    K = (A.csr().toarray() - ALPHA1 * ER.RHO * _dense_mass(A))[np.ix_(free, free)]
    lam = ER.lambda_max_dense(0.5 * (K + K.T), A.explicit_mass()[free])
    A.close()
    G = _context(name, fine_level)
    before = _six(G) + [G.get(M.V_STRESS)]
    theta, dt_crit = G.explicit_stable_dt(40)
    theta2, dt2 = G.explicit_stable_dt()
    print("%s fine_level %d: theta / lambda_max = %.13f, dt_crit %.4e" % (name, fine_level, theta / lam, dt_crit))
    assert 0.9 * lam <= theta <= lam * (1 + 1e-12)
    assert (theta, dt_crit) == (theta2, dt2) and dt_crit == 2.0 / np.sqrt(theta)
    for a, b in zip(before, _six(G) + [G.get(M.V_STRESS)]):
        assert np.array_equal(a, b)
    G.close()


@pytest.mark.parametrize("name,fine_level", [("q2_311p", 1), ("2d_q2_61", 0)])
def test_energy_stays_bounded_at_the_safety_factor(name, fine_level):
    R = ER.reference(name)
    G = _context(name, fine_level, traction=False)
    G.set(M.V_V, 0.1 * ER.initial_state(R.mesh.coords)[1])
    _, dt_crit = G.explicit_stable_dt()
    G.explicit_setup(0.8 * dt_crit)

    def total(kin):
        e = G.energy()
        return e["strain"] + kin + e["body"]
    e0 = total(G.explicit_run(0)["kinetic_lumped"])
    e1 = total(G.explicit_run(200)["kinetic_lumped"])
    print("%s: energy %.6g -> %.6g after 200 steps of %.3e" % (name, e0, e1, 0.8 * dt_crit))
    assert e0 > 0 and 0.5 * e0 <= e1 <= 2.0 * e0
    G.close()


@pytest.mark.parametrize("name,fine_level", [("q2_311p", 0), ("q2_311p", 1), ("2d_q2_61", 0)])
def test_purity(name, fine_level):
    G, F = _context(name, fine_level), _context(name, fine_level)
    for X in (G, F):
        X.set_tuning("precond", 0)
        X.set_tuning("cg_warm_start", 0)
    start = _six(G)
    counters = {key: G.get_tuning(key) for key in ("count_cg_iterations", "count_cg_solves")}
    G.explicit_setup(ER.dt_half_crit(name))
    G.state_save()
    saved = _six(G)
    G.explicit_run(5)
    assert {key: G.get_tuning(key) for key in counters} == counters
    assert not np.array_equal(G.get(M.V_U), saved[0])
    G.state_restore()
    for a, b in zip(saved, _six(G)):
        assert np.array_equal(a, b)
    for w, v in enumerate(start):
        G.set(w, v)
    out = []
    for X in (G, F):
        rc, info = X.newmark_step(tol_lin=1e-10, check=False)
        assert rc == 0 and info.converged == 1
        out.append((info.newton_iterations, info.lin_its_total, _six(X)))
    assert out[0][:2] == out[1][:2]
    for a, b in zip(out[0][2], out[1][2]):
        assert np.array_equal(a, b)
    G.close()
    F.close()


def test_refusals_change_nothing():
    name = "q2_311p"
    G = _context(name)
    L, h = M.lib(), G.h
    before = _six(G) + [G.get(w) for w in (M.V_STRESS, M.V_DELTA, M.V_RHS)]

    def unchanged():
        return all(np.array_equal(a, b) for a, b in zip(before, _six(G) + [G.get(w) for w in (M.V_STRESS, M.V_DELTA, M.V_RHS)]))

    def refused(call, text=None):
        with pytest.raises(M.MiError) as e:
            call()
        assert e.value.code == M.MI_EINVAL and (text is None or text in str(e.value)), str(e.value)
        assert unchanged()
    refused(lambda: G.explicit_run(1), "mi_explicit_setup has not been called")
    refused(lambda: G.explicit_setup(0.0))
    refused(lambda: G.explicit_setup(-1e-4))
    refused(lambda: G.explicit_setup(float("nan")))
    refused(lambda: G.explicit_run(1), "mi_explicit_setup has not been called")  # a refused set-up is none
    refused(lambda: G.explicit_stable_dt(0))
    info = M.ExplicitInfo()
    lam = C.c_double(0)
    assert L.mi_explicit_run(h, 1, None) == M.MI_EINVAL and unchanged()
    assert L.mi_explicit_get_mass(h, None) == M.MI_EINVAL and unchanged()
    assert L.mi_explicit_stable_dt(h, 40, None, C.byref(lam)) == M.MI_EINVAL and unchanged()
    assert L.mi_explicit_stable_dt(h, 40, C.byref(lam), None) == M.MI_EINVAL and unchanged()
    for f, args in (("mi_explicit_setup", (1e-4, 1)), ("mi_explicit_run", (1, C.byref(info))), ("mi_explicit_get_mass", (None,)),
                    ("mi_explicit_stable_dt", (40, C.byref(lam), C.byref(lam)))):
        assert getattr(L, f)(None, *args) == M.MI_EINVAL
    G.explicit_setup(ER.dt_half_crit(name), init_acceleration=False)  # keeps the state as it is
    assert unchanged()
    refused(lambda: G.explicit_run(-1))
    assert G.explicit_run(2)["steps_done"] == 2
    G.close()
    S = _context("q1_222", state=False, traction=False, slabs=2)
    for call in (lambda: S.explicit_setup(1e-4), lambda: S.explicit_run(1), S.explicit_mass, S.explicit_stable_dt):
        with pytest.raises(M.MiError) as e:
            call()
        assert e.value.code == M.MI_EINVAL and "one slab only" in str(e.value)
    rc, _ = S.newmark_step(check=False)  # the team still steps
    assert rc == 0
    S.close()
