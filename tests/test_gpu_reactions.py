"""GPU: nodal forces, support reactions and load resultants (mi_reactions) against tests/golden/reactions_reference.py, the numpy
reference anchored by test_mirror_reactions.py.  Cases: tests/golden/reactions_cases.py (the meshes, roles and displacement
states of stress_cases.py with an acceleration, a body force and a traction).

Tolerances.  Against the reference 1e-12: each term of that term's max, forces of the largest term's max, resultants and moments
of the sums of the absolute values of their addends -- the gate test_gpu_stress_field.py and test_gpu_energy.py apply to the same
point stage against the same mirror; test_mirror_reactions.py shows the reference's own sums to cancel to 1e-14 of those scales.
Equilibrium: a max is bounded by the 2-norm, a sum of n numbers by sqrt(n) times their 2-norm, so the unbalanced force is held
to the residual norm the solver itself reports plus the 1e-12 round-off term; nothing is fitted to what the device returns.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import reactions_cases as RC  # noqa: E402
import reactions_reference as R  # noqa: E402
import stress_cases as SC  # noqa: E402
import stress_reference as S  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

MU, NU, RHO, BODY, DT = RC.MU, RC.NU, RC.RHO, RC.BODY, RC.DT
TOL = 1e-12
COUNTERS = ["count_scalar_allreduce", "count_scalar_allreduce_cg", "count_vector_allreduce", "count_halo_exchange",
            "count_cg_host_sync", "count_cg_iterations", "count_cg_solves", "count_mg_refresh"]  # test_gpu_stress_field.py's
F0 = {2: np.array([[1.08, 0.05], [-0.03, 0.94]]),
      3: np.array([[1.08, 0.05, -0.02], [-0.03, 0.94, 0.04], [0.01, -0.06, 1.03]])}  # test_gpu_stress_field.py's
VECTORS = ("reaction", "unbalanced", "inertia", "body", "load")
STEP_MESHES = [(2, 2, (6, 2)), (3, 2, (3, 2, 2)), (3, 3, (2, 2, 2))]
TRACTION = (0.0, -50.0, 0.0)
LINEAR_TRACTION = (0.0, -1e3, 0.0)


def _context(c, **kw):
    fr = list(c["roles"]) + [0] * (6 - len(c["roles"]))
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=(0.0,) * c["dim"], hi=c["hi"], face_role=fr, mu=MU, nu=NU,
                  rho=RHO, body_force=BODY, perturb=c["perturb"], delta_t=DT, **kw)
    assert G.n == c["mesh"].n and np.array_equal(G.constrained, c["mesh"].constrained)
    return G


def _load(G, c, model):
    if model == R.NEOHOOKE:
        G.set(M.V_U, c["u"])
        G.set(M.V_A, c["acc"])
        G.set(M.V_STRESS, c["traction"])
    else:
        G.set(RC.L_DISPLACEMENT, c["u"])
        G.set(RC.L_VELOCITY, c["v"])
        G.set(RC.L_OLD_VELOCITY, c["v_old"])
        G.set(RC.L_OLD_STRESS, c["f_old"])


def _device(c, model, about=None):
    """mi_reactions of the case on a fresh context, computed once and left unchanged"""
    key = ("device", model, about)
    if key not in c:
        G = _context(c)
        _load(G, c, model)
        c[key] = G.reactions(model, about=about, forces=True, terms=True)
        G.close()
    return c[key]


def _bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in sorted(r) if r[k] is not None)


def _within(got, want, scale, what):
    """|got - want| <= TOL scale, entry by entry (scale 0: equal)"""
    got, want, scale = np.asarray(got, float), np.asarray(want, float), np.asarray(scale, float)
    err = np.abs(got - want)
    rel = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%-20s %.2e (gate %.0e)" % (what, rel.max(), TOL))
    assert rel.max() <= TOL, what


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("mesh,perturbed,model", SC.REFERENCE_CASES)
def test_reactions_against_reference(mesh, perturbed, model):
    c = RC.case(*mesh, perturbed)
    T, ref, det = RC.ref(c, model)
    assert det >= 0.4
    got = _device(c, model)
    assert got["terms"].shape == (4, c["mesh"].n) and got["forces"].shape == (c["mesh"].n,)
    for k, name in enumerate(("internal", "inertia", "body", "load")):
        _within(got["terms"][k], T[k], np.abs(T[k]).max(), name)
    _within(got["forces"], ref["forces"], np.abs(T).max(), "forces")
    for name in VECTORS:
        _within(got[name], ref[name], ref[name + "_scale"], name)
        _within(got[name + "_moment"], ref[name + "_moment"], ref[name + "_moment_scale"], name + " moment")
    for name in ("internal_abs", "max_unbalanced", "max_reaction"):
        _within(got[name], ref[name], abs(ref[name]), name)
    assert got["max_reaction_node"] == ref["max_reaction_node"]
    assert np.array_equal(got["about"], np.zeros(3))
    assert np.abs(ref["reaction"]).max() > 0 and np.abs(T[3][c["mesh"].constrained]).max() > 0


# ------------------------------------------------------------------ 2. the identities, on the device's own numbers
@pytest.mark.parametrize("mesh,perturbed,model", SC.REFERENCE_CASES)
def test_identities_on_the_device(mesh, perturbed, model):
    c = RC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    for about in (None, RC.ABOUT[:dim]):
        ref = RC.ref(c, model, about)[1]
        got = _device(c, model, about)
        x0 = np.zeros(dim) if about is None else np.asarray(about)
        assert np.array_equal(got["about"][:dim], x0)
        x = m.coords + (c["u"].reshape(-1, dim) if model == R.NEOHOOKE else 0.0) - x0
        f, mom, _, _ = R.sum_and_moment(m, x, got["terms"][0])
        ef, em = np.abs(f).max() / got["internal_abs"], np.abs(mom).max() / ref["internal_moment_scale"].max()
        print("about %s: sum internal %.2e of internal_abs, moment %.2e of its absolute sum" % (about, ef, em))
        assert ef <= TOL and em <= TOL
        # reaction + unbalanced = inertia - body - load, force and moment (the scale: the absolute sums of everything added)
        for suffix in ("", "_moment"):
            lhs = got["reaction" + suffix] + got["unbalanced" + suffix]
            rhs = got["inertia" + suffix] - got["body" + suffix] - got["load" + suffix]
            scale = sum(ref[name + suffix + "_scale"] for name in VECTORS) + ref["internal" + suffix + "_scale"]
            _within(lhs - rhs, np.zeros(3), scale, "balance" + suffix)
    if model == R.NEOHOOKE and perturbed:  # the identity is about the CURRENT positions: about X_i it fails by orders of magnitude
        _, mom, _, _ = R.sum_and_moment(m, m.coords, _device(c, model)["terms"][0])
        assert np.abs(mom).max() / RC.ref(c, model)[1]["internal_moment_scale"].max() >= 1e-5


# ------------------------------------------------------------------ 3. homogeneous deformation: the known answer
@pytest.mark.parametrize("dim,p,reps", [(3, 2, (2, 2, 2)), (3, 3, (2, 2, 2)), (2, 3, (3, 2))])
def test_clamp_force_of_a_homogeneous_deformation(dim, p, reps):
    hi = tuple(0.1 * r for r in reps)
    G = M.Context(dim=dim, degree=p, reps=reps, lo=(0.0,) * dim, hi=hi, face_role=[1, 0, 0, 0, 0, 0], mu=MU, nu=NU, rho=RHO,
                  delta_t=DT)
    X = G.coords
    H = F0[dim] - np.eye(dim)
    G.set(M.V_U, (X @ H.T).reshape(-1))
    r = G.reactions(terms=True)
    G.close()
    tau = Mi.material(dim, MU, NU, F0[dim])[0]
    Pk = tau @ np.linalg.inv(F0[dim]).T
    want = np.zeros(3)
    want[:dim] = -Pk[:, 0] * np.prod(hi[1:])
    scale = np.abs(Pk).max() * np.prod(hi[1:])
    print("reaction", r["reaction"], "expected", want)
    assert np.abs(r["reaction"] - want).max() <= TOL * scale
    interior = np.all((X > 1e-9) & (X < np.array(hi) - 1e-9), axis=1)
    assert interior.any()
    internal = r["terms"][0].reshape(-1, dim)
    ei = np.abs(internal[interior]).max() / np.abs(internal).max()
    print("internal force at %d interior nodes: %.2e of max|internal|" % (interior.sum(), ei))
    assert ei <= TOL
    assert not r["terms"][1].any() and not r["terms"][2].any() and not r["terms"][3].any()


# ------------------------------------------------------------------ 4. / 5. after two Newmark steps: the library's own residual, equilibrium
_stepped_cache = {}


def _stepped(mesh, fine_level, point_pass):
    """two mi_newmark_steps under a constant traction and the body force, then what the tests below compare (computed once)"""
    key = (mesh, fine_level, point_pass)
    if key not in _stepped_cache:
        c = RC.case(*mesh, True)
        G = _context(c)
        if fine_level:
            G.set_tuning("fine_level", 1)
        if point_pass:
            G.set_tuning("point_pass_q3", 1)
        G.set_interface_traction(TRACTION[:c["dim"]])
        for _ in range(2):
            _, info = G.newmark_step(tol_lin=1e-10)
            assert info.converged == 1
        r = G.reactions(terms=True)
        G.newton_begin_step()
        G.assemble_residual()
        _stepped_cache[key] = dict(r=r, rhs=G.get(M.V_RHS), res_abs=info.res_abs, free=~c["mesh"].constrained)
        G.close()
    return _stepped_cache[key]


STEP_MODES = ([(STEP_MESHES[0], 0, 0)] + [(STEP_MESHES[1], fl, 0) for fl in (0, 1)] +
              [(STEP_MESHES[2], 0, 0), (STEP_MESHES[2], 1, 0), (STEP_MESHES[2], 1, 1)])


@pytest.mark.parametrize("mesh,fine_level,point_pass", STEP_MODES)
def test_forces_are_the_librarys_own_residual(mesh, fine_level, point_pass):
    s = _stepped(mesh, fine_level, point_pass)
    scale = np.abs(s["r"]["terms"]).max()
    err = np.abs(s["rhs"] + s["r"]["forces"])[s["free"]].max() / scale
    print("system_rhs + forces on the free dofs: %.2e of the largest term (gate %.0e)" % (err, TOL))
    assert err <= TOL


@pytest.mark.parametrize("mesh,fine_level,point_pass", STEP_MODES)
def test_newmark_state_is_in_equilibrium(mesh, fine_level, point_pass):
    s = _stepped(mesh, fine_level, point_pass)
    r, n_free = s["r"], int(s["free"].sum())
    roundoff = TOL * np.abs(r["terms"][0]).max()
    print("max_unbalanced %.3e, |unbalanced| %.3e, res_abs %.3e, round-off term %.3e, |reaction| %.3e" %
          (r["max_unbalanced"], np.linalg.norm(r["unbalanced"]), s["res_abs"], roundoff, np.linalg.norm(r["reaction"])))
    assert r["max_unbalanced"] <= s["res_abs"] + roundoff
    assert np.linalg.norm(r["unbalanced"]) <= np.sqrt(n_free) * s["res_abs"] + roundoff
    assert np.linalg.norm(r["reaction"]) > 0


# ------------------------------------------------------------------ 6. the linear model: the theta scheme's identity
LINEAR_MODES = [(STEP_MESHES[0], 0), (STEP_MESHES[1], 0), (STEP_MESHES[2], 0), (STEP_MESHES[2], 1)]
ABS_TOL = 1e-11


def _linear_context(mesh, operator, theta):
    c = RC.case(*mesh, True)
    G = _context(c)
    if operator:
        G.set_tuning("linear_operator", 1)
    G.linear_setup(theta)
    assert G.get_tuning("linear_operator_active") == operator
    G.set_interface_traction(LINEAR_TRACTION[:c["dim"]])
    return c, G


@pytest.mark.parametrize("mesh,operator", LINEAR_MODES)
def test_linear_model_balances_at_theta_one(mesh, operator):
    """res of mi_linear_step is the 2-norm of the CG's residual of A v = rhs when it stopped (cg_run: sqrt(r.r) of the recurrence,
    <= abs_tol; rows of constrained dofs carry rhs = 0 and v = 0), so ||(A v - rhs)_free||_2 / dt <= res / dt."""
    c, G = _linear_context(mesh, operator, 1.0)
    for _ in range(2):
        _, res = G.linear_step(True, ABS_TOL)
    r = G.reactions(M.STRESS_LINEAR, terms=True)
    G.close()
    T, free = r["terms"], ~c["mesh"].constrained
    out = np.linalg.norm((T[0] + T[1] - T[3])[free])
    bound = res / DT + TOL * np.sqrt(free.sum()) * np.abs(T).max()
    print("||internal + inertia - load|| on free dofs %.3e, bound %.3e, max|internal| %.3e" % (out, bound, np.abs(T[0]).max()))
    assert bound <= 1e-6 * np.abs(T[0]).max()
    assert out <= bound
    assert not T[2].any() and np.abs(r["reaction"]).max() > 0


@pytest.mark.parametrize("mesh,operator", LINEAR_MODES)
def test_linear_model_theta_identity_over_two_calls(mesh, operator):
    """inertia_{n+1} + theta (internal - load)_{n+1} + (1 - theta) (internal - load)_n = (A v - rhs) / dt on the free dofs"""
    theta = 0.5
    c, G = _linear_context(mesh, operator, theta)
    G.linear_step(True, ABS_TOL)
    G.linear_step(True, ABS_TOL)
    Tn = G.reactions(M.STRESS_LINEAR, forces=False, terms=True)["terms"]
    _, res = G.linear_step(True, ABS_TOL)
    T1 = G.reactions(M.STRESS_LINEAR, forces=False, terms=True)["terms"]
    G.close()
    free = ~c["mesh"].constrained
    out = np.linalg.norm((T1[1] + theta * (T1[0] - T1[3]) + (1 - theta) * (Tn[0] - Tn[3]))[free])
    single = np.linalg.norm((T1[0] + T1[1] - T1[3])[free])
    bound = res / DT + TOL * np.sqrt(free.sum()) * max(np.abs(T1).max(), np.abs(Tn).max())
    print("two-call identity %.3e, bound %.3e, max|internal| %.3e; one call alone %.3e" % (out, bound, np.abs(T1[0]).max(), single))
    assert bound <= 1e-6 * np.abs(T1[0]).max()
    assert out <= bound


# ------------------------------------------------------------------ 7. purity and modes
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[1], SC.Q2_MESHES[1]])
def test_reactions_are_mode_independent(mesh, perturbed):
    c = RC.case(*mesh, perturbed)
    G = _context(c)
    _load(G, c, R.NEOHOOKE)
    r0 = G.reactions(terms=True)
    assert _bits(r0) == _bits(_device(c, R.NEOHOOKE))
    assert _bits(G.reactions(terms=True)) == _bits(r0)
    G.set_tuning("fine_level", 1)
    G.assemble()
    assert _bits(G.reactions(terms=True)) == _bits(r0)
    if c["p"] == 3:  # the matrix-free linear set-up releases the tangent array (and clears the state vectors)
        G.set_tuning("linear_operator", 1)
        G.linear_setup(0.5)
        assert G.get_tuning("linear_operator_active") == 1
        _load(G, c, R.NEOHOOKE)
        assert _bits(G.reactions(terms=True)) == _bits(r0)
    G.close()


def _counters(G):
    return [G.get_tuning(k) for k in COUNTERS]


@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[0], SC.Q2_MESHES[0], SC.GENERIC_MESHES[1]])
def test_reactions_change_nothing(mesh):
    c = RC.case(*mesh, True)
    G, H = _context(c), _context(c)
    for X in (G, H):
        X.set_profiling(True)
        X.set_interface_traction(TRACTION[:c["dim"]])
        X.newmark_step(tol_lin=1e-10)  # from rest under load and body force: a state with every vector in use
    norm0, rhs0 = G.assemble(), G.get(M.V_RHS)
    H.assemble()
    vecs = [G.get(w) for w in range(10)]
    counts = {k: v[1] for k, v in G.timings().items()}
    counters = _counters(G)
    for model in (M.STRESS_NEOHOOKE, M.STRESS_LINEAR):
        r0 = G.reactions(model, about=RC.ABOUT[:c["dim"]], terms=True)
        assert _bits(G.reactions(model, about=RC.ABOUT[:c["dim"]], terms=True)) == _bits(r0)
    assert counters == _counters(G)
    assert counts == {k: v[1] for k, v in G.timings().items()}
    for w in range(10):
        assert np.array_equal(vecs[w], G.get(w)), w
    norm1 = G.assemble()
    assert norm1 == norm0 and np.array_equal(G.get(M.V_RHS), rhs0)
    H.assemble()  # the twin never asked for a reaction
    _, ig = G.newmark_step(tol_lin=1e-10)
    _, ih = H.newmark_step(tol_lin=1e-10)
    assert bytes(ig) == bytes(ih)
    assert np.array_equal(G.get(M.V_U), H.get(M.V_U))
    G.close()
    H.close()


@pytest.mark.parametrize("mesh,operator", [(STEP_MESHES[0], 0), (STEP_MESHES[2], 1)])
def test_reactions_leave_the_linear_step_alone(mesh, operator):
    runs = []
    for ask in (True, False):
        c, G = _linear_context(mesh, operator, 0.5)
        G.linear_step(True, ABS_TOL)
        if ask:
            G.reactions(M.STRESS_LINEAR, terms=True)
        out = G.linear_step(True, ABS_TOL)
        runs.append((out, [G.get(w) for w in range(10)]))
        G.close()
    assert runs[0][0] == runs[1][0]
    for w in range(10):
        assert np.array_equal(runs[0][1][w], runs[1][1][w]), w


@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[0], SC.Q2_MESHES[0], SC.GENERIC_MESHES[1]])
def test_folded_cell_is_reported(mesh):
    c = RC.case(*mesh, True)
    s = 2.0
    with np.errstate(invalid="ignore"):
        while min(pt[4] for pt in S.points(c["mesh"], s * c["u"], MU, NU, S.NEOHOOKE)) > 0:
            s *= 2.0
    G = _context(c)
    _load(G, c, R.NEOHOOKE)
    G.set(M.V_U, s * c["u"])
    with pytest.raises(M.MiError) as err:
        G.reactions()
    assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    G.set(M.V_U, c["u"])
    assert _bits(G.reactions(terms=True)) == _bits(_device(c, R.NEOHOOKE))
    assert G.assemble() > 0
    G.close()


def test_emulated_slabs_are_refused():
    c = RC.case(*SC.TEAM_MESHES[0], True)
    T = _context(c, slabs=2)
    assert T.comm_info()[0] == 2
    with pytest.raises(M.MiError) as err:
        T.reactions()
    assert err.value.code == M.MI_EINVAL and "one slab only" in str(err.value)
    T.close()


def test_argument_errors():
    c = RC.case(*SC.GENERIC_MESHES[0], False)
    G = _context(c)
    _load(G, c, R.NEOHOOKE)
    for model in (-1, 2):
        with pytest.raises(M.MiError) as err:
            G.reactions(model)
        assert err.value.code == M.MI_EINVAL
    L = M.lib()
    info = M.ReactionInfo()
    assert L.mi_reactions(G.h, 0, None, None, None, None) == M.MI_EINVAL
    assert L.mi_reactions(None, 0, None, C.byref(info), None, None) == M.MI_EINVAL
    assert L.mi_reactions(G.h, 0, None, C.byref(info), None, None) == M.MI_OK  # every array optional
    assert np.array_equal(np.array(info.reaction), _device(c, R.NEOHOOKE)["reaction"])
    G.close()
