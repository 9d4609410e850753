"""GPU: mi_tangent_modes, the lowest eigenpairs of K_T(u) phi = lambda rho M phi on the free dofs at the committed state, against
a dense eigh of the context's own exported tangent (csr() of a "fine_level" 0 context at that state) minus alpha_1 rho times the
dense mass from mass_apply on unit columns (golden/tangent_modes_reference.py; the conditions the bounds rest on are asserted on
the CPU by tests/test_mirror_tangent_modes.py).  Cases and states: golden/tangent_modes_cases.py, default material and time
step (alpha_1 = 1.6e5).  Every case and state with "precond" 0 and 1, the 3D Q2 / Q3 ones also with "fine_level" 1 -- against
the SAME reference, which is the comparison of the two levels.  tol = 1e-8.

All assertions are derived, none measured.  With r_j = K_T x_j - lambda_j rho M x_j on the free dofs, recomputed in numpy:
  1  stopping rule: |r_j|_2 <= (2 tol + floor_j) max_k |lambda_k| |rho M x_j|_2.  The factor 2 is test_gpu_linear_modes.py's; floor_j
     is tangent_modes_reference.floor(), the a priori rounding bound of K_T x formed as A x - alpha_1 rho M x (<= 6.3e-10 on these
     cases, measured 5e-13: the a-priori bound of any summation order lies a factor 1e3 above what the kernels reach and a factor
     30 below 2 tol; the order-of-magnitude figure eps alpha_1 / |lambda| of the header is no bound and is not asserted).  The
     device's own figure residual[j] is <= tol
  2  |X^T rho M X - I|_max <= 1e-10, and the modes are exactly zero on constrained dofs
  3  rho_j = |r_j|_{M^-1} / |x_j|_M < gap_j / 4, gap_j the distance of j's cluster to the nearest reference eigenvalue outside it;
     the nearest reference eigenvalue lies in j's cluster, and |lambda_j - w_j| <= rho_j + E_REF (Krylov-Weinstein)
  4  the sine of the M-angle between x_j and the eigenspace of its cluster is <= (4 rho_j + E_REF) / gap_j (Davis-Kahan)
E_REF = n_free eps (lambda_max + alpha_1): the backward error of the dense reference, whose K_T is itself a difference.

Where the context has a hierarchy the V-cycle run must need fewer iterations than the Jacobi run of the same case.  No absolute
cap on the iteration counts is asserted: none follows from the reference (MAX_IT is a cap, not an expectation).

Further: two calls return the same bits; the six state vectors and the external stress are unchanged bit for bit; with
"precond" 0 the next newmark_step equals an undisturbed twin's bit for bit, with "precond" 1 it converges; max_it = 2 gives
MI_ENOCONV_LIN with its = 2 and finite lambda; the refusals (team, "linear_operator" 1 context, bad arguments, a folded state)
leave the context usable.
"""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import tangent_modes_cases as TC  # noqa: E402
import tangent_modes_reference as TR  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = 1e-8
MAX_IT = 4000  # a cap, not an expectation
RUNS = [(n, s, pre, fl) for n, s in TC.RUNS for fl in ((0, 1) if n in TC.FINE_LEVEL_CASES else (0,)) for pre in (0, 1)]
IDS = ["%s-%s-%s-%s" % (n, s, "multigrid" if p else "jacobi", "matrix_free" if f else "assembled") for n, s, p, f in RUNS]
V_EXT = 6  # MI_V_EXTERNAL_STRESS
_refs, _its = {}, {}


def _context(name, kind=None, precond=0, fine_level=0, **kw):
    c = TC.CASES[name]
    lo, hi, perturb = TC.case_geometry(name)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb, **kw)
    if fine_level:
        G.set_tuning("fine_level", 1)
    G.set_tuning("precond", precond)
    if kind is not None:
        G.set(M.V_U, TC.state(kind, G.coords))
    return G


def _dense_mass(G):
    """rho M [n, n] from the device's own mass on unit columns, six at a time"""
    n = G.n
    Md = np.zeros((n, n))
    for j0 in range(0, n, 6):
        cols = np.arange(j0, min(j0 + 6, n))
        X = np.zeros((len(cols), n))
        X[np.arange(len(cols)), cols] = 1.0
        Md[:, cols] = G.mass_apply(X).T
    return TC.RHO * Md


def _reference(name, kind):
    """dense eigenpairs of the exported (A - alpha_1 rho M)_ff, rho M_ff of an assembled context; computed once, left unchanged"""
    if (name, kind) not in _refs:
        A = _context(name, kind)
        A.assemble()
        Af, Mf, free = TR.free_pencil(A.csr(), _dense_mass(A), A.constrained)
        A.close()
        Kf = Af - TC.ALPHA1 * Mf
        w, V = TR.eigh_free(0.5 * (Kf + Kf.T), Mf)
        _refs[name, kind] = dict(Af=Af, Kf=Kf, Mf=Mf, free=free, w=w, V=V, Mchol=sla.cho_factor(Mf))
    return _refs[name, kind]


def _check(name, out, ref, what, k=None):
    k = TC.CASES[name]["n_modes"] if k is None else k
    Af, Kf, Mf, free, w, V = ref["Af"], ref["Kf"], ref["Mf"], ref["free"], ref["w"], ref["V"]
    lam, modes = out["lam"], out["modes"]
    e_ref = len(free) * EPS * (w[-1] + TC.ALPHA1)
    top = np.abs(w[:k]).max()
    assert np.all(np.isfinite(lam)) and np.all(np.diff(lam) >= 0)
    # 2: constraints exactly, orthonormality
    cons = np.ones(modes.shape[1], dtype=bool)
    cons[free] = False
    assert np.all(modes[:, cons] == 0.0)
    X = modes[:, free].T
    MX, KX = Mf @ X, Kf @ X
    orth = np.abs(X.T @ MX - np.eye(k)).max()
    # 1: the stopping rule
    Rm = KX - MX * lam[None, :]
    ratio = np.linalg.norm(Rm, axis=0) / (np.abs(lam).max() * np.linalg.norm(MX, axis=0))
    floor = TR.floor(Af, Mf, X, np.abs(lam).max())
    # 3: eigenvalues
    xm = np.sqrt(np.einsum("ij,ij->j", X, MX))
    rho = np.sqrt(np.einsum("ij,ij->j", Rm, sla.cho_solve(ref["Mchol"], Rm))) / xm
    gap, of = TR.gaps(w, k)
    nearest = np.array([int(np.argmin(np.abs(w - l))) for l in lam])
    # 4: mode shapes
    sines = np.zeros(k)
    for j in range(k):
        Vc = V[:, of[j][0]:of[j][1]]
        x = X[:, j] / xm[j]
        d = x - Vc @ (Vc.T @ (Mf @ x))
        sines[j] = np.sqrt(d @ (Mf @ d))
    print("%s: its %d, lambda %s, device residual %.2e, recomputed %.2e (floor %.1e), orth %.2e, rho / gap %.2e, |lam - w| / top %.2e, "
          "sine / bound %.2e" % (what, out["its"], lam, out["residual"].max(), ratio.max(), floor.max(), orth, (rho / gap).max(),
                                 np.abs(lam - w[:k]).max() / top, (sines * gap / (4 * rho + e_ref)).max()))
    assert np.all(out["residual"] <= TOL)
    assert np.all(ratio <= 2 * TOL + floor)
    assert orth <= 1e-10
    assert np.all(rho < gap / 4)
    assert all(of[j][0] <= nearest[j] < of[j][1] for j in range(k))
    assert np.all(np.abs(lam - w[:k]) <= rho + e_ref)
    assert np.all(sines <= (4 * rho + e_ref) / gap)


@pytest.mark.parametrize("name,kind,precond,fine_level", RUNS, ids=IDS)
def test_modes_against_dense_reference(name, kind, precond, fine_level):
    ref = _reference(name, kind)
    G = _context(name, kind, precond, fine_level)
    out = G.tangent_modes(TC.CASES[name]["n_modes"], tol=TOL, max_it=MAX_IT)
    _check(name, out, ref, "%s %s precond %d fine_level %d" % (name, kind, precond, fine_level))
    if kind == "compress":
        assert out["lam"][0] < 0  # a buckled state is reported as such
    # the V-cycle is applied and is the tangent's: where a hierarchy exists it needs fewer iterations than the diagonal did on the
    # same case (the Jacobi run of a case comes first; selected alone, the V-cycle run has nothing to compare with)
    _its[name, kind, fine_level, precond] = out["its"]
    if precond == 1 and G.mg_n_levels() > 1 and (name, kind, fine_level, 0) in _its:
        assert out["its"] < _its[name, kind, fine_level, 0]
    G.close()


@pytest.mark.parametrize("precond,fine_level", [(0, 0), (1, 1)])
def test_two_calls_return_the_same_bits(precond, fine_level):
    G = _context("q2_311", "stretch", precond, fine_level)
    a = G.tangent_modes(3, tol=TOL, max_it=MAX_IT)
    b = G.tangent_modes(3, tol=TOL, max_it=MAX_IT)
    for key in ("lam", "modes", "residual"):
        assert np.array_equal(a[key], b[key])
    assert a["its"] == b["its"]
    lam_only = G.tangent_modes(3, tol=TOL, max_it=MAX_IT, want_modes=False)
    assert lam_only["modes"] is None and np.array_equal(lam_only["lam"], a["lam"])
    G.close()


def _step(G):
    rc, info = G.newmark_step(tol_lin=1e-10, check=False)
    return rc, info, [G.get(w) for w in range(6)]


@pytest.mark.parametrize("precond,fine_level", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_state_is_untouched_and_the_next_step_follows(precond, fine_level):
    name = "q2_311"
    G, twin = _context(name, None, precond, fine_level), _context(name, None, precond, fine_level)
    for X in (G, twin):
        X.set_interface_traction((0.0, -40.0, 10.0))
        rc, info, _ = _step(X)
        assert rc == 0 and info.converged == 1
    before = [G.get(w) for w in range(7)]
    assert np.abs(before[0]).max() > 0 and np.abs(before[V_EXT]).max() > 0
    counters = {key: G.get_tuning(key) for key in ("count_cg_iterations", "count_cg_solves")}
    out = G.tangent_modes(3, tol=TOL, max_it=MAX_IT)
    assert np.all(out["residual"] <= TOL)
    for w, v in enumerate(before):
        assert np.array_equal(G.get(w), v), w
    assert {key: G.get_tuning(key) for key in counters} == counters
    rc, info, state = _step(G)
    assert rc == 0 and info.converged == 1
    if precond == 0:
        rc_t, info_t, state_t = _step(twin)
        assert rc_t == 0 and info.newton_iterations == info_t.newton_iterations and info.lin_its_total == info_t.lin_its_total
        for a, b in zip(state, state_t):
            assert np.array_equal(a, b)
    G.close()
    twin.close()


def test_not_converged_returns_the_best_pairs():
    G = _context("q1_422", "stretch")
    with pytest.raises(M.MiError) as e:
        G.tangent_modes(3, tol=TOL, max_it=2)
    assert e.value.code == M.MI_ENOCONV_LIN
    part = e.value.partial
    assert part["its"] == 2 and np.all(np.isfinite(part["lam"])) and np.all(np.isfinite(part["residual"]))
    assert np.all(part["residual"][-1:] > TOL) and np.all(np.isfinite(part["modes"]))
    _check("q1_422", G.tangent_modes(3, tol=TOL, max_it=MAX_IT), _reference("q1_422", "stretch"), "q1_422 after max_it 2")
    G.close()


def test_refusals_leave_the_context_usable():
    name, kind = "q3_211", "bend"
    G = _context(name, kind)
    for kw in (dict(n_modes=0), dict(n_modes=17), dict(n_modes=1, tol=0.0), dict(n_modes=1, max_it=0)):
        with pytest.raises(M.MiError) as e:
            G.tangent_modes(**kw)
        assert e.value.code == M.MI_EINVAL, kw
    good = TC.state(kind, G.coords)
    folded = good.copy()
    folded[0::3] = -1.5 * G.coords[:, 0]  # det F < 0 everywhere
    G.set(M.V_U, folded)
    with pytest.raises(M.MiError) as e:
        G.tangent_modes(1)
    assert e.value.code == M.MI_EINVAL and "inverted element" in str(e.value)
    assert np.array_equal(G.get(M.V_U), folded)
    for w in range(1, 7):  # the other five state vectors and the external stress: untouched (here: still zero)
        assert not G.get(w).any(), w
    G.set(M.V_U, good)
    # a "linear_operator" 1 set-up releases the tangent array: refused until an assembled set-up brings it back
    G.set_tuning("linear_operator", 1)
    G.linear_setup(0.5)
    G.set(M.V_U, good)  # (a linear set-up starts from rest)
    with pytest.raises(M.MiError) as e:
        G.tangent_modes(1)
    assert e.value.code == M.MI_EINVAL and "linear_operator" in str(e.value)
    assert np.array_equal(G.get(M.V_U), good)
    G.set_tuning("linear_operator", 0)
    G.linear_setup(0.5)
    G.set(M.V_U, good)
    _check(name, G.tangent_modes(3, tol=TOL, max_it=MAX_IT), _reference(name, kind), "q3_211 after refusals")
    G.close()
    S = _context("q1_422", "stretch", slabs=2)
    with pytest.raises(M.MiError) as e:
        S.tangent_modes(1)
    assert e.value.code == M.MI_EINVAL and "one slab only" in str(e.value)
    S.set(M.V_U, np.zeros(S.n))
    rc, info = S.newmark_step(check=False)  # the team still steps
    assert rc == 0
    S.close()
