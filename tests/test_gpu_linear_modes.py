"""GPU: mi_linear_modes, the lowest eigenpairs of K phi = lambda M phi on the free dofs, against a dense eigh of the assembled
context's own exported K and M (golden/modes_reference.py; the conditions the bounds below rest on are asserted on the CPU by
tests/test_mirror_modes.py).  Contexts: dt = 0.02, theta = 0.5; every case with "linear_precond" 0 and 1, q3_212d also with
"linear_operator" 1 (its reference: a second, assembled context); tol = 1e-8, max_it = 1000 (a cap, not an expectation).

All assertions are derived, none measured.  With r_j = K x_j - lambda_j M x_j on the free dofs, recomputed in numpy:
  1  stopping rule: |r_j|_2 <= 2 tol max_k |lambda_k| |M x_j|_2.  The factor 2 covers the rounding of the two evaluations of the
     residual (<= 1e-10 relative under eps lambda_max / lambda_n <= 1e-10) and, for the matrix-free form, the 1e-12 by which its
     products differ from the assembled matrices'; the device's own figure residual[j] is <= tol
  2  |X^T M X - I|_max <= 1e-10, and the modes are exactly zero on constrained dofs
  3  rho_j = |r_j|_{M^-1} / |x_j|_M (dense solve) is < gap_j / 4, gap_j the distance of the j-th reference eigenvalue to the
     nearest outside its cluster.  Some reference eigenvalue lies within rho_j of lambda_j (Krylov-Weinstein), so the nearest one
     is the j-th: asserted, with |lambda_j - w_j| <= rho_j + E_REF.  No mode is missed or doubled.  The rigid cluster is matched
     as a cluster: the number of |lambda_j| <= 2 tol lambda_n equals its size
  4  the sine of the M-angle between x_j and the reference eigenvector (for the rigid cluster: its eigenspace) is
     <= (4 rho_j + E_REF) / gap_j (Davis-Kahan with the gap reduced by rho_j < gap_j / 4)
E_REF = n_free eps lambda_max: the backward error of the dense reference itself.

Further: two calls return the same bits; the call changes no state vector and no "count_cg_*" counter, and three linear steps
after it equal those of a twin context bit for bit; a context with dt = 0.005 returns the same eigenvalues within (3); max_it = 2
gives MI_ENOCONV_LIN with its = 2 and finite lambda; the refusals leave the context usable.

Iterations the device needed at tol 1e-8 (MI355X; Jacobi diagonal / multigrid V-cycle):
  q3_212d 159 / 23 (matrix-free: 159 / 23)   q2_432g 187 / 26   q1_543d 78 / 11   q4_211 577 / 31   2d_q2_93 148 / 18
  2d_q3_free 159 / 17   q2_free3d 169 / 23   2d_q2_93 at dt = 0.005 with the V-cycle: 25
Measured there as well: recomputed stopping ratio = the device's to three digits (4.4e-9 .. 9.6e-9), |X^T M X - I| <= 2.2e-15,
rho / gap <= 1.8e-6, |lambda - w| <= 4.4e-13 lambda_n, sine <= 7.4e-3 of its bound.
"""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import modes_reference as MR  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = 1e-8
RUNS = [(name, pre, 0) for name in MR.CASES for pre in (0, 1)] + [("q3_212d", 0, 1), ("q3_212d", 1, 1)]
IDS = ["%s-%s-%s" % (n, "multigrid" if p else "jacobi", "matrix_free" if o else "assembled") for n, p, o in RUNS]
COUNTERS = ["count_cg_iterations", "count_cg_solves"]
_refs = {}


def _context(name, precond=0, operator=0, dt=MR.DT, setup=True, **kw):
    c = MR.CASES[name]
    lo, hi, perturb = MR.case_geometry(name)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb, delta_t=dt,
                  **kw)
    G.set_tuning("linear_operator", operator)
    G.set_tuning("linear_precond", precond)
    if setup:
        G.linear_setup(MR.THETA)
        assert G.get_tuning("linear_operator_active") == operator and G.get_tuning("linear_precond_active") == precond
    return G


def _reference(name, G=None):
    """dense eigenpairs of the exported K_ff, M_ff of an assembled context of the case; computed once, left unchanged"""
    if name not in _refs:
        own = G is None or G.get_tuning("linear_operator_active") != 0
        A = _context(name) if own else G
        Kf, Mf, free = MR.free_pencil(A.linear_csr(0), A.linear_csr(1), A.constrained)
        if own:
            A.close()
        w, V = MR.eigh_free(Kf, Mf)
        _refs[name] = dict(Kf=Kf, Mf=Mf, free=free, w=w, V=V, Mchol=sla.cho_factor(Mf), n_rigid=MR.rigid_count(name))
    return _refs[name]


def _check(name, out, ref, what):
    c = MR.CASES[name]
    k, nr = c["n_modes"], ref["n_rigid"]
    Kf, Mf, free, w, V = ref["Kf"], ref["Mf"], ref["free"], ref["w"], ref["V"]
    lam, modes = out["lam"], out["modes"]
    e_ref = len(free) * EPS * w[-1]
    top = w[k - 1]
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
    # 3: eigenvalues
    xm = np.sqrt(np.einsum("ij,ij->j", X, MX))
    rho = np.sqrt(np.einsum("ij,ij->j", Rm, sla.cho_solve(ref["Mchol"], Rm))) / xm
    gap = MR.gaps(w, k, nr)
    nearest = np.array([int(np.argmin(np.abs(w - l))) for l in lam])
    # 4: mode shapes
    sines = np.zeros(k)
    for j in range(k):
        Vc = V[:, :nr] if j < nr else V[:, j:j + 1]
        x = X[:, j] / xm[j]
        d = x - Vc @ (Vc.T @ (Mf @ x))
        sines[j] = np.sqrt(d @ (Mf @ d))
    print("%s: its %d, device residual %.2e, recomputed %.2e, orth %.2e, rho / gap %.2e, |lam - w| / lam_n %.2e, "
          "sine / bound %.2e" % (what, out["its"], out["residual"].max(), ratio.max(), orth, (rho / gap).max(),
                                 np.abs(lam - w[:k]).max() / top, (sines * gap / (4 * rho + e_ref)).max()))
    assert np.all(out["residual"] <= TOL)
    assert np.all(ratio <= 2 * TOL)
    assert orth <= 1e-10
    assert np.all(rho < gap / 4)
    assert int(np.sum(np.abs(lam) <= 2 * TOL * top)) == nr
    assert np.array_equal(nearest[nr:], np.arange(nr, k))
    assert np.all(nearest[:nr] < nr)
    assert np.all(np.abs(lam - w[:k]) <= rho + e_ref)
    assert np.all(sines <= (4 * rho + e_ref) / gap)


@pytest.mark.parametrize("name,precond,operator", RUNS, ids=IDS)
def test_modes_against_dense_reference(name, precond, operator):
    G = _context(name, precond, operator)
    ref = _reference(name, G)
    out = G.linear_modes(MR.CASES[name]["n_modes"], tol=TOL, max_it=1000)
    _check(name, out, ref, "%s precond %d operator %d" % (name, precond, operator))
    G.close()


@pytest.mark.parametrize("precond,operator", [(0, 0), (1, 1)])
def test_two_calls_return_the_same_bits(precond, operator):
    G = _context("q3_212d", precond, operator)
    a = G.linear_modes(6, tol=TOL)
    b = G.linear_modes(6, tol=TOL)
    for key in ("lam", "modes", "residual"):
        assert np.array_equal(a[key], b[key])
    assert a["its"] == b["its"]
    lam_only = G.linear_modes(6, tol=TOL, want_modes=False)
    assert lam_only["modes"] is None and np.array_equal(lam_only["lam"], a["lam"])
    G.close()


def _three_steps(G, seed=3):
    rng = np.random.default_rng(seed)
    k = len(G.interface()[0])
    out = []
    for step in range(3):
        G.set_interface_traction(1e3 * rng.standard_normal((k, G.dim)))
        its, res = G.linear_step(step != 1, 1e-9)
        out += [np.array([its, res]), G.get(M.V_U), G.get(M.V_V)]
    return out


@pytest.mark.parametrize("precond,operator", [(0, 0), (1, 0), (1, 1)])
def test_call_is_pure(precond, operator):
    G, twin = _context("q3_212d", precond, operator), _context("q3_212d", precond, operator)
    rng = np.random.default_rng(11)
    state = [rng.standard_normal(G.n) * ~G.constrained for _ in range(10)]
    for X in (G, twin):
        for which, v in enumerate(state):
            X.set(which, v)
    before = {key: G.get_tuning(key) for key in COUNTERS}
    G.linear_modes(6, tol=TOL)
    for which, v in enumerate(state):
        assert np.array_equal(G.get(which), v), which
    assert {key: G.get_tuning(key) for key in COUNTERS} == before
    assert G.get_tuning("linear_operator_active") == operator and G.get_tuning("linear_precond_active") == precond
    for a, b in zip(_three_steps(G), _three_steps(twin)):
        assert np.array_equal(a, b)
    G.close()
    twin.close()


def test_result_does_not_depend_on_the_time_step():
    name = "2d_q2_93"
    G = _context(name, 1, dt=0.005)
    ref = _reference(name)
    out = G.linear_modes(MR.CASES[name]["n_modes"], tol=TOL, max_it=1000)
    _check(name, out, ref, "%s dt 0.005" % name)
    G.close()


def test_not_converged_returns_the_best_pairs():
    G = _context("q2_432g")
    with pytest.raises(M.MiError) as e:
        G.linear_modes(14, tol=TOL, max_it=2)
    assert e.value.code == M.MI_ENOCONV_LIN
    part = e.value.partial
    assert part["its"] == 2 and np.all(np.isfinite(part["lam"])) and np.all(np.isfinite(part["residual"]))
    assert np.all(part["residual"][-1:] > TOL) and np.all(np.isfinite(part["modes"]))
    assert G.linear_modes(1, tol=1e-6)["lam"][0] > 0  # the context stays usable
    G.close()


def test_refusals_leave_the_context_usable():
    G = _context("q1_543d", setup=False)
    with pytest.raises(M.MiError) as e:  # no set-up
        G.linear_modes(1)
    assert e.value.code == M.MI_EINVAL
    G.linear_setup(MR.THETA)
    for kw in (dict(n_modes=0), dict(n_modes=17), dict(n_modes=1, tol=0.0), dict(n_modes=1, max_it=0)):
        with pytest.raises(M.MiError) as e:
            G.linear_modes(**kw)
        assert e.value.code == M.MI_EINVAL, kw
    ref = _reference("q1_543d", G)
    _check("q1_543d", G.linear_modes(1, tol=TOL), ref, "q1_543d after refusals")
    its, res = G.linear_step(True, 1e-9)
    assert its > 0 or res <= 1e-9
    G.close()
    S = _context("q1_543d", slabs=2)
    with pytest.raises(M.MiError) as e:
        S.linear_modes(1)
    assert e.value.code == M.MI_EINVAL and "one slab only" in str(e.value)
    its, res = S.linear_step(True, 1e-9)  # the team still steps
    assert np.isfinite(res)
    S.close()
