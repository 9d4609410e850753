"""GPU: mi_evaluate_stress (Context.evaluate_stress: the kernel family stress_at_points and sym_eig_batch) and
mi_principal_stress against tests/golden/stress_points_reference.py, the numpy reference anchored by
test_mirror_stress_points.py, and against known answers.

Meshes, material and states: tests/golden/stress_cases.py -- Q3_MESHES, Q2_MESHES and GENERIC_MESHES, box and perturbed: 2D and 3D,
degrees 1 to 4, all 16 instances of stress_at_points.  Points: point_eval_cases.interior_pairs / boundary_pairs (every face, edge
and corner of every cell), the context's own nodes, points outside and NaN.

Tolerances.  sigma and von Mises 1e-12 of max|sigma| against the closed form and the reference: the tolerance of the stress and
point tests (worst observed gradient error there 5.6e-14).  Principal stresses, measured against the tensor alone (no
gap-dependent comparison of eigenvectors): |sigma v_k - lambda_k v_k|_2 <= c eps |sigma|_F and |sum lambda - tr sigma| likewise,
c = 8 x 1.65 = 13.2; |V V^T - I| <= 8 x 6.0 = 48 eps.  1.65 and 6.0 are the worst figures of the numpy mirror of the device's
statements on the same tensors (test_mirror_stress_points.py: residual 1.61, trace 1.64, orthonormality 6.00 in 3D); the 8
covers fused multiply-adds and the different rounding of the sweeps on the device (measured there: 2.29, 2.54 and 6.00).  The
states of stress_cases.py are admissible at quadrature points; where one folds a cell at a boundary point (det F = -0.11 at one
corner of the perturbed 2 x 2 x 2 Q3 case) the raw neo-Hookean stress is asked to be the error, not compared.  Every comparison
prints its worst figure.
"""
import ctypes as C
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
TOL = 1e-12
C_RES, C_ORTH = 8 * SP.MIRROR_EIG_RES, 8 * SP.MIRROR_EIG_ORTH
MESHES = SC.Q3_MESHES + SC.Q2_MESHES + SC.GENERIC_MESHES
MODELS = (M.STRESS_NEOHOOKE, M.STRESS_LINEAR)
KINDS = (M.STRESS_AT_RAW, M.STRESS_AT_RECOVERED)


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


def _pairs(m, n, seed):
    """n interior pairs and the pairs on every face, edge and corner of every cell"""
    ic, ixi = PC.interior_pairs(m, n, np.random.default_rng(seed))
    bc, bxi = PC.boundary_pairs(m)
    return np.concatenate([ic, bc]), np.concatenate([ixi, bxi])


def _unfolded_pairs(c, n, seed):
    """_pairs without those at which the case's random state folds a containing cell (see _unfolded)"""
    cells, xi = _pairs(c["mesh"], n, seed)
    ok = _unfolded(c, cells, xi)
    assert ok.sum() >= len(ok) - 2
    return cells[ok], xi[ok]


def _in_answering_cell(m, cells, xi, answered):
    """the pairs as pairs of the cells that answered: across a shared face the face's own coordinates agree (the Q1 maps of both
    cells restrict to the same map of the shared vertices), the normal one flips between 1 and 0"""
    out = np.array(xi, float)
    for k, (c, a) in enumerate(zip(cells, answered)):
        assert a in PC.containing_cells(m, c, xi[k]), (k, c, a)
        for d in range(m.dim):
            ci, ai = c % m.reps[d], a % m.reps[d]
            c, a = c // m.reps[d], a // m.reps[d]
            if ai != ci:
                out[k, d] = 0.0 if ai > ci else 1.0
    return out


def _unfolded(c, cells, xi):
    """which pairs have det F > 0.1 in EVERY cell that contains them, by the reference.  stress_cases.py makes its states
    admissible at the quadrature points; on a cell's boundary a random nodal field can still fold (one corner point of the
    perturbed 2 x 2 x 2 Q3 case has det F = -0.11), and there the raw neo-Hookean stress is an error, not a number"""
    m = c["mesh"]
    ok = np.ones(len(cells), bool)
    for k in range(len(cells)):
        for a in PC.containing_cells(m, cells[k], xi[k]):
            x = _in_answering_cell(m, cells[k:k + 1], xi[k:k + 1], [a])
            with np.errstate(invalid="ignore"):
                ok[k] = ok[k] and SP.raw(m, c["u"], MU, NU, S.NEOHOOKE, [a], x)[1][0] > 0.1
    return ok


def _outside(c):
    hi, dim = np.array(c["hi"]), c["dim"]
    h = hi / np.array(c["reps"])
    pts = []
    for d in range(dim):
        for side in (0, 1):
            x = 0.5 * hi
            x[d] = hi[d] + 0.3 * h[d] if side else -0.3 * h[d]  # (beyond the perturbation of a face's vertices, 0.1 h)
            pts.append(x)
    return np.array(pts + [1e6 * np.ones(dim), np.full(dim, np.nan), np.array([np.nan] + list(0.5 * hi[1:])), np.full(dim, np.inf)])


def _flat(dim, s):
    return np.array([s[d, e] for d, e in S.PAIRS[dim]])


def _eig_check(dim, sigma, lam, dirs, what):
    res, orth, tr, ordered, signed = SP.eig_figures(dim, sigma, lam, dirs)
    print("%s: residual %.2f, trace %.2f eps |sigma|_F (gate %.1f), orthonormality %.2f eps (gate %.0f)" % (what, res, tr, C_RES, orth, C_ORTH))
    assert ordered and signed
    assert res <= C_RES and tr <= C_RES and orth <= C_ORTH


# ------------------------------------------------------------------ 1. affine state: the closed form everywhere
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_affine_state_has_the_closed_form_at_every_point(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    A = 0.05 * PC.Affine(dim, np.random.default_rng(4)).A
    G = _context(c)
    G.set(M.V_U, (m.coords @ A.T + 0.01).reshape(-1))
    cells, xi = _pairs(m, 33, 11)
    out = _outside(c)
    X = np.concatenate([PE.points(m, cells, xi), G.coords, out])
    n_in = len(cells) + m.nnodes
    for model in MODELS:
        want = _flat(dim, S.point_stress(dim, MU, NU, A, model)[0])
        wvm = S.von_mises(dim, want[None, :])[0]
        for kind in KINDS:
            r = G.evaluate_stress(X, model=model, kind=kind)
            es = np.abs(r["sigma"][:n_in] - want[None, :]).max() / np.abs(want).max()
            ev = np.abs(r["von_mises"][:n_in] - wvm).max() / np.abs(want).max()
            print("model %d kind %d, %d points: sigma %.2e, von Mises %.2e of max|sigma|" % (model, kind, n_in, es, ev))
            assert es <= TOL and ev <= TOL
            assert r["n_outside"] == len(out) and np.array_equal(r["cell"][n_in:], np.full(len(out), -1))
            assert np.all(r["sigma"][n_in:] == 0.0) and np.all(r["von_mises"][n_in:] == 0.0)
            assert r["cell"][:n_in].min() >= 0
            for k in range(len(cells)):
                assert r["cell"][k] in PC.containing_cells(m, cells[k], xi[k]), (k, r["cell"][k])
    G.close()


# ------------------------------------------------------------------ 2. random admissible state: against the reference
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_random_state_against_reference(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    G = _loaded(c)
    cells, xi = _pairs(m, 33, 12)
    ok = _unfolded(c, cells, xi)
    assert ok[:33].all() and (~ok).sum() <= 2
    for k in np.nonzero(~ok)[0]:  # where the answering cell (mi_evaluate_points names it) is folded, the raw neo-Hookean stress is the error
        Xk = PE.points(m, cells[k:k + 1], xi[k:k + 1])
        a = G.evaluate(M.V_U, Xk)[2]
        det = SP.raw(m, c["u"], MU, NU, S.NEOHOOKE, a, _in_answering_cell(m, cells[k:k + 1], xi[k:k + 1], a))[1][0]
        print("a folded boundary point: det F %.3f in the answering cell %d" % (det, a[0]))
        if det < -0.01:
            with pytest.raises(M.MiError) as err:
                G.evaluate_stress(Xk, kind=M.STRESS_AT_RAW)
            assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    cells, xi = cells[ok], xi[ok]
    X = PE.points(m, cells, xi)
    for model in MODELS:
        nodal, nodal_vm, _ = G.stress_field(model)
        smax = np.abs(nodal).max()
        # raw: the reference in the cell that answered
        r = G.evaluate_stress(X, model=model, kind=M.STRESS_AT_RAW)
        assert r["n_outside"] == 0 and np.array_equal(r["cell"][:33], cells[:33])
        ref, det = SP.raw(m, c["u"], MU, NU, model, r["cell"], _in_answering_cell(m, cells, xi, r["cell"]))
        e_raw = np.abs(r["sigma"] - ref).max() / np.abs(ref).max()
        e_vm = np.abs(r["von_mises"] - S.von_mises(dim, r["sigma"])).max() / np.abs(ref).max()
        # recovered: numpy interpolation of the device's own nodal field; at the nodes the nodal field itself
        q = G.evaluate_stress(X, model=model, kind=M.STRESS_AT_RECOVERED)
        e_rec = np.abs(q["sigma"] - SP.interpolate(m, nodal, cells, xi)).max() / smax
        e_rvm = np.abs(q["von_mises"] - S.von_mises(dim, q["sigma"])).max() / smax
        at_nodes = G.evaluate_stress(G.coords, model=model, kind=M.STRESS_AT_RECOVERED)
        e_nod = np.abs(at_nodes["sigma"] - nodal).max() / smax
        e_nvm = np.abs(at_nodes["von_mises"] - nodal_vm).max() / smax
        # raw at every point of the model's rule, projected in numpy: the nodal field of stress_q2 / stress_q3 / stress_cells
        qc, qxi, N, JxW = SP.quadrature_pairs(m, model)
        rq = G.evaluate_stress(PE.points(m, qc, qxi), model=model, kind=M.STRESS_AT_RAW)
        assert rq["n_outside"] == 0 and np.array_equal(rq["cell"], qc)
        e_prj = np.abs(SP.lumped(m, qc, rq["sigma"], N, JxW) - nodal).max() / smax
        print("model %d, min det F %.2f: raw %.2e, recovered %.2e, at nodes %.2e, raw projected %.2e, von Mises %.2e %.2e %.2e" %
              (model, det.min(), e_raw, e_rec, e_nod, e_prj, e_vm, e_rvm, e_nvm))
        assert e_raw <= TOL and e_rec <= TOL and e_nod <= TOL and e_prj <= TOL
        assert e_vm <= TOL and e_rvm <= TOL and e_nvm <= TOL
        assert at_nodes["n_outside"] == 0
    G.close()


# ------------------------------------------------------------------ 3. principal stresses, through both entry points
@pytest.mark.parametrize("dim", [2, 3])
def test_principal_stresses_of_given_tensors(dim):
    c = SC.case(*(SC.Q2_MESHES[0] if dim == 3 else SC.GENERIC_MESHES[0]), False)
    G = _context(c)
    T = SP.eig_tensors(dim)
    lam, dirs = G.principal_stress(T, directions=True)
    _eig_check(dim, T, lam, dirs, "%dD, %d tensors" % (dim, len(T)))
    ref = SP.principal(dim, T)[0]
    scale = np.array([max(np.linalg.norm(SP.full_tensor(dim, a)), 1e-300) for a in T])
    assert (np.abs(lam - ref).max(axis=1) <= C_RES * SP.EPS * scale).all()
    again = G.principal_stress(T, directions=True)
    assert again[0].tobytes() == lam.tobytes() and again[1].tobytes() == dirs.tobytes()
    assert G.principal_stress(T)[0].tobytes() == lam.tobytes() and G.principal_stress(T)[1] is None
    for k in (64, 65, 66):  # hydrostatic and zero: the basis of the statements, the coordinate axes
        assert np.array_equal(dirs[k], np.eye(dim)) and np.array_equal(lam[k], T[k, :dim])
    many = np.tile(T, (8, 1))  # more than one workgroup
    assert G.principal_stress(many, directions=True)[1].tobytes() == np.tile(dirs, (8, 1, 1)).tobytes()
    assert G.principal_stress(np.zeros((0, T.shape[1])))[0].shape == (0, dim)
    G.close()


@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[1], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1], SC.GENERIC_MESHES[5]])
def test_principal_stresses_at_points(mesh):
    c = SC.case(*mesh, True)
    m, dim = c["mesh"], c["dim"]
    G = _loaded(c)
    cells, xi = _unfolded_pairs(c, 33, 13)
    X = np.concatenate([PE.points(m, cells, xi), _outside(c)])
    for model in MODELS:
        for kind in KINDS:
            r = G.evaluate_stress(X, model=model, kind=kind, principal=True, directions=True)
            _eig_check(dim, r["sigma"], r["principal"], r["directions"], "model %d kind %d, %d points" % (model, kind, len(X)))
            lam, dirs = G.principal_stress(r["sigma"], directions=True)  # the same kernel on the same tensors
            assert lam.tobytes() == r["principal"].tobytes() and dirs.tobytes() == r["directions"].tobytes()
            only = G.evaluate_stress(X, model=model, kind=kind, principal=True)
            assert only["principal"].tobytes() == r["principal"].tobytes() and only["directions"] is None
            assert np.array_equal(r["directions"][len(cells):], np.tile(np.eye(dim), (len(X) - len(cells), 1, 1)))
    G.close()


# ------------------------------------------------------------------ 4. the contract
def _all_bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("sigma", "von_mises", "principal", "directions", "cell"))


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[1], SC.GENERIC_MESHES[3]])
def test_two_calls_give_the_same_bits(mesh, perturbed):
    c = SC.case(*mesh, perturbed)
    m = c["mesh"]
    G = _loaded(c)
    X = np.concatenate([PE.points(m, *_unfolded_pairs(c, 257, 14)), _outside(c)])
    for model in MODELS:
        for kind in KINDS:
            a = G.evaluate_stress(X, model=model, kind=kind, principal=True, directions=True)
            G.evaluate_stress(X[:5], model=1 - model, kind=1 - kind)  # (another call in between)
            b = G.evaluate_stress(X, model=model, kind=kind, principal=True, directions=True)
            assert _all_bits(a) == _all_bits(b) and a["n_outside"] == b["n_outside"] == len(_outside(c))
            plain = G.evaluate_stress(X, model=model, kind=kind)  # without the principal values: the same tensors
            assert plain["sigma"].tobytes() == a["sigma"].tobytes() and plain["principal"] is None
    G.close()


@pytest.mark.parametrize("mesh", [SC.Q2_MESHES[0], SC.Q3_MESHES[0], SC.GENERIC_MESHES[1]])
def test_evaluation_changes_nothing(mesh):
    c = SC.case(*mesh, True)
    m = c["mesh"]
    X = PE.points(m, *_pairs(m, 33, 15))

    def ask(Y):
        for model in MODELS:
            for kind in KINDS:
                Y.evaluate_stress(X, model=model, kind=kind, principal=True, directions=True)
        Y.principal_stress(SP.eig_tensors(c["dim"]), directions=True)

    G, H = _context(c), _context(c)
    for Y in (G, H):
        Y.set_profiling(True)
        Y.set_interface_traction((0.0, -50.0, 0.0)[:c["dim"]])
        Y.newmark_step(tol_lin=1e-10)
    vecs = [G.get(w) for w in range(10)]
    counts = {k: v[1] for k, v in G.timings().items()}
    ask(G)
    assert counts == {k: v[1] for k, v in G.timings().items()}
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
    ask(G)
    assert G.linear_step(1, 1e-12) == H.linear_step(1, 1e-12)
    for w in range(10):
        assert np.array_equal(G.get(w), H.get(w)), w
    G.close()
    H.close()


@pytest.mark.parametrize("perturbed", [False, True])
def test_same_values_under_the_operator_modes(perturbed):
    c = SC.case(*SC.Q2_MESHES[1], perturbed)
    m = c["mesh"]
    X = PE.points(m, *_unfolded_pairs(c, 33, 16))
    G = _loaded(c)
    want = [_all_bits(G.evaluate_stress(X, model=mo, kind=k, principal=True, directions=True)) for mo in MODELS for k in KINDS]

    def same():
        got = [_all_bits(G.evaluate_stress(X, model=mo, kind=k, principal=True, directions=True)) for mo in MODELS for k in KINDS]
        assert got == want

    G.set_tuning("fine_level", 1)
    G.assemble()
    same()
    G.set_tuning("linear_operator", 2)  # the matrix-free linear set-up releases the tangent array and clears the state vectors
    G.linear_setup(0.5)
    assert G.get_tuning("linear_operator_active") == 2
    G.set(M.V_U, c["u"])
    same()
    G.close()


@pytest.mark.parametrize("mesh", [SC.Q3_MESHES[0], SC.Q2_MESHES[0], SC.GENERIC_MESHES[1]])
def test_folded_point_and_folded_cell_are_reported(mesh):
    c = SC.case(*mesh, True)
    m = c["mesh"]
    qc, qxi, _, _ = SP.quadrature_pairs(m, S.NEOHOOKE)
    s = 2.0
    with np.errstate(invalid="ignore"):
        while True:
            det = SP.raw(m, s * c["u"], MU, NU, S.NEOHOOKE, qc, qxi)[1]
            if det.min() < -0.05:
                break
            s *= 2.0
    bad, good = int(np.argmin(det)), np.nonzero(det > 0.2)[0]
    assert len(good) > 0
    Xq = PE.points(m, qc, qxi)
    G = _loaded(c)
    G.set(M.V_U, s * c["u"])
    with pytest.raises(M.MiError) as err:
        G.evaluate_stress(Xq[[good[0], bad]], kind=M.STRESS_AT_RAW)
    assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    with pytest.raises(M.MiError) as err:  # the recovered field needs the whole mesh: a fold anywhere is an error
        G.evaluate_stress(Xq[good[:3]], kind=M.STRESS_AT_RECOVERED)
    assert err.value.code == M.MI_EINVAL and "inverted element" in str(err.value)
    r = G.evaluate_stress(Xq[good], kind=M.STRESS_AT_RAW)  # the raw stress asks about its own points alone
    ref = SP.raw(m, s * c["u"], MU, NU, S.NEOHOOKE, qc[good], qxi[good])[0]
    assert np.abs(r["sigma"] - ref).max() <= TOL * np.abs(ref).max()
    lin = G.evaluate_stress(Xq, model=M.STRESS_LINEAR, kind=M.STRESS_AT_RAW)  # no such case in the linear model
    ref = SP.raw(m, s * c["u"], MU, NU, S.LINEAR, qc, qxi)[0]
    assert np.abs(lin["sigma"] - ref).max() <= TOL * np.abs(ref).max()
    G.set(M.V_U, c["u"])  # the context works afterwards
    for kind in KINDS:
        assert np.abs(G.evaluate_stress(Xq[:9], kind=kind)["sigma"]).max() > 0
    assert G.assemble() > 0
    G.close()


def test_teams_are_refused():
    c = SC.case(*SC.TEAM_MESHES[0], True)
    T = _loaded(c, slabs=2)
    assert T.comm_info()[0] == 2
    for kind in KINDS:
        with pytest.raises(M.MiError) as err:
            T.evaluate_stress(np.full((1, 3), 0.05), kind=kind)
        assert err.value.code == M.MI_EINVAL and "one slab only" in str(err.value)
    lam, dirs = T.principal_stress(SP.eig_tensors(3), directions=True)  # reads no state: any context will do
    _eig_check(3, SP.eig_tensors(3), lam, dirs, "on a team")
    T.close()


def test_argument_errors():
    c = SC.case(*SC.GENERIC_MESHES[1], False)
    G = _loaded(c)
    L = M.lib()
    X = np.array([[0.05, 0.05], [0.2, 0.1]])
    sig = np.full((2, 3), 7.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    nout = C.c_int64(5)
    assert L.mi_evaluate_stress(None, 0, 0, 2, dp(X), dp(sig), None, None, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_stress(G.h, 0, 0, 2, None, dp(sig), None, None, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_stress(G.h, 0, 0, 2, dp(X), None, None, None, None, None, None) == M.MI_EINVAL
    assert L.mi_evaluate_stress(G.h, 0, 0, -1, dp(X), dp(sig), None, None, None, None, None) == M.MI_EINVAL
    for bad in (-1, 2):
        assert L.mi_evaluate_stress(G.h, bad, 0, 2, dp(X), dp(sig), None, None, None, None, None) == M.MI_EINVAL
        assert L.mi_evaluate_stress(G.h, 0, bad, 2, dp(X), dp(sig), None, None, None, None, None) == M.MI_EINVAL
    assert np.all(sig == 7.0)
    assert L.mi_evaluate_stress(G.h, 0, 1, 0, dp(X), dp(sig), None, None, None, None, C.byref(nout)) == M.MI_OK  # no points
    assert np.all(sig == 7.0) and nout.value == 0
    assert L.mi_evaluate_stress(G.h, 0, 0, 2, dp(X), dp(sig), None, None, None, None, None) == M.MI_OK  # all but sigma optional
    assert np.array_equal(sig, G.evaluate_stress(X)["sigma"])
    lam = np.full((2, 2), 7.0)
    assert L.mi_principal_stress(None, 2, dp(sig), dp(lam), None) == M.MI_EINVAL
    assert L.mi_principal_stress(G.h, 2, None, dp(lam), None) == M.MI_EINVAL
    assert L.mi_principal_stress(G.h, 2, dp(sig), None, None) == M.MI_EINVAL
    assert L.mi_principal_stress(G.h, -1, dp(sig), dp(lam), None) == M.MI_EINVAL
    assert L.mi_principal_stress(G.h, 0, None, None, None) == M.MI_OK and np.all(lam == 7.0)
    assert L.mi_principal_stress(G.h, 2, dp(sig), dp(lam), None) == M.MI_OK
    assert np.array_equal(lam, G.principal_stress(sig)[0])
    G.close()
