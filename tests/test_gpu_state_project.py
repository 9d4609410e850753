"""GPU: mi_project_load and mi_state_project (Context.project_load, Context.project_state_from) -- the load of a source mesh's
fields on the composite rule and the L2 projection of its six state vectors -- against the dense numpy reference
tests/golden/projection_reference.py and against what a projection is.

Pairs: projection_cases.EXACT_PAIRS (identity, refinement, nested coarsening Q2 / Q3 with sub 2, degree drop on boxes and on a
perturbed lattice, a 2D coarsening with sub 3), NON_NESTED (3 x 2 x 3 -> 2 x 2 x 2 on the same box) and one pair per (dim,
degree) for the load kernel's eight instances.  Source states: random vectors with zeros on the constrained dofs.

Tolerances, each figure printed before it is asserted:
  load         1e-12 relmax against the reference: the family's gate for direct sums (device sums against numpy).
  solve bound  |w - w*|_2 <= kappa_2(M_ff) (res + 64 eps) |w*|_2 per vector, as test_gpu_mass.py: w* the dense projection, kappa_2
               numpy's on dst's mesh, res what the call reports; plus 1e-12 |w*| where w* itself comes through an evaluation.
  residual     |(b - M w)_f|_2 <= (res + 64 eps) |b_f|_2 with the device's own b and M w.
  Pythagoras   |src_sq - dst_sq - int |w_src - w_dst|^2| <= (1e-12 + 2 kappa_2 (res + 64 eps)) src_sq: for w = w* + d with d in
               dst's space the defect is -2 (w*, d)_M - 2 |d|_M^2, and |d|_M / |w*|_M is within the solve bound.
  sums         |sum_i (M w - b)_i| <= sqrt(n) (res + 64 eps) |b|_2 + n eps |b|_1 with all faces free.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import point_eval_cases as PC  # noqa: E402
import projection_cases as PJ  # noqa: E402
import projection_reference as PR  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
TOL_SUM, TOL_SOLVE = 1e-12, 1e-12
SIX = [M.V_U, M.V_U_OLD, M.V_V, M.V_V_OLD, M.V_A, M.V_A_OLD]
REST = [M.V_STRESS, M.V_DELTA, M.V_NEWTON, M.V_RHS]
FREE = [0] * 6
ALL_PAIRS = PJ.EXACT_PAIRS + [PJ.NON_NESTED]
# the load kernel's other instances: src and dst on the same perturbed lattice, dst one degree lower where there is one
INSTANCE_PAIRS = [("%dD-Q%d" % (dim, p), (dim, min(p + 1, 4), PJ.REPS[dim], True, 1), (dim, p, PJ.REPS[dim], True, 1), 1)
                  for dim, p in ((3, 1), (3, 3), (3, 4), (2, 2), (2, 3), (2, 4))]
SUB3_3D = ("coarsen-3D-Q2-sub3", (3, 2, (1, 1, 1), False, 3), (3, 2, (1, 1, 1), False, 1), 3)
_ref = {}


def _loaded(c, state, **kw):
    G = PC.context(M, c, **kw)
    for w, v in enumerate(state):
        G.set(w, v)
    return G


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _reference(case):
    """(src dict, dst dict, sub, src state, b*, src_sq*, w*, dense mass of dst, kappa_2): computed once, left unchanged"""
    if case[0] not in _ref:
        cs, cd, sub = PJ.pair(case)
        state = PJ.source_state(cs)
        md = cd["mesh"]
        b, sq = PR.load(md, cs["mesh"], state[:6], sub)
        Md = PR.scalar_mass(md)
        _ref[case[0]] = (cs, cd, sub, state, b, sq, PR.solve(Md, b, md.dim, md.constrained), Md, PR.kappa2(Md, md.dim, md.constrained))
    return _ref[case[0]]


# ------------------------------------------------------------------ 1. the load
@pytest.mark.parametrize("case", ALL_PAIRS + INSTANCE_PAIRS + [SUB3_3D], ids=PJ.pair_id)
def test_load_against_the_reference(case):
    cs, cd, sub = PJ.pair(case)
    state = PJ.source_state(cs)
    S, D = _loaded(cs, state), PC.context(M, cd)
    which = [M.V_V, M.V_U]
    b = D.project_load(S, which, sub=sub)
    ref, _ = PR.load(cd["mesh"], cs["mesh"], state[which], sub)
    print("%s: load relmax %.2e" % (case[0], _relmax(b, ref)))
    assert _relmax(b, ref) <= TOL_SUM
    one = D.project_load(S, M.V_U, sub=sub)  # a vector's load does not depend on its neighbours
    assert one.tobytes() == b[1].tobytes()
    S.close(), D.close()


@pytest.mark.parametrize("case", [PJ.EXACT_PAIRS[2], PJ.EXACT_PAIRS[5], PJ.NON_NESTED], ids=PJ.pair_id)
def test_chunk_size_does_not_change_a_bit(case):
    cs, cd, sub = PJ.pair(case)
    state = PJ.source_state(cs)
    S, D, E = _loaded(cs, state), _loaded(cd, PJ.source_state(cd, 12)), _loaded(cd, PJ.source_state(cd, 12))
    auto = D.project_load(S, SIX, sub=sub)
    again = D.project_load(S, SIX, sub=sub)
    D.set_tuning("project_chunk_cells", 1)
    assert D.get_tuning("project_chunk_cells") == 1
    one = D.project_load(S, SIX, sub=sub)
    assert auto.tobytes() == again.tobytes() == one.tobytes()
    ia, ib = E.project_state_from(S, sub=sub), D.project_state_from(S, sub=sub)
    assert ia["src_sq"].tobytes() == ib["src_sq"].tobytes() and ia["dst_sq"].tobytes() == ib["dst_sq"].tobytes()
    for w in range(10):
        assert D.get(w).tobytes() == E.get(w).tobytes()
    for G in (S, D, E):
        G.close()


# ------------------------------------------------------------------ 2. the definition, bit for bit; purity
@pytest.mark.parametrize("case", [PJ.EXACT_PAIRS[3], PJ.EXACT_PAIRS[5], PJ.NON_NESTED, INSTANCE_PAIRS[4]], ids=PJ.pair_id)
def test_equals_the_host_route(case):
    cs, cd, sub = PJ.pair(case)
    s_state, d_state = PJ.source_state(cs), PJ.source_state(cd, seed=12)
    S, D, H = _loaded(cs, s_state), _loaded(cd, d_state), _loaded(cd, d_state)
    info = D.project_state_from(S, sub=sub)
    b = H.project_load(S, SIX, sub=sub)
    x, its, res, _ = H.mass_solve(b, masked=True, tol=1e-12, max_it=500)
    for k, w in enumerate(SIX):
        H.set(w, x[k])
    for w in range(10):
        assert D.get(w).tobytes() == H.get(w).tobytes(), w
    assert info["its"] == its and info["res"] == res.max() and info["sub"] == sub
    assert info["n_points"] == D.ncells * (sub * (cd["p"] + 2)) ** cd["dim"]
    for w in SIX:
        assert np.all(D.get(w)[D.constrained] == 0.0)
    for w in REST:  # nothing else in dst, nothing in src
        assert np.array_equal(D.get(w), d_state[w]), w
    for w in range(10):
        assert np.array_equal(S.get(w), s_state[w]), w
    for G in (S, D, H):
        G.close()


def test_following_steps_are_unchanged():
    """a Newmark step of src after it was projected from, and of a twin that never was, return the same bits"""
    cs, cd, sub = PJ.pair(PJ.EXACT_PAIRS[2])
    t = (0.0, -50.0, 0.0)
    S, K, D = PC.context(M, cs), PC.context(M, cs), PC.context(M, cd)
    for G in (S, K):
        G.set_interface_traction(t)
        G.newmark_step(tol_lin=1e-12)
    D.project_state_from(S, sub=sub)
    D.project_load(S, SIX, sub=sub)
    S.mass_solve(S.get(M.V_RHS), masked=True)
    for G in (S, K):
        G.newmark_step(tol_lin=1e-12)
    for w in range(10):
        assert S.get(w).tobytes() == K.get(w).tobytes(), w
    for G in (S, K, D):
        G.close()


# ------------------------------------------------------------------ 3. the cases and what a projection is
@pytest.mark.parametrize("case", ALL_PAIRS, ids=PJ.pair_id)
def test_projection_properties(case):
    cs, cd, sub, state, b_ref, sq_ref, w_ref, Md, kappa = _reference(case)
    ms, md = cs["mesh"], cd["mesh"]
    S, D = _loaded(cs, state), PC.context(M, cd)
    info = D.project_state_from(S, sub=sub, tol=TOL_SOLVE)
    w = np.array([D.get(k) for k in SIX])
    slack = info["res"] + 64 * EPS
    # against the dense projection
    err = np.linalg.norm(w - w_ref, axis=1) / np.linalg.norm(w_ref, axis=1)
    print("%s: kappa_2 %.1f, %d iterations, res %.2e, |w - w*| / |w*| %.2e (bound %.2e)" %
          (case[0], kappa, info["its"], info["res"], err.max(), kappa * slack + TOL_SUM))
    assert info["res"] <= TOL_SOLVE
    assert np.all(err <= kappa * slack + TOL_SUM)
    assert np.all(w[:, md.constrained] == 0.0)
    # the free-dof residual, with the device's own load and product
    b = D.project_load(S, SIX, sub=sub)
    r = (b - D.mass_apply(w))[:, ~md.constrained]
    rel = np.linalg.norm(r, axis=1) / np.linalg.norm(b[:, ~md.constrained], axis=1)
    print("    free-dof residual %.2e" % rel.max())
    assert np.all(rel <= slack)
    # never more of int |w|^2 than the source has; the two sums against the reference
    print("    src_sq relmax %.2e, dst_sq / src_sq %s" % (_relmax(info["src_sq"], sq_ref), info["dst_sq"] / info["src_sq"]))
    assert _relmax(info["src_sq"], sq_ref) <= TOL_SUM
    assert np.all(info["dst_sq"] <= info["src_sq"] * (1 + 1e-12))
    dst_sq = np.einsum("kn,kn->k", w, PR.mass_apply(Md, w, md.dim))
    assert _relmax(info["dst_sq"], dst_sq) <= TOL_SUM
    err_sq = PR.error_sq(md, ms, state[:6], w, sub)
    if case in PJ.EXACT_PAIRS:
        defect = np.abs(info["src_sq"] - info["dst_sq"] - err_sq) / info["src_sq"]
        print("    Pythagoras defect %.2e (bound %.2e)" % (defect.max(), TOL_SUM + 2 * kappa * slack))
        assert np.all(defect <= TOL_SUM + 2 * kappa * slack)
    # what the case is about
    T = PC.context(M, cd)
    T.transfer_state_from(S)
    wt = np.array([T.get(k) for k in SIX])
    T.close()
    if case[0] == "identity":
        assert np.all(np.linalg.norm(w - state[:6], axis=1) <= (kappa * slack + TOL_SUM) * np.linalg.norm(state[:6], axis=1))
    if case[0] == "refine-Q2":  # src's space lies in dst's: the projection is the interpolation
        assert np.all(np.linalg.norm(w - wt, axis=1) <= (kappa * slack + TOL_SUM) * np.linalg.norm(wt, axis=1))
    if case[0] in PJ.SAMPLING_LOSES or case[0] == "non-nested":
        sampled = PR.error_sq(md, ms, state[:6], wt, sub)
        print("    int |w_src - w_dst|^2: projected %s, sampled %s" % (err_sq, sampled))
        assert np.all(sampled > err_sq)
    S.close(), D.close()


def test_sums_are_conserved_with_all_faces_free():
    cs, cd, sub = PJ.pair(PJ.EXACT_PAIRS[2], roles=FREE)
    state = np.random.default_rng(4).standard_normal((10, cs["mesh"].n))
    S, D = _loaded(cs, state), PC.context(M, cd)
    assert not D.constrained.any()
    info = D.project_state_from(S, sub=sub)
    w = np.array([D.get(k) for k in SIX])
    b, Mw = D.project_load(S, SIX, sub=sub), D.mass_apply(w)
    n = b.shape[1]
    bound = np.sqrt(n) * (info["res"] + 64 * EPS) * np.linalg.norm(b, axis=1) + n * EPS * np.abs(b).sum(axis=1)
    print("sum (M w - b): %s, bound %s" % (np.abs((Mw - b).sum(axis=1)), bound))
    assert np.all(np.abs((Mw - b).sum(axis=1)) <= bound)
    S.close(), D.close()


def test_modes_of_the_contexts():
    """ "fine_level" 1 on both sides and a "linear_operator" 1 set-up return the bits of plain contexts"""
    cs = cd = PC.make_mesh(3, 3, PJ.REPS[3], True)  # Q3 -> Q3 on the perturbed lattice: the matrix-free linear model is Q3's
    sub = 1
    state = PJ.source_state(cs)
    S, D = _loaded(cs, state), PC.context(M, cd)
    D.project_state_from(S, sub=sub)
    want = [D.get(k) for k in SIX]
    S.close(), D.close()
    for key in ("fine_level", "linear_operator"):
        S, D = _loaded(cs, state), PC.context(M, cd)
        for G in (S, D):
            G.set_tuning(key, 1)
            if key == "linear_operator":
                G.linear_setup(0.5)
        for k, v in enumerate(state[:6]):  # (a linear set-up may have touched the vectors)
            S.set(k, v)
        D.project_state_from(S, sub=sub)
        for k in range(6):
            assert D.get(SIX[k]).tobytes() == want[k].tobytes(), (key, k)
        S.close(), D.close()


# ------------------------------------------------------------------ 4. errors
def test_errors_leave_dst_unchanged():
    cs = PC.make_mesh(3, 2, PJ.REPS[3], False)
    cd = PC.make_mesh(3, 2, PJ.REPS[3], False, lo=(0.05, 0.0, 0.0))  # the same cells, moved half a cell along x
    d_state = PJ.source_state(cd, seed=12)
    S, D, E = _loaded(cs, PJ.source_state(cs)), _loaded(cd, d_state), _loaded(cs, d_state)
    with pytest.raises(M.MiError) as err:
        D.project_state_from(S)
    assert err.value.code == M.MI_EINVAL and "outside src's mesh" in str(err.value)
    cell = int(re.search(r"dst's cell (\d+)", str(err.value)).group(1))
    assert cell % 3 == 2, cell  # a cell of the last layer along x: those stick out
    with pytest.raises(M.MiError):
        D.project_load(S, SIX)
    with pytest.raises(M.MiError) as err:  # no convergence: nothing is written either
        E.project_state_from(S, max_it=2)
    assert err.value.code == M.MI_ENOCONV_LIN
    for G in (D, E):
        for w in range(10):
            assert np.array_equal(G.get(w), d_state[w]), w
    for G in (S, D, E):
        G.close()


def test_refusals():
    c3, c2 = PC.make_mesh(3, 2, (2, 2, 4), False), PC.make_mesh(2, 2, (3, 2), False)
    A, A2, B, T = PC.context(M, c3), PC.context(M, c3), PC.context(M, c2), PC.context(M, c3, slabs=2)
    assert T.comm_info()[0] == 2
    for dst, src, sub, text in ((A, B, 1, "2D"), (B, A, 1, "3D"), (T, A, 1, "one slab only"), (A, T, 1, "one slab only"),
                                (A, A2, 0, "sub"), (A, A2, 5, "sub")):
        for call in (lambda: dst.project_state_from(src, sub=sub), lambda: dst.project_load(src, SIX, sub=sub)):
            with pytest.raises(M.MiError) as err:
                call()
            assert err.value.code == M.MI_EINVAL and text in str(err.value)
    L = M.lib()
    ids = (C.c_int * 7)(*range(7))
    b = np.zeros((7, A.n))
    bp = b.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mi_state_project(None, A.h, 1, 1e-12, 10, None) == M.MI_EINVAL
    assert L.mi_state_project(A.h, None, 1, 1e-12, 10, None) == M.MI_EINVAL
    assert L.mi_state_project(A.h, A2.h, 1, -1.0, 10, None) == M.MI_EINVAL
    assert L.mi_project_load(None, A.h, 1, ids, 1, bp) == M.MI_EINVAL and L.mi_project_load(A.h, None, 1, ids, 1, bp) == M.MI_EINVAL
    assert L.mi_project_load(A.h, A2.h, 7, ids, 1, bp) == M.MI_EINVAL
    assert L.mi_project_load(A.h, A2.h, 1, None, 1, bp) == M.MI_EINVAL and L.mi_project_load(A.h, A2.h, 1, ids, 1, None) == M.MI_EINVAL
    bad = (C.c_int * 1)(10)
    assert L.mi_project_load(A.h, A2.h, 1, bad, 1, bp) == M.MI_EINVAL
    assert L.mi_project_load(A.h, A2.h, 0, None, 1, None) == M.MI_OK
    assert np.all(b == 0.0)
    for G in (A, A2, B, T):
        G.close()
