"""GPU: mi_state_transfer (Context.transfer_state_from) against its definition -- mi_evaluate_points of src at dst's node
coordinates, set into dst, constrained dofs zeroed -- bit for bit, against tests/golden/point_eval_reference.py and through
properties an independent kernel checks (mi_energy).

The src vectors are random with zeros on the constrained dofs; both contexts carry the same face roles, so a field that vanishes on
src's constrained faces vanishes at dst's constrained nodes too.  Meshes of tests/golden/point_eval_cases.py: boxes with edges
0.1, 0.13, 0.07, refine = 2 halves every cell.  Tolerances: 1e-12 relmax for everything that is an evaluation (the standing tolerance
of device sums against numpy; every figure is printed), 1e-8 for a Newmark step (the suite's step tolerance), the same bits where
the definition says so.
"""
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import point_eval_cases as PC  # noqa: E402
import point_eval_reference as PE  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

TOL, TOL_STEP = 1e-12, 1e-8
SIX = [M.V_U, M.V_U_OLD, M.V_V, M.V_V_OLD, M.V_A, M.V_A_OLD]
REST = [M.V_STRESS, M.V_DELTA, M.V_NEWTON, M.V_RHS]
REPS = {2: (3, 2), 3: (3, 2, 3)}


def _random_state(c, seed=11):
    m = c["mesh"]
    return np.random.default_rng(seed + m.n).standard_normal((10, m.n)) * ~m.constrained


def _loaded(c, state, **kw):
    G = PC.context(M, c, **kw)
    for w, v in enumerate(state):
        G.set(w, v)
    return G


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("pair", [((3, 2, False, 1), (3, 2, False, 2)), ((3, 2, True, 1), (3, 3, True, 1)), ((3, 3, True, 1), (3, 2, True, 1)),
                                  ((2, 1, True, 1), (2, 4, True, 1)), ((3, 4, False, 1), (3, 1, False, 2)), ((2, 3, False, 1), (2, 3, False, 1))])
def test_equals_the_host_route(pair):
    (dim, ps, perturbed, rs), (_, pd, _, rd) = pair
    cs, cd = PC.make_mesh(dim, ps, REPS[dim], perturbed, refine=rs), PC.make_mesh(dim, pd, REPS[dim], perturbed and rd == rs, refine=rd)
    s_state, d_state = _random_state(cs), _random_state(cd, seed=12)
    S, D, H = _loaded(cs, s_state), _loaded(cd, d_state), _loaded(cd, d_state)
    D.transfer_state_from(S)
    val, _, cell, nout = S.evaluate(SIX, H.coords)  # the host route on the twin
    assert nout == 0 and cell.min() >= 0
    for k, w in enumerate(SIX):
        v = val[k].reshape(-1).copy()
        v[H.constrained] = 0.0
        H.set(w, v)
    for w in range(10):
        assert D.get(w).tobytes() == H.get(w).tobytes(), w
    for w in SIX:
        assert np.all(D.get(w)[D.constrained] == 0.0)
    for w in REST:  # nothing else in dst, nothing in src
        assert np.array_equal(D.get(w), d_state[w]), w
    for w in range(10):
        assert np.array_equal(S.get(w), s_state[w]), w
    for G in (S, D, H):
        G.close()


# ------------------------------------------------------------------ 2. identity and continuation
@pytest.mark.parametrize("mesh", [(3, 2, True), (3, 3, False), (2, 2, True)])
def test_identity_transfer_and_continuation(mesh):
    dim, p, perturbed = mesh
    c = PC.make_mesh(dim, p, REPS[dim], perturbed)
    t = (0.0, -50.0, 0.0)[:dim]
    S, D, K = PC.context(M, c), PC.context(M, c), PC.context(M, c)
    S.set_interface_traction(t)
    S.newmark_step(tol_lin=1e-12)  # a state with every vector in use
    D.transfer_state_from(S)
    for w in SIX:
        a, b = D.get(w), S.get(w)
        if np.abs(b).max() > 0:
            print("vector %d: %.2e" % (w, _relmax(a, b)))
            assert _relmax(a, b) < TOL
        else:
            assert not a.any()
        K.set(w, b)  # the control context gets the same vectors through mi_vec_set
    for G in (D, K):
        G.set_interface_traction(t)
        G.newmark_step(tol_lin=1e-12)
    err = _relmax(D.get(M.V_U), K.get(M.V_U))
    print("step after the transfer against the control: %.2e" % err)
    assert err < TOL_STEP
    for G in (S, D, K):
        G.close()


# ------------------------------------------------------------------ 3. nested refinement on boxes: exact
def _same_field(cs, S, cd, D, n=257):
    """src and dst evaluated at the same random points"""
    md = cd["mesh"]
    X = PE.points(md, *PC.interior_pairs(md, n, np.random.default_rng(21)))
    a, _, _, na = S.evaluate(SIX, X)
    b, _, _, nb = D.evaluate(SIX, X)
    assert na == 0 and nb == 0
    return _relmax(b, a)


@pytest.mark.parametrize("pair", [((3, 2, (3, 2, 3), 1), (3, 2, 2)), ((3, 1, (3, 2, 3), 1), (3, 2, 1)), ((3, 3, (3, 2, 3), 1), (3, 4, 1)),
                                  ((2, 3, (3, 2), 1), (2, 3, 2)), ((2, 2, (3, 2), 1), (2, 3, 2)), ((3, 2, (8, 8, 8), 1), (3, 2, 2))])
def test_nested_refinement_is_exact_and_round_trips(pair):
    (dim, ps, reps, rs), (_, pd, rd) = pair
    cs, cd = PC.make_mesh(dim, ps, reps, False, refine=rs), PC.make_mesh(dim, pd, reps, False, refine=rd)
    s_state = _random_state(cs)
    S, D, B = _loaded(cs, s_state), PC.context(M, cd), PC.context(M, cs)
    D.transfer_state_from(S)
    err = _same_field(cs, S, cd, D)
    print("%dD Q%d %s -> Q%d x%d: the two fields at the same points %.2e" % (dim, ps, reps, pd, rd, err))
    assert err < TOL
    # against the reference's pairs as well: the nodes of dst as (src cell, xi)
    cells, xi = PE.refine_pairs(cs["mesh"], cd["mesh"])
    for w in (M.V_U, M.V_A_OLD):
        ref, _ = PE.evaluate_batch(cs["mesh"], s_state[w], cells, xi)
        ref = ref.reshape(-1) * ~cd["mesh"].constrained
        assert _relmax(D.get(w), ref) < TOL
    B.transfer_state_from(D)  # back onto src's mesh
    back = max(_relmax(B.get(w), s_state[w]) for w in SIX)
    print("round trip %.2e" % back)
    assert back < TOL
    for G in (S, D, B):
        G.close()


@pytest.mark.parametrize("pair", [((3, 2, (3, 2, 3)), (3, 2, 2)), ((3, 2, (3, 2, 3)), (3, 3, 1)), ((2, 3, (3, 2)), (2, 4, 2))])
def test_energies_are_preserved(pair):
    """kinetic energy and body potential of dst equal src's: both integrands have degree <= 2 p per direction, which the rule
    QGauss(p' + 2), p' >= p, integrates exactly -- the transfer checked through mi_energy, an independent kernel.  u points along
    the body force everywhere, so the potential is a sum of terms of one sign"""
    (dim, ps, reps), (_, pd, rd) = pair
    body = (0.3, -9.81, 1.0)
    cs, cd = PC.make_mesh(dim, ps, reps, False), PC.make_mesh(dim, pd, reps, False, refine=rd)
    ms = cs["mesh"]
    rng = np.random.default_rng(31)
    state = _random_state(cs)
    u = 1e-3 * min(PC.EDGE[:dim]) * np.abs(rng.standard_normal((ms.nnodes, dim))) * np.sign(body[:dim])
    state[M.V_U] = u.reshape(-1) * ~ms.constrained
    S, D = _loaded(cs, state, body_force=body, rho=870.0), PC.context(M, cd, body_force=body, rho=870.0)
    D.transfer_state_from(S)
    es, ed = S.energy(), D.energy()
    for k in ("kinetic", "body"):
        err = abs(ed[k] - es[k]) / abs(es[k])
        print("%s: src %.17g dst %.17g rel %.2e" % (k, es[k], ed[k], err))
        assert abs(es[k]) > 0 and err < TOL
    S.close()
    D.close()


# ------------------------------------------------------------------ 4. a non-nested pair: sampling
@pytest.mark.parametrize("dim,perturbed", [(3, False), (3, True), (2, True)])
def test_lower_degree_destination_samples_the_source(dim, perturbed):
    cs, cd = PC.make_mesh(dim, 3, REPS[dim], perturbed), PC.make_mesh(dim, 2, REPS[dim], perturbed)
    state = _random_state(cs)
    S, D = _loaded(cs, state), PC.context(M, cd)
    D.transfer_state_from(S)
    err = max(_relmax(D.get(w), PE.interpolate(cs["mesh"], state[w], cd["mesh"])) for w in SIX)
    print("Q3 -> Q2 against the reference's interpolation: %.2e" % err)
    assert err < TOL
    S.close()
    D.close()


# ------------------------------------------------------------------ 5. failures and refusals
def test_destination_outside_the_source_is_refused_and_unchanged():
    cs = PC.make_mesh(3, 2, (3, 2, 3), False)
    cd = PC.make_mesh(3, 2, (3, 2, 3), False, lo=(0.05, 0.0, 0.0))  # the same cells, shifted by half a cell along x
    d_state = _random_state(cd, seed=13)
    S, D = _loaded(cs, _random_state(cs)), _loaded(cd, d_state)
    with pytest.raises(M.MiError) as err:
        D.transfer_state_from(S)
    assert err.value.code == M.MI_EINVAL and "outside" in str(err.value) and "node 6 " in str(err.value)  # (the last of the first x-row)
    for w in range(10):
        assert np.array_equal(D.get(w), d_state[w]), w
    S.transfer_state_from(S)  # onto itself: allowed, the identity up to rounding
    S.close()
    D.close()


def test_refusals():
    c3, c2 = PC.make_mesh(3, 2, (2, 2, 4), False), PC.make_mesh(2, 2, (3, 2), False)
    A, B, T = PC.context(M, c3), PC.context(M, c2), PC.context(M, c3, slabs=2)
    for dst, src, text in ((A, B, "2D"), (B, A, "3D"), (T, A, "one slab only"), (A, T, "one slab only")):
        with pytest.raises(M.MiError) as err:
            dst.transfer_state_from(src)
        assert err.value.code == M.MI_EINVAL and text in str(err.value)
    assert M.lib().mi_state_transfer(None, A.h) == M.MI_EINVAL and M.lib().mi_state_transfer(A.h, None) == M.MI_EINVAL
    for G in (A, B, T):
        G.close()
