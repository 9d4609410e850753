"""GPU: the multigrid V-cycle and its parts against an independent numpy reference (tests/golden/mg_reference.py).

Why: the V-cycle only preconditions.  A restriction weight w swapped with 1 - w, a Chebyshev coefficient wrong from the third
step on, a coarse operator assembled at the wrong state, a prolongation that forgets a mask -- all of these still converge to
the right solution and change the iteration counts by a few.  Here the cycle z = M^-1 r (mi_spmv under "spmv_as_smoother" 2)
is compared with B_ref r, where B_ref is built in numpy from mirror.py's operators alone.  From the device the reference
takes one scalar per level, the smoother's lmax, and (a) bounds that scalar against the true eigenvalue in numpy.

Per case: create the context, set the shape keys, then "precond" 1, a sheared state with V_U and V_DELTA both non-zero,
update_acceleration, assemble, one cg_solve (which builds the coarse operators for this state), then
  (a) mi_mg_level_describe of every level equals the reference's derivation of the hierarchy, and
      lambda_true <= lmax <= 1.15 lambda_true (1 + 1e-10) on every smoothed level (lambda_true: D^-1 A of the MIRROR's level);
  (b) undecomposed cases, through the borrowed level contexts: state to 1e-14, matrix to 1e-12 of its largest entry, diagonal
      blocks to 1e-12, constraint flags equal;
  (c) relmax = max |z - z_ref| / max |z_ref| <= TOL for a random right-hand side, the solve's own and a unit vector at the
      node next to the clamped face and a mesh corner; two applications give the same bits.

TOL: 64 x the worst rounding of the reference itself (float64 against long double cycle, E_REF = 1.0e-15 over a measured
8.98e-16, tests/test_mirror_multigrid.py on these very cases), rounded up to the next power of ten: 1e-13; never above 1e-10.
64 is the margin for the device's different summation orders (sliced-ELL rows, slot gathers, the three-term form, blocked
Gauss-Jordan without pivoting).

Measured on an MI355X, worst relmax of (c) per group of cases:
  3D Q2, assembled fine level (cases 1, 7-10)          3.9e-15      unfused forms of case 1 (mg_fuse 0 / 2,
  matrix-free smoother / fine level (3, 4)             1.9e-15        mg_restrict_fuse 0)               2.6e-15 (same bits)
  3D Q3, both smoother rules (5)                       2.9e-15      slabs, shared and induced cuts (12, 13)  3.7e-15
  3D Q1 (6)                                            1.7e-15      lagged and rebuilt coarse operators (14) 1.9e-15
  2D Q2 and Q4 (11)                                    5.2e-15      after mg_coarsest 2 / mg_dense 0         2.8e-15
and of (b): states 2.3e-16, matrices and diagonal blocks 3.1e-15.  (a): lmax / lambda_true = 1.149930 .. 1.150000 on every
level of every case.  The upper bound holds because the Ritz value and the power value both lie below lambda_true, the
latter only as a norm in the inner product of D, in which D^-1 A is self-adjoint.  The bound found the Euclidean norm that
the power iteration used to take: on q2_543_mf_fine, level 1, lmax was 4.129772 against lambda_true 3.590850, ratio 1.150082
(|D^-1 A|_2 = 3.79 there; the same iteration in numpy gives the same 3.591106).

The state: the shear of test_gpu_smoother_operator.py at a quarter of its amplitude (at half, the tangent of the 8 x 8 x 8
cube is indefinite and no CG converges), plus noise; V_U also holds small values on the constrained dofs, without which a
transfer that forgets the constraint mask computes the same numbers (the mask of the prolongation itself is redundant
wherever constraints cover whole faces: a coarse correction is zero on them already).

Shown to fail (each change made in a scratch copy, numbers only, never committed; 21 tests, the first assertion that
fails in each): restriction weights w and 1 - w swapped in build_transfer -- (c) in 20, the first solve does not converge in
one; c2 = rho / delta in chebyshev -- (c) in all 21; no cmask_tgt in lattice_interp -- (a) upper bound in 15 (the coarse
operators of an unmasked state have other eigenvalues), (b) states in 5, (c) in one; level-1 state from V_U alone in
mg_update -- (b) states in 15, (c) in 5, (a) in one.

"precond_storage" 32 and "smoother_precision" 32 are held to their own references in tests/test_gpu_multigrid_fp32.py.  Out of
scope: the fourth-kind smoother (experiments build only).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mg_reference as R  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

TOL = min(1e-10, 10.0 ** math.ceil(math.log10(64 * R.E_REF)))
TRACTION = {3: (0.0, -1e3, 200.0), 2: (0.0, -1e3)}


def _relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """mesh, geometry and the state of a case (shared and left unchanged)"""
    m, lo, hi, perturb = R.case_mesh(name)
    u, du = R.case_state(m, seed=len(name))
    return m, lo, hi, perturb, u, du


@functools.lru_cache(maxsize=None)
def _reference(name, variant=""):
    """the numpy hierarchy of a case at its state; variant: "coarsest2" / "polynomial" = the shape after the key change of the
    hierarchy-rebuild test (same fine level)"""
    m, _, _, _, u, du = _inputs(name)
    if variant == "":
        return R.case_reference(name, u + du, m)
    kw = dict(coarsest2=dict(coarsest=2), polynomial=dict(dense=0))[variant]
    return R.case_reference(name, u + du, m, fine=_reference(name), **kw)


def _context(name, extra_keys=()):
    c = R.case(name)
    m, lo, hi, perturb, u, du = _inputs(name)
    G = M.Context(dim=c["dim"], degree=c["p"], reps=c["reps"], lo=lo, hi=hi, face_role=c["roles"], perturb=perturb,
                  slabs=c.get("slabs", 1), cut_axis=c.get("cut_axis", 0))
    assert np.array_equal(G.constrained, m.constrained) and np.abs(G.coords - m.coords).max() < 1e-14
    for k, v in list(c.get("keys", [])) + list(extra_keys):
        G.set_tuning(k, v)
    G.set_tuning("precond", 1)
    G.set_interface_traction(TRACTION[c["dim"]])
    return G


def _solve(G, u, du, tol=1e-8):
    G.set(M.V_U, u)
    G.set(M.V_DELTA, du)
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    G.set(M.V_NEWTON, np.zeros(G.n))  # (the CG starts from what this vector holds)
    rc, its, _ = G.cg_solve(tol, 400)
    assert rc == 0
    return its


def _minv(G, r):
    G.set_tuning("spmv_as_smoother", 2)
    try:
        return G.spmv(r)
    finally:
        G.set_tuning("spmv_as_smoother", 0)


def _check_rule(G, name):
    c = R.CASES[name]
    keys = dict(c.get("keys", []))
    if c["p"] == 3 and keys.get("fine_level"):
        assert G.get_tuning("smoother_quadrature_q3_active") == c["nq0"]
    elif c["p"] == 2 and c["dim"] == 3 and (keys.get("fine_level") or keys.get("element_tangents")):
        assert G.get_tuning("smoother_quadrature_active") == c["nq0"]
    else:
        assert c.get("nq0") is None


def _check_shape_and_estimates(G, ref, distributed=None, bounds="first", lambda_true=None, slack=None):
    """(a); returns lmax per level.  lambda_true: the eigenvalue of a level where it is not ref.lambda_true (the fp32-stored
    matrices of tests/test_gpu_multigrid_fp32.py); slack: {level: relative width} by which both bounds of a level whose
    products run in fp32 arithmetic are widened (same file; no other level, and none here).  bounds "first": both bounds, for first estimates (power value and Ritz value both lie
    below lambda_true, times the safety factor 1.15); "refresh": the lower bound alone -- a refresh continues the power
    iteration and keeps, as a factor, what the Krylov estimate added to the FIRST power value (estimate_lmax: "never given
    back"), so its product may pass 1.15 lambda_true by design; None: no bound (estimates of an older operator)"""
    nl = G.mg_n_levels()
    assert nl == len(ref.shape)
    lmax = []
    for l, sh in enumerate(ref.shape):
        d = G.mg_level_describe(l)
        print("level %d: %s" % (l, d))
        assert (d["degree"], d["reps"], d["n_dofs"]) == (sh["degree"], sh["reps"], sh["n_dofs"])
        assert (d["exact_solve"], d["smoother_degree"], d["interval_ratio"]) == (sh["exact"], sh["nu"], sh["ratio"])
        assert d["distributed"] == (distributed[l] if distributed else 0)
        if sh["exact"]:
            assert d["lmax"] == 0.0
        elif bounds:
            lam = (lambda_true or ref.lambda_true)(l)
            w = (slack or {}).get(l, 0.0)
            print("level %d: lmax / lambda_true = %.6f" % (l, d["lmax"] / lam))
            assert lam * (1 - w) <= d["lmax"], (l, lam, d["lmax"])
            assert bounds == "refresh" or d["lmax"] <= 1.15 * lam * (1 + 1e-10) * (1 + w), (l, lam, d["lmax"])
        lmax.append(d["lmax"])
    return lmax


def _check_parts(G, ref, levels=None, matrix0=True):
    """(b)"""
    for l in (range(len(ref.shape)) if levels is None else levels):
        V = G.mg_level_context(l)
        assert V.n == ref.shape[l]["n_dofs"]
        assert np.array_equal(V.constrained, ref.meshes[l].constrained)
        if l > 0:
            e = _relmax(V.total_displacement(), ref.states[l])
            print("level %d state relmax %.2e" % (l, e))
            assert e <= 1e-14
        D = V.diagonal_blocks()
        e = _relmax(D, ref.D[l])
        print("level %d diagonal blocks relmax %.2e" % (l, e))
        assert e <= 1e-12
        if l > 0 or matrix0:
            A, A_ref = V.csr(), (ref.A_assembled if l == 0 else ref.A[l])
            e = float(abs(A - A_ref).max() / abs(A_ref).max())
            print("level %d matrix relmax %.2e" % (l, e))
            assert e <= 1e-12
        V.close()


def _rhs_set(G, m, seed):
    free = ~m.constrained
    rng = np.random.default_rng(seed)
    node = 1
    for d in range(1, m.dim):  # lattice index (1, 1, 1): next to the clamped face x = lo and to the corner at lo
        node += int(np.prod(m.nn[:d]))
    e = np.zeros(m.n)
    e[node * m.dim] = 1.0
    assert free[node * m.dim]
    return [("random", rng.standard_normal(m.n) * free), ("rhs", G.get(M.V_RHS) * free), ("unit", e)]


def _check_cycle(G, m, ref, lmax, tag, seed=0):
    """(c); returns the worst relmax (every figure is asserted on its own: a NaN fails)"""
    worst = 0.0
    for what, r in _rhs_set(G, m, seed):
        z = _minv(G, r)
        z_ref = ref.vcycle(r, lmax)
        e = _relmax(z, z_ref)
        print("V-cycle %s, %s: relmax %.2e (tolerance %.0e)" % (tag, what, e, TOL))
        assert np.all(np.isfinite(z)) and e <= TOL, (tag, what, e)
        worst = max(worst, e)
        assert np.array_equal(_minv(G, r), z)  # a fixed linear operator between operator updates
    return worst


SINGLE = [n for n, c in R.CASES.items() if c.get("slabs", 1) == 1]
TEAMS = {"q2_4412_3slabs_z": [1, 1, 0, 0], "q2_1244_2slabs_x": [1, 1, 0, 0], "q2_4416_induced": [1, 1, 1, 0]}


@pytest.mark.parametrize("name", SINGLE)
def test_vcycle_and_its_parts_match_the_reference(name):
    """cases 1 and 3-11 of the table in mg_reference.CASES: (a) with both bounds on the first estimates, (b) and (c) on one slab"""
    m, _, _, _, u, du = _inputs(name)
    G = _context(name)
    _solve(G, u, du)
    _check_rule(G, name)
    ref = _reference(name)
    lmax = _check_shape_and_estimates(G, ref)
    _check_parts(G, ref, matrix0=not dict(R.CASES[name].get("keys", [])).get("fine_level"))
    _check_cycle(G, m, ref, lmax, name)
    G.close()


@pytest.mark.parametrize("key,value", [("mg_fuse", 0), ("mg_fuse", 2), ("mg_restrict_fuse", 0)])
def test_unfused_forms_match_the_reference(key, value):
    """case 2, the whole protocol under each key: cheb_step_blk3 / cheb_step_blk, lattice_restrict_unrolled, vec_residual and the epilogues on every level against
    the reference itself, not merely against the fused bits"""
    name = "q2_654"
    m, _, _, _, u, du = _inputs(name)
    G = _context(name)
    G.set_tuning(key, value)
    _solve(G, u, du)
    ref = _reference(name)
    lmax = _check_shape_and_estimates(G, ref)
    _check_parts(G, ref)
    _check_cycle(G, m, ref, lmax, "%s %s %d" % (name, key, value))
    G.close()


@pytest.mark.parametrize("name", sorted(TEAMS))
def test_vcycle_on_slabs_matches_the_undecomposed_reference(name):
    """cases 12 and 13: (a) and (c).  The reference is numpy throughout and knows nothing of slabs; only lmax comes from the
    team.  Shared Q1 slab level, ownership-masked restriction plus all-reduce, halo-skip; with "mg_dist_nodes" 0 the induced
    cuts of the first coarsened level."""
    m, _, _, _, u, du = _inputs(name)
    G = _context(name)
    assert G.comm_info()[0] == R.CASES[name]["slabs"] and G.get_tuning("cut_axis") == R.CASES[name]["cut_axis"]
    _solve(G, u, du)
    assert G.get_tuning("mg_distributed_levels") == sum(TEAMS[name])
    with pytest.raises(M.MiError):
        G.mg_level_context(1)
    ref = _reference(name)
    lmax = _check_shape_and_estimates(G, ref, distributed=TEAMS[name])
    _check_cycle(G, m, ref, lmax, name)
    G.close()


def test_lagged_coarse_operators_are_those_of_the_older_state():
    """case 14, on case 3: a second assemble + cg_solve at a changed state in the same time step.  Under "mg_lag" 1 the coarse
    operators stay: the view reports the interpolation of the OLD state, and the cycle is the reference with level 0 at the new
    state and the levels below at the old one.  With "mg_lag" 0 the third solve rebuilds them at the new state."""
    name = "q2_753_mf27"
    m, _, _, _, u, du = _inputs(name)
    G = _context(name)
    _solve(G, u, du)
    n0 = G.get_tuning("count_mg_refresh")
    du2 = 0.55 * du + 1e-5 * np.random.default_rng(2).standard_normal(m.n) * ~m.constrained
    _solve(G, u, du2)
    assert G.get_tuning("count_mg_refresh") == n0  # lagged
    lagged = R.case_reference(name, u + du2, m, coarse_from=u + du)
    lmax = _check_shape_and_estimates(G, lagged, bounds=None)  # (estimates of the older operators: no bound)
    _check_parts(G, lagged, levels=range(1, len(lagged.shape)))
    assert _relmax(G.mg_level_context(0).diagonal_blocks(), lagged.D[0]) <= 1e-12
    _check_cycle(G, m, lagged, lmax, name + " lagged")
    G.set_tuning("mg_lag", 0)
    _solve(G, u, du2)
    assert G.get_tuning("count_mg_refresh") == n0 + 1
    fresh = R.case_reference(name, u + du2, m, fine=lagged)
    lmax = _check_shape_and_estimates(G, fresh, bounds="refresh")
    _check_parts(G, fresh)
    _check_cycle(G, m, fresh, lmax, name + " mg_lag 0")
    assert _relmax(fresh.states[1], lagged.states[1]) > 1e-3  # the two states are far apart: the view told them apart
    G.close()


@pytest.mark.parametrize("key,value,variant", [("mg_coarsest", 2, "coarsest2"), ("mg_dense", 0, "polynomial")])
def test_hierarchy_rebuilt_between_two_solves_gets_its_operators(key, value, variant):
    """A shape key on a context that has a hierarchy rebuilds it; the new levels have no operators, so the next solve must
    build them whatever "mg_lag" and the refresh interval say (it used to skip the update and apply levels with lmax = 0 and an
    unfilled dense inverse: NaN, MI_ENOCONV_LIN).  The second solve of the time step converges in the iterations of a context
    that had the key from the start; afterwards (a), with both bounds -- the new hierarchy's estimates are first estimates --,
    and (c) hold for the new shape."""
    name = "q2_654"
    m, _, _, _, u, du = _inputs(name)
    F = _context(name, extra_keys=[(key, value)])
    its_fresh = _solve(F, u, du)
    F.close()
    G = _context(name)
    _solve(G, u, du)
    n0 = G.get_tuning("count_mg_refresh")
    G.set_tuning(key, value)
    with pytest.raises(M.MiError):  # the view does not describe operators that were never built
        G.mg_level_describe(0)
    G.set(M.V_NEWTON, np.zeros(G.n))
    rc, its, _ = G.cg_solve(1e-8, 400)
    assert rc == 0 and G.get_tuning("count_mg_refresh") == n0 + 1
    assert abs(its - its_fresh) <= 2, (its, its_fresh)
    ref = _reference(name, variant)
    assert len(ref.shape) != len(_reference(name).shape) or ref.shape[-1]["exact"] != _reference(name).shape[-1]["exact"]
    lmax = _check_shape_and_estimates(G, ref)
    _check_cycle(G, m, ref, lmax, "%s after %s %d" % (name, key, value))
    G.close()
