"""GPU: the multigrid smoother's fine-level product against an independent reference of the same operator.

The smoother's product (mi_spmv under "spmv_as_smoother" 1, after assemble() with the point records of "element_tangents" 2
or "fine_level" 1) is compared with tests/golden/mirror.py's Operator: y = sum_e K_e(nq) x_e in numpy, constrained columns
masked, a constrained row multiplied by the assembled matrix's diagonal entry.  nq is the rule the library REPORTS
("smoother_quadrature_active": 3 = mf_spmv27 on the records of mf_records27, 4 = the 64-point product), and on a deformed state
the product must lie far from the other rule, so a report that does not match the kernel that ran fails.

Why a reference: the smoother only preconditions.  A wrong smoother product changes how many CG iterations a solve takes,
not what it converges to, so the oracle, golden and Newmark tests cannot see it.

Coverage: the four instances mf_spmv27 / mf_records27 <BOX, LAT>; geometry from per-cell 1/h (cubic and graded non-cubic
boxes) or from the trilinear map (distorted cells); node ids from the lattice ("cell_lattice" 1) or from conn (0).  Cell counts
1, 2, 3, 15, 17, 99: odd counts (the last wave's second half mirrors the last cell), fewer than 8 pairs, exactly 8 pairs and
8k + 1 pairs against "xcd_chunk".  Undeformed, sheared, random and folded states.  Clamped, z-clamped and interface faces.
Both fine levels.  Slabs cut along x, y and z with the layered launches ("mf_halo_overlap" 1) and without them.

Tolerances, relmax = max |y - y_ref| / max |y_ref|:
  fp64: 1e-12.  Observed worst (MI355X): 2.0e-14 for the 27-point rule (a 2-slab case), 1.8e-14 for the 64-point rule.
  fp32 ("smoother_precision" 32): 1e-5.  Each output is a sum over the 81 dofs of a cell, assembled over up to 8 cells,
  with records and arithmetic in fp32 (unit roundoff u = 6e-8).  The worst-case bound of such a sum is about
  81 u sum|K_ij x_j| = 4.8e-6 sum|K_ij x_j|.  sum|K_ij x_j| and max|y| are of the same size here, because the mass term
  dominates the diagonal.  Observed worst (MI355X): 1.5e-7.
"""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

CL, IF, ZC = O.FACE_CLAMPED, O.FACE_INTERFACE, O.FACE_ZCLAMP
ROLES_A = [CL, IF, IF, IF, ZC, IF]
ROLES_B = [CL, IF, IF, IF, ZC, ZC]
A1 = 1.0 / (0.25 * 0.005**2)  # alpha_1 of the default Newmark parameters
TOL = {64: 1e-12, 32: 1e-5}
APART = 1e-6  # the two rules on a deformed state: at least this far apart (the mirror tests show they are)


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _geometry(kind, reps, seed):
    """lo, hi, perturb of a cube / graded / distorted mesh of reps cells"""
    reps = np.array(reps)
    if kind == "cube":
        return (0.0, 0.0, 0.0), tuple(0.1 * reps), None
    h = np.array([0.13, 0.1, 0.07])  # hx != hy != hz
    hi = tuple(h * reps)
    rng = np.random.default_rng(seed)
    nv = reps + 1
    vid = np.stack(np.meshgrid(*[np.arange(n) for n in nv], indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)
    if kind == "graded":  # rectilinear: every vertex plane moved along its own axis, so the spacing varies plane by plane
        planes = [0.3 * h[d] * rng.uniform(-1, 1, nv[d]) for d in range(3)]
        return (0.0, 0.0, 0.0), hi, np.stack([planes[d][vid[:, d]] for d in range(3)], -1)
    assert kind == "distorted"
    return (0.0, 0.0, 0.0), hi, 0.08 * h.min() * rng.standard_normal((len(vid), 3))


def _shear(X):
    """a smooth large deformation with shear (F != F^T, J != 1) that vanishes on x = min x and has u_z = 0 on both z faces"""
    L = np.ptp(X, axis=0).max()
    s = (X - X.min(axis=0)) / L
    tz = np.ptp(s[:, 2])
    u = np.zeros_like(X)
    u[:, 0] = s[:, 0] * (0.3 * s[:, 1] + 0.2 * s[:, 2])
    u[:, 1] = s[:, 0] * (0.25 + 0.3 * s[:, 2] ** 2)
    u[:, 2] = s[:, 0] * s[:, 2] * (tz - s[:, 2]) * (0.6 * np.sin(3.0 * s[:, 1]) - 0.5)
    return L * u.reshape(-1)


def _states(m, reps, kind, rng):
    """(name, u, du, deformed): V_U and V_DELTA both non-zero, since the records read u + du"""
    free = ~m.constrained
    X = m.coords
    w = 1e-3 * rng.standard_normal(m.n) * free
    yield "undeformed", w, -w, False  # u + du = 0 exactly
    s = _shear(X) * free
    yield "shear", 0.6 * s, s - 0.6 * s, True
    h = 0.07
    yield "random", 0.02 * h * rng.standard_normal(m.n) * free, 0.01 * h * rng.standard_normal(m.n) * free, True
    if kind != "distorted":
        # u_x = -1.05 x M(eta), M = 4 eta (1 - eta) in every cell's own eta along y (Q2 holds it exactly: M = 1 on the mid
        # nodes, 0 on the vertices): det F = 1 - 1.05 M folds at the 27-point rule's eta = 0.5, not at the 64-point rule's
        jy = (np.arange(m.nnodes) // m.nn[0]) % m.nn[1]
        u = np.zeros((m.nnodes, 3))
        u[:, 0] = -1.05 * (X[:, 0] - X[:, 0].min()) * (jy % 2)  # (0 on the clamped face)
        u = u.reshape(-1) * free
        yield "folded", 0.5 * u, u - 0.5 * u, True


def _smoother_product(G, x):
    G.set_tuning("spmv_as_smoother", 1)
    try:
        return G.spmv(x)
    finally:
        G.set_tuning("spmv_as_smoother", 0)


def _compare(G, m, u, du, x, deformed, expect, bits=64):
    """set the state, assemble, and hold the smoother's product to the reference at the reported rule; worst relmax"""
    G.set(M.V_U, u)
    G.set(M.V_DELTA, du)
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    q = G.get_tuning("smoother_quadrature_active")
    assert q == expect
    y = _smoother_product(G, x)
    ut = u + du
    op4 = Mi.Operator(m, ut, alpha1=A1, nq=4)
    op3 = Mi.Operator(m, ut, alpha1=A1, nq=3, fold_to_identity=True, cdiag=op4.cdiag)
    ref = {3: op3(x), 4: op4(x)}
    err = _relmax(y, ref[q])
    assert err <= TOL[bits], (q, err)
    if deformed:
        assert _relmax(y, ref[7 - q]) > max(APART, 10 * TOL[bits])
    return err, op3.folded.any()


def _pair(kind, reps, roles, seed, **kw):
    lo, hi, perturb = _geometry(kind, reps, seed)
    G = M.Context(dim=3, degree=2, reps=reps, lo=lo, hi=hi, face_role=roles, perturb=perturb, **kw)
    m = Mi.Mesh(3, 2, reps, lo, hi, roles, perturb=perturb)
    assert np.array_equal(G.constrained, m.constrained) and np.abs(G.coords - m.coords).max() < 1e-14
    return G, m


def _setup(G, lattice, fine_level):
    if fine_level:
        G.set_tuning("fine_level", 1)
    else:
        G.set_tuning("element_tangents", 2)
    G.set_tuning("cell_lattice", lattice)
    assert G.get_tuning("cell_lattice") == lattice


# (geometry, reps, cell_lattice, fine_level, roles): with the geometries, both lattice settings reach all four instances
CASES = [
    ("cube", (1, 1, 1), 1, 0, ROLES_A),
    ("graded", (1, 1, 1), 0, 1, ROLES_B),
    ("distorted", (2, 1, 1), 1, 1, ROLES_A),
    ("cube", (2, 1, 1), 0, 0, ROLES_B),
    ("graded", (3, 1, 1), 1, 0, ROLES_A),
    ("distorted", (1, 1, 3), 0, 0, ROLES_B),
    ("graded", (3, 5, 1), 0, 1, ROLES_A),  # 15 cells: 8 pairs, the last one half mirrored
    ("distorted", (5, 3, 1), 1, 0, ROLES_B),
    ("cube", (1, 17, 1), 1, 1, ROLES_A),  # 17 cells: 9 pairs = 8 + 1
    ("distorted", (1, 1, 17), 0, 1, ROLES_A),
    ("graded", (3, 3, 11), 1, 1, ROLES_B),  # 99 cells
    ("distorted", (3, 11, 3), 0, 0, ROLES_A),
    ("cube", (3, 3, 11), 0, 1, ROLES_B),
]


@pytest.mark.parametrize("kind,reps,lattice,fine_level,roles", CASES)
def test_smoother_product_matches_the_reference(kind, reps, lattice, fine_level, roles):
    """the 27-point product (the default rule) on one slab: every state, to 1e-12 of the reference; the folded state against
    the reference's fold rule, with folded points present"""
    G, m = _pair(kind, reps, roles, seed=sum(reps))
    _setup(G, lattice, fine_level)
    rng = np.random.default_rng(len(m.cells))
    worst = 0.0
    for name, u, du, deformed in _states(m, reps, kind, rng):
        x = rng.standard_normal(m.n)
        err, folded = _compare(G, m, u, du, x, deformed, 3)
        assert folded == (name == "folded")
        worst = max(worst, err)
    print("smoother product %s %s lattice %d fine_level %d: worst relmax %.2e" % (kind, reps, lattice, fine_level, worst))
    G.close()


# (geometry, slabs, cut_axis, mf_halo_overlap, cell_lattice, fine_level)
SLAB_CASES = [
    ("cube", 2, 1, 1, 1, 0),
    ("graded", 3, 2, 0, 1, 1),
    ("distorted", 3, 3, 1, 1, 0),
    ("graded", 2, 3, 1, 0, 0),
    ("distorted", 2, 2, 0, 1, 1),
    ("cube", 3, 3, 1, 1, 1),
]


@pytest.mark.parametrize("kind,slabs,cut_axis,overlap,lattice,fine_level", SLAB_CASES)
def test_smoother_product_on_slabs_matches_the_undecomposed_reference(kind, slabs, cut_axis, overlap, lattice, fine_level):
    """emulated slabs: the gathered global product against the reference of the whole mesh.  With "mf_halo_overlap" 1 and
    lattice ids the product runs in launches over cell layers around the halo exchange (sel_n), as in the V-cycle."""
    reps = (6, 6, 6)
    G, m = _pair(kind, reps, ROLES_A, seed=7 * slabs + cut_axis, slabs=slabs, cut_axis=cut_axis)
    assert G.comm_info()[0] == slabs
    _setup(G, lattice, fine_level)
    G.set_tuning("mf_halo_overlap", overlap)
    rng = np.random.default_rng(slabs * 10 + cut_axis)
    worst = 0.0
    for name, u, du, deformed in _states(m, reps, kind, rng):
        if name == "undeformed":
            continue
        err, _ = _compare(G, m, u, du, rng.standard_normal(m.n), deformed, 3)
        worst = max(worst, err)
    print("smoother product on %d slabs, cut %d, overlap %d, %s: worst relmax %.2e" % (slabs, cut_axis, overlap, kind, worst))
    G.close()


# (tuning key, value, fine_level, precision of the product, rule the library must report)
RULE_CASES = [
    ("smoother_precision", 32, 0, 32, 4),
    ("smoother_precision", 32, 1, 32, 4),
    ("mf_single_launch", 0, 0, 64, 4),
    ("smoother_quadrature", 4, 0, 64, 4),
    ("smoother_quadrature", 4, 1, 64, 4),
]


@pytest.mark.parametrize("key,value,fine_level,bits,rule", RULE_CASES)
def test_reported_rule_is_the_rule_that_ran(key, value, fine_level, bits, rule):
    """the configurations under which the smoother keeps the 64-point kernel report 4, and their product IS the 64-point
    operator: to the reference at nq = 4 (fp32: 1e-5), far from nq = 3.  Graded boxes with lattice ids: the fp32 kernel exists
    for that shape only (elsewhere "smoother_precision" 32 multiplies in fp64)."""
    reps = (3, 2, 3)
    G, m = _pair("graded", reps, ROLES_B, seed=5)
    _setup(G, 1, fine_level)
    G.set_tuning(key, value)
    rng = np.random.default_rng(9)
    worst = 0.0
    for name, u, du, deformed in _states(m, reps, "graded", rng):
        err, _ = _compare(G, m, u, du, rng.standard_normal(m.n), deformed, rule, bits)
        worst = max(worst, err)
    if bits == 32:
        assert worst > 1e-9  # the fp32 arithmetic ran (an fp64 product agrees to 1e-14)
    print("smoother product under %s %d, fine_level %d: rule %d, worst relmax %.2e" % (key, value, fine_level, rule, worst))
    G.close()
