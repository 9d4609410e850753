"""GPU: what the 27-point smoother product reads of its operand and of the cell geometry, at the smallest shapes that show it.

mf_spmv27 gathers x for every node of a cell and masks the constrained entries, and on box meshes takes 1/hx, 1/hy, 1/hz and
the volume per cell, two cells to a wave.  Three properties, on the helpers of test_gpu_smoother_operator.py (the smoother's
form of mi_spmv after assemble() with point records), for both fine levels:

1. A constrained entry of x never reaches a free row.  The mask is a selection, not a factor: with NaN in every constrained
   entry the free rows hold the same bits as with 0 there.  (mi_spmv passes non-finite operands through unchanged, so NaN it
   is.)  Constrained rows are diag * x by design and are left out.
2. The same product twice gives the same bits.
3. Each half of a wave takes the geometry of ITS cell: on the graded (3,1,1) mesh, where the two cells of the first wave differ
   in hx, the product agrees with mirror.Operator(nq=3) to 1e-12 and lies more than 1e-6 from the reference of the mesh with
   the sizes of cells 0 and 1 exchanged.  That the two references are that far apart is asserted first (no GPU involved).

Shapes: graded (3,1,1) with lattice ids -- boxes, an odd cell count, so the second half of the last wave mirrors the last cell;
distorted (2,1,1) with ids from the connectivity -- the trilinear geometry; cube (1,1,1) -- a single half-wave.
"""
import numpy as np
import pytest

from test_gpu_smoother_operator import A1, M, Mi, ROLES_A, _geometry, _pair, _relmax, _setup, _smoother_product

pytestmark = pytest.mark.gpu

TOL = 1e-12  # as test_gpu_smoother_operator.py (fp64)
APART = 1e-6

# (geometry, reps, cell_lattice)
SHAPES = [
    ("graded", (3, 1, 1), 1),
    ("distorted", (2, 1, 1), 0),
    ("cube", (1, 1, 1), 1),
]
CASES = [s + (fl,) for s in SHAPES for fl in (0, 1)]


def _seed(reps):
    return sum(reps)


def _assembled(kind, reps, lattice, fine_level):
    """context and mirror mesh at a random deformed state, assembled, the 27-point rule active; u + du"""
    G, m = _pair(kind, reps, ROLES_A, seed=_seed(reps))
    _setup(G, lattice, fine_level)
    rng = np.random.default_rng(100 + len(m.cells))
    free = ~m.constrained
    h = 0.07
    u = 0.02 * h * rng.standard_normal(m.n) * free
    du = 0.01 * h * rng.standard_normal(m.n) * free
    G.set(M.V_U, u)
    G.set(M.V_DELTA, du)
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    assert G.get_tuning("smoother_quadrature_active") == 3
    return G, m, u + du, rng


def _swapped_graded(reps, seed):
    """perturb of the graded mesh with the x-sizes of cells 0 and 1 exchanged: the vertex plane between them moves"""
    lo, hi, perturb = _geometry("graded", reps, seed)
    hx = hi[0] / reps[0]
    nvx = reps[0] + 1
    plane = [i * hx + perturb[i, 0] for i in range(nvx)]  # (vertices are x fastest: the first nvx are the x planes)
    new1 = plane[0] + (plane[2] - plane[1])
    swapped = perturb.copy()
    swapped[1::nvx, 0] = new1 - hx
    return lo, hi, swapped


@pytest.mark.parametrize("kind,reps,lattice,fine_level", CASES)
def test_constrained_operand_entries_never_reach_free_rows(kind, reps, lattice, fine_level):
    G, m, _, rng = _assembled(kind, reps, lattice, fine_level)
    c = m.constrained
    assert c.any() and (~c).any()
    x0 = rng.standard_normal(m.n) * ~c
    x1 = np.where(c, np.nan, x0)
    y0 = _smoother_product(G, x0)
    y1 = _smoother_product(G, x1)
    assert np.isfinite(y0).all()
    assert np.array_equal(y1[~c], y0[~c])  # bitwise (all finite, so no NaN != NaN in the comparison)
    G.close()


@pytest.mark.parametrize("kind,reps,lattice,fine_level", CASES)
def test_product_is_repeatable(kind, reps, lattice, fine_level):
    G, m, _, rng = _assembled(kind, reps, lattice, fine_level)
    x = rng.standard_normal(m.n)
    ya = _smoother_product(G, x)
    yb = _smoother_product(G, x)
    assert np.isfinite(ya).all() and np.array_equal(ya, yb)
    G.close()


@pytest.mark.parametrize("fine_level", [0, 1])
def test_each_half_wave_takes_the_geometry_of_its_cell(fine_level):
    kind, reps, lattice = SHAPES[0]
    G, m, ut, rng = _assembled(kind, reps, lattice, fine_level)
    x = rng.standard_normal(m.n)
    lo, hi, swapped = _swapped_graded(reps, _seed(reps))
    ms = Mi.Mesh(3, 2, reps, lo, hi, ROLES_A, perturb=swapped)
    assert np.array_equal(ms.constrained, m.constrained)
    w = [np.ptp(np.array(mesh.cells[e][1])[:, 0]) for mesh in (m, ms) for e in (0, 1)]
    assert abs(w[0] - w[3]) < 1e-15 and abs(w[1] - w[2]) < 1e-15 and abs(w[0] - w[1]) > 1e-3  # exchanged, and different
    op4 = Mi.Operator(m, ut, alpha1=A1, nq=4)
    ref = Mi.Operator(m, ut, alpha1=A1, nq=3, fold_to_identity=True, cdiag=op4.cdiag)(x)
    ref_swapped = Mi.Operator(ms, ut, alpha1=A1, nq=3, fold_to_identity=True, cdiag=op4.cdiag)(x)
    apart = _relmax(ref_swapped, ref)
    assert apart > 10 * APART, apart  # the two references themselves (the free rows: cdiag is shared)
    y = _smoother_product(G, x)
    err, far = _relmax(y, ref), _relmax(y, ref_swapped)
    print("graded %s fine_level %d: relmax to the reference %.2e, to the swapped mesh %.2e (references %.2e apart)" %
          (reps, fine_level, err, far, apart))
    assert err <= TOL, err
    assert far > APART, far
    G.close()
