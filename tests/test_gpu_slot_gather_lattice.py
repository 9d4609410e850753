"""GPU: the slot gathers with slot positions by arithmetic ("mf_gather_lattice" 1) and in node tiles (2) against the slot tables (0).

On lattice meshes with cell-major slots the four gathers (mf_gather, the residual gather, mf_gather_cheb3,
mf_gather_dot) find a node's contributions from its coordinates instead of through slot_base / slot_src, and the two
Chebyshev gathers walk 2 x 2 node lines per workgroup.  Neither changes which values are added nor in which order, so every
result must have the BITS of the table form: numpy.array_equal throughout, no tolerance.  (That the table form itself is the
operator is the business of test_gpu_smoother_operator.py and test_gpu_parity.py, which run under the default mode.)

Per shape and fine level, modes 1 and 2 against mode 0, each mode in a context of its own:
  1. the smoother-form product of a random x (mf_spmv27 + mf_gather);
  2. the CG-form product of the same x (mf_spmv + mf_gather; on "fine_level" 1 this is the CG's operator);
  3. one Newmark step under the multigrid preconditioner from a random small state: the smoother runs mf_gather_cheb3 and
     the residual gather, the CG of "fine_level" 1 runs mf_gather_dot (its p.q decides every step length, so equal
     iterates mean equal partial sums).  Displacement, velocity, acceleration, Newton and CG iteration counts.
"mf_gather_lattice_active" must report the mode that was set.

Shapes, the smallest at which the arithmetic can go wrong: one cell (seven parity triples empty); one shared face per
direction (swapped strides); the first node with eight cells; odd counts and colours of different size; (5,4,3) with partial
tiles at the end of every direction; (65,2,1) = 131 nodes along x, two x segments of the 128-node tile; graded boxes; two
slabs along each axis and three along z (ghost nodes, owned ranges, the lattice laid along another axis).

Where the arithmetic does not apply -- node ids from the connectivity ("cell_lattice" 0, here on a distorted mesh),
node-major slots ("smoother_quadrature" 4) -- the request is accepted, 0 is reported and the results are those of mode 0.
"""
import numpy as np
import pytest

from test_gpu_smoother_operator import M, ROLES_A, _pair, _setup, _smoother_product

pytestmark = pytest.mark.gpu

# (geometry, reps, slabs, cut_axis)
SHAPES = [
    ("cube", (1, 1, 1), 1, 0),
    ("cube", (2, 1, 1), 1, 0),
    ("cube", (1, 2, 1), 1, 0),
    ("cube", (1, 1, 2), 1, 0),
    ("cube", (2, 2, 2), 1, 0),
    ("cube", (3, 2, 2), 1, 0),
    ("cube", (5, 4, 3), 1, 0),
    ("cube", (65, 2, 1), 1, 0),
    ("graded", (3, 1, 1), 1, 0),
    ("graded", (4, 3, 3), 2, 1),
    ("cube", (3, 4, 3), 2, 2),
    ("graded", (3, 3, 4), 2, 3),
    ("cube", (2, 2, 6), 3, 3),
]
CASES = [s + (fl,) for s in SHAPES for fl in (0, 1)]


def _run(kind, reps, slabs, cut_axis, fine_level, mode, lattice=1, extra=()):
    """what one mode computes: the reported mode, the two products, the state after one Newmark step and its counts"""
    kw = dict(slabs=slabs, cut_axis=cut_axis) if slabs > 1 else {}
    G, m = _pair(kind, reps, ROLES_A, seed=sum(reps), **kw)
    G.set_tuning("precond", 1)
    _setup(G, lattice, fine_level)
    for key, value in extra:
        G.set_tuning(key, value)
    G.set_tuning("mf_gather_lattice", mode)
    rng = np.random.default_rng(1000 + len(m.cells))
    free = ~m.constrained
    h = 0.07
    G.set(M.V_U, 0.005 * h * rng.standard_normal(m.n) * free)
    G.set(M.V_V_OLD, 0.01 * rng.standard_normal(m.n) * free)
    G.set_interface_traction((0.0, -2e3, 500.0))
    G.update_acceleration()
    assert np.isfinite(G.assemble())
    active = G.get_tuning("mf_gather_lattice_active")
    x = rng.standard_normal(m.n)
    out = {"smoother product": _smoother_product(G, x), "cg product": G.spmv(x)}
    rc, info = G.newmark_step(tol_lin=1e-8)
    assert rc == 0 and info.converged == 1
    assert G.get_tuning("mf_gather_lattice_active") == active
    out["u"], out["v"], out["a"] = G.get(M.V_U), G.get(M.V_V), G.get(M.V_A)
    out["counts"] = np.array([info.newton_iterations, info.assemblies, info.lin_its_total])
    G.close()
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return active, out


def _assert_same(out, ref, what):
    for k in ref:
        assert np.array_equal(out[k], ref[k]), (what, k, np.abs(out[k] - ref[k]).max())


@pytest.mark.parametrize("kind,reps,slabs,cut_axis,fine_level", CASES)
def test_lattice_gathers_have_the_bits_of_the_table_gathers(kind, reps, slabs, cut_axis, fine_level):
    active, ref = _run(kind, reps, slabs, cut_axis, fine_level, 0)
    assert active == 0
    assert ref["counts"][2] > 0  # the linear solves iterated: the Chebyshev gathers ran
    for mode in (1, 2):
        active, out = _run(kind, reps, slabs, cut_axis, fine_level, mode)
        assert active == mode
        _assert_same(out, ref, "mode %d" % mode)


@pytest.mark.parametrize("fine_level", [0, 1])
def test_the_default_is_a_lattice_form(fine_level):
    active, _ = _run("cube", (3, 2, 2), 1, 0, fine_level, -1)
    assert active in (1, 2)


# (geometry, reps, cell_lattice, further keys): where the arithmetic or the tiles do not apply
FALLBACKS = [
    ("distorted", (2, 1, 1), 0, ()),
    ("cube", (3, 2, 2), 0, ()),
    ("graded", (3, 2, 2), 1, (("smoother_quadrature", 4),)),  # node-major slots
]


@pytest.mark.parametrize("kind,reps,lattice,extra", FALLBACKS)
@pytest.mark.parametrize("fine_level", [0, 1])
def test_where_the_lattice_form_does_not_apply_the_tables_run(kind, reps, lattice, extra, fine_level):
    active, ref = _run(kind, reps, 1, 0, fine_level, 0, lattice, extra)
    assert active == 0
    for mode in (1, 2):
        active, out = _run(kind, reps, 1, 0, fine_level, mode, lattice, extra)
        assert active == 0  # (never 2 where the tiles do not apply)
        _assert_same(out, ref, "mode %d" % mode)
