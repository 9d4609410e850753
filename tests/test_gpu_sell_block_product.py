"""GPU: sell_spmm, the block product on the assembled tangent (mi_spmm / Context.spmm; the stiffness images of
mi_tangent_modes), on the meshes of tests/test_gpu_sell_lds_product.py: q2_11 (11^3 Q2 cells, 12,167 nodes, 190 slices, the
smallest above the 160-slice threshold; WXT 3 / 5, a chunk staged whole) and q3_7 (the generic x-widths, chunks in two halves),
with that file's roles, perturbation and state.

sell_spmm is sell_slice on NV = 3 columns per launch (mi::SELL_SPMM_NV, profiles/tangent_modes/resources.tsv): per row and column
the same operations in the same order, so the claims are exact.
  * spmm(X)[:, j] == spmv(X[:, j]) bit for bit for 1 .. 2 NV + 1 columns: every group size and every remainder
  * the vectors: noise, a smooth field, unit columns, the constrained dofs alone
  * every row within the a-priori bound of the long double product (tests/golden/spmv_reference.py, no margin)
  * the result block is pre-filled with another product: a row nobody computes keeps a wrong value
  * the same bits on a second call
  * "spmm_launches" counts the block launches (ceil(nv / NV) per call); "spmv_lds_launches" / "spmv_split_launches" stay put
  * ineligible contexts (3 x 1 x 1 cells: a split launch; a 2D mesh; "fine_level" 1) return the per-column results with
    "spmm_launches" 0
  * mi_tangent_modes on q2_11 with "modes_block_product" 1 and 0: identical lambda bits, "spmm_launches" > 0 only at 1
"""
import functools
import os
import sys

import numpy as np
import pytest

import test_gpu_sell_lds_product as TL
from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import spmv_reference as S  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

NV = 3  # mi::SELL_SPMM_NV


@functools.lru_cache(maxsize=None)
def _built(name):
    _, G = TL._make(name)
    return G, G.csr()


def _columns(G, nv):
    """[n, nv]: noise, a smooth field, a unit column, the constrained dofs alone, then noise again"""
    named = TL._inputs(G)
    rng = np.random.default_rng(nv)
    cols = [named[j][1] if j < len(named) else rng.standard_normal(G.n) for j in range(nv)]
    return np.stack(cols, axis=1)


def _spmm(G, X):
    """G.spmm(X) into a block that holds another product"""
    other = np.stack([G.spmv(-3.0 * X[::-1, j]) for j in range(X.shape[1])], axis=1)
    return G.spmm(X, out=other)


@pytest.mark.parametrize("name", ["q2_11", "q3_7"])
def test_block_product_equals_the_single_products_bit_for_bit(name):
    G, A = _built(name)
    TL._assert_lds(G, name)
    for nv in range(1, 2 * NV + 2):
        X = _columns(G, nv)
        before = G.get_tuning("spmm_launches")
        Y = _spmm(G, X)
        assert G.get_tuning("spmm_launches") - before == -(-nv // NV), nv
        for j in range(nv):
            assert np.array_equal(Y[:, j], G.spmv(X[:, j])), (name, nv, j)
        assert np.array_equal(G.spmm(X, out=np.full_like(X, 7.0)), Y)  # the same bits again, over another fill
        TL._assert_lds(G, name)
    # every row of the widest block within the bound of the long double product
    worst = 0.0
    for j in range(X.shape[1]):
        ratio, zeros = S.worst_ratio(Y[:, j], A, X[:, j], False)
        worst = max(worst, ratio)
        assert np.all(np.isfinite(Y[:, j])) and zeros and ratio <= 1.0, (name, j, ratio, zeros)
    free = ~G.constrained
    assert np.all(Y[free, 3] == 0.0)  # the constrained dofs alone: the free rows are exactly zero
    print("%s: worst |y - y_ref| / bound %.3f over %d columns" % (name, worst, X.shape[1]))


@pytest.mark.parametrize("what", ["split", "2d", "fine_level"])
def test_ineligible_contexts_go_column_by_column(what):
    if what == "2d":
        G = TL._make("2d_q1")[1]
    else:
        G = M.Context(dim=3, degree=2, reps=(3, 1, 1), hi=(1.5, 0.3, 0.3), face_role=[M.FACE_CLAMPED] + [M.FACE_INTERFACE] * 5)
        if what == "fine_level":
            G.set_tuning("fine_level", 1)
        G.assemble()
    X = np.random.default_rng(5).standard_normal((G.n, 2 * NV + 1))
    Y = G.spmm(X, out=np.full_like(X, 7.0))
    assert G.get_tuning("spmm_launches") == 0
    for j in range(X.shape[1]):
        assert np.array_equal(Y[:, j], G.spmv(X[:, j])), (what, j)
    G.close()


def test_tangent_modes_take_the_block_product_and_keep_their_bits():
    G = TL._make("q2_11")[1]
    G.set(M.V_DELTA, np.zeros(G.n))
    G.set_tuning("precond", 0)
    out = {}
    for key in (1, 0):
        G.set_tuning("modes_block_product", key)
        before = G.get_tuning("spmm_launches")
        try:
            res = G.tangent_modes(2, tol=1e-8, max_it=6, want_modes=False)
        except M.MiError as e:  # (six iterations: the comparison is of bits, not of convergence)
            assert e.code == M.MI_ENOCONV_LIN
            res = e.partial
        out[key] = (res["lam"], res["residual"], G.get_tuning("spmm_launches") - before)
    assert np.all(np.isfinite(out[1][0])) and np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    assert out[1][2] > 0 and out[0][2] == 0
    G.close()
