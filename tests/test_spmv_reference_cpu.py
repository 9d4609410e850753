"""CPU: the long double product and the a-priori bound of tests/golden/spmv_reference.py, before any GPU test trusts them.

  * on random block matrices (2 x 2 and 3 x 3 blocks, rows of 1 to 40 blocks, empty rows among them, values over six decades)
    scipy's float64 product lies within the bound of the long double product, row by row, and is exactly zero on empty rows;
  * so does a float64 product summed in reversed order and one summed pairwise (the orders furthest from left to right);
  * the bound is not loose: one entry perturbed by 8 u relative makes its row violate it.  The row has n = 5 (two 2 x 2
    blocks), gamma_5 = 5 u, and x is a unit vector at the entry's column -- one of the inputs of the GPU test -- so that
    (|A| |x|)_i is the entry itself.  (Under white noise an entry must dominate its row to show: the bound is that of a sum.)
  * the fp32 reference is the product of the rounded values.

Measured: worst |y - y_ref|_i / bound_i of scipy's product 0.22, reversed 0.25, pairwise 0.25 (the short rows decide);
the perturbed entry 1.48 - 1.56.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import spmv_reference as S  # noqa: E402


def _block_matrix(D, nodes, seed):
    """random block rows of 1 .. 40 blocks of D x D (every 7th node row empty), values over six decades, both signs"""
    rng = np.random.default_rng(seed)
    indptr, indices = [0], []
    for i in range(nodes):
        k = 0 if i % 7 == 3 else int(rng.integers(1, min(40, nodes) + 1))
        indices.extend(np.sort(rng.choice(nodes, k, replace=False)))
        indptr.append(len(indices))
    data = rng.standard_normal((len(indices), D, D)) * 10.0 ** rng.uniform(-3, 3, (len(indices), 1, 1))
    A = sp.bsr_matrix((data, np.array(indices), np.array(indptr)), shape=(nodes * D, nodes * D)).tocsr()
    A.sort_indices()
    return A


def _row_sum(terms, order):
    if order == "reversed":
        s = 0.0
        for t in terms[::-1]:
            s += t
        return s
    t = list(terms)
    while len(t) > 1:  # pairwise
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0] if t else 0.0


def _product_in_order(A, x, order):
    y = np.zeros(A.shape[0])
    for i in range(A.shape[0]):
        a, b = A.indptr[i], A.indptr[i + 1]
        y[i] = _row_sum(A.data[a:b] * x[A.indices[a:b]], order)
    return y


@pytest.mark.parametrize("D,nodes,seed", [(2, 90, 1), (3, 70, 2), (3, 50, 3)])
def test_float64_products_in_any_order_stay_within_the_bound(D, nodes, seed):
    assert np.finfo(np.longdouble).eps < 1e-18
    A = _block_matrix(D, nodes, seed)
    x = np.random.default_rng(seed + 10).standard_normal(A.shape[0]) * 10.0 ** np.random.default_rng(seed).uniform(-2, 2, A.shape[0])
    empty = np.diff(A.indptr) == 0
    assert empty.any() and np.all(S.bound(A, x)[empty] == 0) and np.all(S.product(A, x)[empty] == 0)
    for what, y in [("scipy", A @ x), ("reversed", _product_in_order(A, x, "reversed")),
                    ("pairwise", _product_in_order(A, x, "pairwise"))]:
        ratio, zeros = S.worst_ratio(y, A, x)
        print("%s: worst |y - y_ref| / bound %.2f" % (what, ratio))
        assert zeros and ratio <= 1.0, (what, ratio)
    # the reference agrees with exact rational arithmetic where that is cheap: integers
    Ai = A.copy()
    Ai.data = np.round(10 * np.random.default_rng(4).standard_normal(len(A.data)))
    xi = np.round(10 * np.random.default_rng(5).standard_normal(A.shape[0]))
    assert np.array_equal(S.product(Ai, xi), (Ai @ xi).astype(np.longdouble))


def test_one_entry_perturbed_by_8u_violates_the_bound():
    """rows of two 2 x 2 blocks: n = 5"""
    nodes, D = 40, 2
    rng = np.random.default_rng(6)
    indices = np.stack([np.arange(nodes), (np.arange(nodes) + 1) % nodes], -1)
    indices.sort(axis=1)
    data = rng.uniform(1.0, 2.0, (nodes * 2, D, D)) * rng.choice([-1.0, 1.0], (nodes * 2, D, D))
    A = sp.bsr_matrix((data, indices.reshape(-1), np.arange(0, 2 * nodes + 1, 2)), shape=(nodes * D, nodes * D)).tocsr()
    A.sort_indices()
    assert np.all(np.diff(A.indptr) == 4)
    for row, k in [(0, 0), (17, 3), (79, 2)]:
        e = A.indptr[row] + k
        x = np.zeros(A.shape[0])
        x[A.indices[e]] = 1.0
        assert S.worst_ratio(A @ x, A, x) == (0.0, True)  # one term per row: exact
        B = A.copy()
        B.data[e] *= 1 + 8 * S.U
        y = B @ x
        err = np.abs(y.astype(np.longdouble) - S.product(A, x))
        bnd = S.bound(A, x)
        print("row %d: perturbed entry, error / bound %.2f" % (row, float(err[row] / bnd[row])))
        assert err[row] > bnd[row] > 0
        assert np.all(np.delete(err, row) == 0)


def test_f32_reference_is_the_product_of_the_rounded_values():
    A = _block_matrix(3, 30, 8)
    x = np.random.default_rng(9).standard_normal(A.shape[0])
    A32 = A.copy()
    A32.data = A.data.astype(np.float32).astype(np.float64)
    assert np.array_equal(S.product(A, x, f32=True), S.product(A32, x))
    assert np.array_equal(S.bound(A, x, f32=True), S.bound(A32, x))
    # ... which the fp64 bound of the unrounded matrix does not cover: the two references are told apart
    ratio, _ = S.worst_ratio(A32 @ x, A, x)
    assert ratio > 1e3
    ratio, zeros = S.worst_ratio(A32 @ x, A, x, f32=True)
    assert zeros and ratio <= 1.0
