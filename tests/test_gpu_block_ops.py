"""GPU: the block-vector kernels of mi_linear_modes (block_gram, block_combine through the hooks mi_block_gram,
mi_block_combine) against long double numpy.

Bound: the a-priori one of ANY summation order, with or without FMA, no margin (the idiom of golden/spmv_reference.py; Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5)):
    |C_ij - ref| <= gamma_n  sum_r |a_ri| |b_rj|        gamma_k = k u / (1 - k u), u = 2^-53
    |Y_rj - ref| <= gamma_ks sum_k |s_rk| |c_kj|
Entries whose bound is zero must be exact zeros.

Rows: 1, one wave of 64 and its neighbours, a workgroup of 256 and its neighbours (block_combine's grid), one row fewer and one
more than the rows a workgroup of block_gram covers (BLOCK_CHUNK of mi_kernels.h, read from the source), and 3 chunks with a
ragged tail.  Columns: 1, the 8-wide register tile of block_gram and its neighbours, two tiles, the widest block of the
eigensolver's test cases (51) and the widest allowed (60; block_combine writes at most 20).
Two calls give the same bits.
"""
import os
import re

import numpy as np
import pytest

from conftest import load_pkg

M = load_pkg()
pytestmark = pytest.mark.gpu

U = np.longdouble(2.0) ** -53
_src = open(os.path.join(M.PKG_DIR, "csrc", "mi_kernels.h")).read()
CHUNK = int(re.search(r"BLOCK_CHUNK\s*=\s*(\d+)", _src).group(1))
ROWS = [1, 63, 64, 65, 255, 257, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 1000]
GRAM_COLS = [(1, 1), (7, 9), (8, 8), (9, 7), (16, 1), (51, 51), (60, 60), (16, 60)]
COMBINE_COLS = [(1, 1), (7, 20), (8, 8), (9, 7), (16, 16), (51, 9), (60, 20), (60, 1)]


@pytest.fixture(scope="module")
def ctx():
    G = M.Context(dim=2, degree=1, reps=(2, 2), hi=(1.0, 1.0), face_role=[1, 7, 7, 7, 0, 0])
    yield G
    G.close()


def gamma(k):
    k = np.longdouble(k)
    return k * U / (1 - k * U)


def _block(rng, n, m):
    """entries of mixed sign and magnitude, some exact zeros"""
    a = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-3, 3, (n, m))
    a[rng.uniform(size=(n, m)) < 0.05] = 0.0
    return a


def _check(dev, ref, bnd, what):
    err = np.abs(dev.astype(np.longdouble) - ref)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    print("%s: worst error / bound %.3e" % (what, ratio))
    assert np.all(np.isfinite(dev))
    assert ratio <= 1.0
    assert np.all(err[~pos] == 0)


@pytest.mark.parametrize("ma,mb", GRAM_COLS)
@pytest.mark.parametrize("n", ROWS)
def test_block_gram(ctx, n, ma, mb):
    rng = np.random.default_rng(1000 * ma + 10 * mb + n)
    a, b = _block(rng, n, ma), _block(rng, n, mb)
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    ref = al.T @ bl
    bnd = gamma(n) * (np.abs(al).T @ np.abs(bl))
    c = M.block_gram(ctx, a, b)
    _check(c, ref, bnd, "block_gram n %d, %d x %d" % (n, ma, mb))
    assert np.array_equal(c, M.block_gram(ctx, a, b))


@pytest.mark.parametrize("ks,my", COMBINE_COLS)
@pytest.mark.parametrize("n", ROWS)
def test_block_combine(ctx, n, ks, my):
    rng = np.random.default_rng(1000 * ks + 10 * my + n + 7)
    s, coef = _block(rng, n, ks), _block(rng, ks, my)
    sl, cl = s.astype(np.longdouble), coef.astype(np.longdouble)
    ref = sl @ cl
    bnd = gamma(ks) * (np.abs(sl) @ np.abs(cl))
    y = M.block_combine(ctx, s, coef)
    _check(y, ref, bnd, "block_combine n %d, %d -> %d" % (n, ks, my))
    assert np.array_equal(y, M.block_combine(ctx, s, coef))


def test_hooks_refuse_what_the_kernels_do_not_cover(ctx):
    a = np.ones((4, 61))
    for call in (lambda: M.block_gram(ctx, a, a[:, :3]), lambda: M.block_gram(ctx, a[:, :3], a),
                 lambda: M.block_combine(ctx, a, np.ones((61, 2))), lambda: M.block_combine(ctx, a[:, :5], np.ones((5, 21)))):
        with pytest.raises(M.MiError) as e:
            call()
        assert e.value.code == M.MI_EINVAL
    assert np.array_equal(M.block_gram(ctx, a[:, :2], a[:, :3]), np.full((2, 3), 4.0))  # the context stays usable
