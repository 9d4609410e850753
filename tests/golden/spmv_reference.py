"""Reference of the matrix-vector product y = A x for the sliced-ELL kernels, with an a-priori rounding bound.

  product(csr, x)   y = A x in np.longdouble: data and x cast up, the products summed row by row with np.add.reduceat over
                    indptr.  No scipy kernel takes part (they exist in double only).
  bound(csr, x)     componentwise: row i gets gamma_n (|A| |x|)_i with gamma_n = n u / (1 - n u), n = the number of scalar
                    entries of the row plus one, u = 2^-53.  gamma_(n-1) (|A| |x|)_i bounds the error of an fp64 dot product of
                    n - 1 terms summed in ANY order, with or without FMA (Higham, Accuracy and Stability of Numerical
                    Algorithms, 2nd ed., (3.5) and section 3.1: every term passes through at most n - 1 roundings, an FMA
                    removes one of them); the one further u covers the rounding of the long double reference itself and of
                    its conversion (2^-64 per operation, far below u / n for any row here).  Derived, not measured: no margin
                    is added anywhere.
  f32=True          the matrix values rounded to fp32 first (the smoother's copy under "precond_storage" 32); the arithmetic of
                    that kernel is fp64 on the widened values, so product and bound are those of the rounded matrix.

Zero entries that the device pads its rows with add exact zeros to a sum and leave both the value and the bound as they are.
Rows without an entry have bound 0: the kernel must write an exact zero there.
"""
import numpy as np

U = 2.0 ** -53


def _values(csr, f32):
    v = np.asarray(csr.data, dtype=np.float64)
    if f32:
        v = v.astype(np.float32)
    return v.astype(np.longdouble)


def _row_sums(csr, terms):
    """sum of terms[indptr[i] : indptr[i + 1]] per row (np.add.reduceat, which needs the empty rows taken out: it would
    return the element AT the index for them)"""
    indptr = np.asarray(csr.indptr, dtype=np.int64)
    y = np.zeros(csr.shape[0], np.longdouble)
    rows = np.nonzero(np.diff(indptr) > 0)[0]
    if len(rows):
        y[rows] = np.add.reduceat(terms, indptr[rows])
    return y


def product(csr, x, f32=False):
    x = np.asarray(x).astype(np.longdouble)
    return _row_sums(csr, _values(csr, f32) * x[csr.indices])


def bound(csr, x, f32=False):
    x = np.asarray(x).astype(np.longdouble)
    n = (np.diff(np.asarray(csr.indptr, dtype=np.int64)) + 1).astype(np.longdouble)
    gamma = n * np.longdouble(U) / (1 - n * np.longdouble(U))
    return gamma * _row_sums(csr, np.abs(_values(csr, f32)) * np.abs(x)[csr.indices])


def worst_ratio(y, csr, x, f32=False):
    """(max over the rows with a non-zero bound of |y - y_ref| / bound, whether every row with a zero bound is exactly its
    reference value -- which is zero)"""
    ref, bnd = product(csr, x, f32), bound(csr, x, f32)
    err = np.abs(np.asarray(y).astype(np.longdouble) - ref)
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    return ratio, bool(np.all(err[~pos] == 0))
