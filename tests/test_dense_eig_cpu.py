"""The host's dense generalised eigensolver (mi_dense_sym_eig: Cholesky of B + cyclic Jacobi, what mi_linear_modes solves its
Rayleigh-Ritz problems with) against scipy.linalg.eigh(A, B).  No device.

Pencils: B = Q diag(d) Q^T with d in [0.5, 2] (so that the reduction to standard form, in the solver and in the reference, costs
no more than a factor 4 of accuracy), A = L Q' diag(w) Q'^T L^T with L the Cholesky factor of B: the eigenvalues are the chosen w.
  random      w log-uniform over three decades
  repeated    a triple and a double eigenvalue among them
  singular    A with a null space of dimension max(1, n // 4)
Assertions, with s = |B^-1 A|_2 = max |w|:  |w - w_ref| <= 64 n eps s,  |V^T B V - I|_max <= 64 n eps,
|V^T A V - diag w|_max <= 64 n eps s.
"""
import numpy as np
import pytest
import scipy.linalg as sla

from conftest import load_pkg

M = load_pkg()
EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 7, 48, 60]


def _orth(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def pencil(n, kind, seed):
    rng = np.random.default_rng(seed)
    Q = _orth(rng, n)
    B = (Q * rng.uniform(0.5, 2.0, n)) @ Q.T
    B = 0.5 * (B + B.T)
    w = 10.0 ** rng.uniform(0.0, 3.0, n)
    if kind == "repeated" and n >= 2:
        w[:min(3, n)] = w[0]
        if n >= 7:
            w[4:6] = w[4]
    if kind == "singular":
        w[:max(1, n // 4)] = 0.0
    L = np.linalg.cholesky(B)
    LQ = L @ _orth(rng, n)
    A = (LQ * w) @ LQ.T
    return 0.5 * (A + A.T), B, np.sort(w)


@pytest.mark.parametrize("kind", ["random", "repeated", "singular"])
@pytest.mark.parametrize("n", SIZES)
def test_dense_sym_eig_against_scipy(n, kind):
    A, B, w_made = pencil(n, kind, seed=100 * n + len(kind))
    w_ref = sla.eigh(A, B, eigvals_only=True)
    s = max(np.abs(w_ref).max(), np.abs(w_made).max())
    w, V = M.dense_sym_eig(A, B)
    tol = 64 * n * EPS
    sp = s if s > 0 else 1.0  # (n = 1 singular: A = 0)
    print("n %d %s: |w - w_ref| / s %.2e, |V^T B V - I| %.2e, |V^T A V - diag w| / s %.2e (bound %.2e)" %
          (n, kind, np.abs(w - w_ref).max() / sp, np.abs(V.T @ B @ V - np.eye(n)).max(),
           np.abs(V.T @ A @ V - np.diag(w)).max() / sp, tol))
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - w_ref).max() <= tol * s
    assert np.abs(V.T @ B @ V - np.eye(n)).max() <= tol
    assert np.abs(V.T @ A @ V - np.diag(w)).max() <= tol * s


def test_dense_sym_eig_refuses_an_indefinite_b():
    A = np.eye(3)
    B = np.diag([1.0, -1.0, 1.0])
    with pytest.raises(M.MiError) as e:
        M.dense_sym_eig(A, B)
    assert e.value.code == M.MI_EINVAL
    with pytest.raises(M.MiError):
        M.dense_sym_eig(np.eye(65), np.eye(65))
