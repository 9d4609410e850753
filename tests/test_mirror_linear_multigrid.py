"""CPU: the numpy V-cycle of the linear model (tests/golden/linear_mg_reference.py), anchored before the GPU tests trust it.

On every case of the GPU table (theta = 0.5, dt = 0.02, default material), with lmax = 1.15 x the true lambda_max(D^-1 A):
  * B is symmetric, x . B y = y . B x to 1e-12 of |x| . |B y|, and x . B x > 0, on random vectors;
  * E_LIN: the relmax between the float64 and the long double cycle on a random right-hand side is measured, and the worst
    is what linear_mg_reference.E_LIN states (rounded up); the tolerance of the GPU cycle test rests on it;
  * PCG from zero to 1e-10 |b|: the cycle needs at most half of Jacobi's iterations.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import linear_mg_reference as LR  # noqa: E402
import pcg_reference as P  # noqa: E402

_lmax = {}


def _case(name):
    ref = LR.reference(name)
    if name not in _lmax:
        _lmax[name] = ref.true_lmax()
    return ref, _lmax[name]


@pytest.mark.parametrize("name", list(LR.CASES))
def test_cycle_is_symmetric_and_positive(name):
    ref, lmax = _case(name)
    m = ref.meshes[0]
    rng = np.random.default_rng(len(name))
    free = ~m.constrained
    for _ in range(2):
        x, y = rng.standard_normal(m.n) * free, rng.standard_normal(m.n) * free
        Bx, By = ref.vcycle(x, lmax), ref.vcycle(y, lmax)
        asym = abs(x @ By - y @ Bx) / (np.abs(x) @ np.abs(By))
        print("%s: asymmetry %.1e, x.Bx %.3e" % (name, asym, x @ Bx))
        assert asym <= 1e-12
        assert x @ Bx > 0 and y @ By > 0


def test_reference_rounding_on_the_gpu_cases():
    """e per case: float64 against long double cycle, random right-hand side, true lmax x 1.15"""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = 0.0
    for name in LR.CASES:
        ref, lmax = _case(name)
        m = ref.meshes[0]
        r = np.random.default_rng(5).standard_normal(m.n) * ~m.constrained
        z, zl = ref.vcycle(r, lmax), ref.vcycle(r, lmax, np.longdouble)
        e = float(np.abs(z - zl).max() / np.abs(zl).max())
        print("e_lin %-10s %.2e" % (name, e))
        assert e <= LR.E_LIN, (name, e)  # (each on its own: a NaN fails)
        worst = max(worst, e)
    print("worst e_lin %.3e" % worst)
    assert LR.E_LIN / 4 <= worst <= LR.E_LIN  # the constant is the measurement, rounded up


@pytest.mark.parametrize("name", list(LR.CASES))
def test_cycle_halves_the_jacobi_iterations(name):
    ref, lmax = _case(name)
    m = ref.meshes[0]
    A = P.Matrix(ref.A[0])
    b = np.random.default_rng(11).standard_normal(m.n) * ~m.constrained
    tol = 1e-10 * np.linalg.norm(b)
    its = {}
    for pre, Minv, K in (("vcycle", P.vcycle(ref, lmax), 50), ("jacobi", P.jacobi(ref.A[0]), 600)):
        with np.errstate(invalid="ignore", divide="ignore"):  # (the recurrence runs on past convergence on the small cases)
            rn = P.pcg(A, Minv, b, np.zeros(m.n), K)[1]
        its[pre] = P.first_converged(rn, tol)
        assert its[pre] is not None, (pre, rn[-1] / rn[0])  # (measured: 9-34 cycles, 100-318 Jacobi iterations)
    print("%s: Jacobi %d, V-cycle %d iterations" % (name, its["jacobi"], its["vcycle"]))
    assert 2 * its["vcycle"] <= its["jacobi"]
