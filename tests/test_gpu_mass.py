"""GPU: mi_mass_apply and mi_mass_solve (Context.mass_apply, Context.mass_solve) -- the unit-density consistent mass on the
assembly's rule QGauss(p + 2), applied without a matrix, and its Jacobi-PCG on several columns at once -- against the dense
numpy reference tests/golden/projection_reference.py (anchored on the CPU by test_mirror_projection.py).

Meshes: projection_cases.MASS_MESHES.  Bounds, each derived and each figure printed before it is asserted:
  product   row by row |y - y_ref|_i <= gamma_k (|M| |x|)_i, gamma_k = k eps / (1 - k eps), the a-priori bound of an fp64 sum of k
            terms (the bound spmv_reference.py holds sell_spmv to).  k = 2 (npc + nq + 2^dim + 16): a row's entry is a sum over
            the npc nodes of a cell inside a sum over its nq points inside a sum over the at most 2^dim cells of a node, with at
            most 16 roundings in the products N N JxW and the Jacobian's determinant -- once for the device and once for the
            reference, which rounds as often.
  energies  1e-12 relative: two fp64 sums of the same positive terms (1/2 rho v^T M v against mi_energy's kinetic; the linear
            model's M / rho on a box mesh).
  solve     |x - x*|_2 <= kappa_2(M_ff) (res + 64 eps) |x*|_2 per column: x* is the dense solve, kappa_2 numpy's on that mesh,
            res the returned |b - M x| / |b|; 64 eps for the dense solve's own residual.  res <= tol at tol = 1e-12: the
            recurrence's residual and the freshly formed one part by about its eps kappa ~ 1e-14 here.
            Iterations: within +-2 of the numpy Jacobi-PCG on the same system and tolerance.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import point_eval_cases as PC  # noqa: E402
import projection_cases as PJ  # noqa: E402
import projection_reference as PR  # noqa: E402

M = load_pkg()
pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
TOL = 1e-12
_mass = {}


def _dense(key):
    """(mesh dict, dense scalar mass, kappa_2 of its free blocks): computed once, left unchanged"""
    if key not in _mass:
        c = PJ.mass_mesh(key)
        Md = PR.scalar_mass(c["mesh"])
        _mass[key] = (c, Md, PR.kappa2(Md, c["mesh"].dim, c["mesh"].constrained))
    return _mass[key]


def _columns(c, nrhs=6, seed=3):
    return np.random.default_rng(seed + c["mesh"].n).standard_normal((nrhs, c["mesh"].n))


def _gamma(k):
    return k * EPS / (1 - k * EPS)


# ------------------------------------------------------------------ product
@pytest.mark.parametrize("key", PJ.MASS_MESHES, ids=PJ.mesh_id)
def test_apply_against_the_dense_mass(key):
    c, Md, _ = _dense(key)
    m = c["mesh"]
    G = PC.context(M, c)
    x = _columns(c)
    k = 2 * (m.npc + (m.p + 2) ** m.dim + 2 ** m.dim + 16)
    worst = 0.0
    for masked in (False, True):
        y = G.mass_apply(x, masked=masked)
        ref = PR.mass_apply(Md, x, m.dim, m.constrained if masked else None)
        xa = np.abs(x) * (~m.constrained if masked else 1.0)
        bound = _gamma(k) * PR.mass_apply(np.abs(Md), xa, m.dim)
        rows = ~m.constrained if masked else np.ones(m.n, bool)
        worst = max(worst, float((np.abs(y - ref)[:, rows] / bound[:, rows]).max()))
        if masked:
            assert np.all(y[:, m.constrained] == 0.0)
    print("%s: worst |y - y_ref| / (gamma_%d |M||x|) = %.3e" % (PJ.mesh_id(key), k, worst))
    assert worst <= 1.0
    G.close()


@pytest.mark.parametrize("key", [(3, 1, (3, 2, 3), True), (3, 2, (3, 2, 3), True), (3, 3, (3, 2, 3), True), (3, 4, (1, 1, 1), True),
                                 (2, 4, (3, 2), True), (2, 2, (3, 2), False)], ids=PJ.mesh_id)
def test_kinetic_energy(key):
    c = PJ.mass_mesh(key)
    G = PC.context(M, c, rho=1234.5)
    v = _columns(c, 1)[0]
    G.set(M.V_V, v)
    e = G.energy()["kinetic"]
    mine = 0.5 * 1234.5 * float(v @ G.mass_apply(v))
    print("%s: kinetic %.17g, 1/2 rho v^T M v %.17g, rel %.2e" % (PJ.mesh_id(key), e, mine, abs(mine - e) / e))
    assert abs(mine - e) <= 1e-12 * e
    G.close()


@pytest.mark.parametrize("key", [(3, 2, (3, 2, 3), False), (3, 3, (3, 2, 3), False), (2, 3, (3, 2), False), (3, 1, (3, 2, 3), False)],
                         ids=PJ.mesh_id)
def test_equals_the_linear_models_mass_on_boxes(key):
    c = PJ.mass_mesh(key)
    G = PC.context(M, c, rho=1234.5)
    G.linear_setup(0.5)
    Ml = G.linear_csr(1)
    x = _columns(c)
    y, ref = G.mass_apply(x), (Ml @ x.T).T / 1234.5
    rel = float(np.abs(y - ref).max() / np.abs(ref).max())
    print("%s: relmax against linear_csr(1) / rho %.2e" % (PJ.mesh_id(key), rel))
    assert rel <= 1e-12
    G.close()


@pytest.mark.parametrize("key", [(3, 2, (3, 2, 3), True), (2, 3, (3, 2), True), (3, 2, (6, 5, 4), False)], ids=PJ.mesh_id)
def test_masked_semantics_and_repeatability(key):
    c = PJ.mass_mesh(key)
    m = c["mesh"]
    G = PC.context(M, c)
    x = _columns(c)
    xn = x.copy()
    xn[:, m.constrained] = np.nan  # read as 0, whatever stands there
    y = G.mass_apply(xn, masked=True)
    assert np.all(y[:, m.constrained] == 0.0) and np.all(np.isfinite(y))
    assert y.tobytes() == G.mass_apply(x * ~m.constrained, masked=True).tobytes()
    free = G.mass_apply(x * ~m.constrained)  # the unmasked product of the same vector: the same free rows
    assert np.array_equal(free[:, ~m.constrained], y[:, ~m.constrained])
    for masked in (False, True):
        a, b = G.mass_apply(x, masked=masked), G.mass_apply(x, masked=masked)
        assert a.tobytes() == b.tobytes()
        for j in (0, 5):  # a column does not depend on its neighbours
            assert a[j].tobytes() == G.mass_apply(x[j], masked=masked).tobytes()
    G.close()


# ------------------------------------------------------------------ solve
@pytest.mark.parametrize("key", PJ.MASS_MESHES, ids=PJ.mesh_id)
def test_solve_against_the_dense_solve(key):
    c, Md, kappa = _dense(key)
    m = c["mesh"]
    G = PC.context(M, c)
    b = _columns(c, seed=5)
    x, its, res, rc = G.mass_solve(b, masked=True, tol=TOL)
    ref = PR.solve(Md, b, m.dim, m.constrained)
    assert rc == M.MI_OK and np.all(x[:, m.constrained] == 0.0)
    err = np.linalg.norm(x - ref, axis=1) / np.linalg.norm(ref, axis=1)
    bound = kappa * (res + 64 * EPS)
    A = PR.VectorMass(Md, m.dim, m.constrained)
    its_ref = max(PR.jacobi_pcg(A, b[j], TOL, 500)[1] for j in range(6))
    print("%s: kappa_2 %.1f, res %.2e, |x - x*| / |x*| %.2e = %.3f of the bound, %d iterations (numpy %d)" %
          (PJ.mesh_id(key), kappa, res.max(), err.max(), float((err / bound).max()), its, its_ref))
    assert np.all(res <= TOL)
    assert np.all(err <= bound)
    assert abs(its - its_ref) <= 2
    G.close()


def test_solve_unmasked():
    key = (3, 2, (3, 2, 3), True)
    c, Md, _ = _dense(key)
    m = c["mesh"]
    G = PC.context(M, c)
    b = _columns(c, 2, seed=6)
    x, its, res, rc = G.mass_solve(b, masked=False, tol=TOL)
    none = np.zeros(m.n, bool)
    ref = PR.solve(Md, b, m.dim, none)
    ev = np.linalg.eigvalsh(Md)
    err = np.linalg.norm(x - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print("unmasked: res %.2e, err %.2e, bound %.2e, %d iterations" % (res.max(), err.max(), ev[-1] / ev[0] * (res.max() + 64 * EPS), its))
    assert rc == M.MI_OK and np.all(res <= TOL) and np.all(err <= ev[-1] / ev[0] * (res + 64 * EPS))
    G.close()


@pytest.mark.parametrize("key", [(3, 2, (3, 2, 3), True), (3, 2, (6, 5, 4), False), (2, 4, (3, 2), True)], ids=PJ.mesh_id)
def test_columns_together_equal_columns_alone(key):
    c = PJ.mass_mesh(key)
    G = PC.context(M, c)
    b = _columns(c, seed=7)
    b[1] *= 1e-3  # columns of different size and smoothness stop at different iterations
    b[4] = np.abs(b[4])
    x, its, res, _ = G.mass_solve(b, masked=True, tol=1e-10)
    slowest = 0
    for j in range(6):
        xj, itj, resj, _ = G.mass_solve(b[j], masked=True, tol=1e-10)
        assert xj.tobytes() == x[j].tobytes(), j
        assert resj[0] == res[j]
        slowest = max(slowest, itj)
    assert its == slowest
    x2 = G.mass_solve(b, masked=True, tol=1e-10)[0]
    assert x2.tobytes() == x.tobytes()
    G.close()


def test_zero_column_and_no_convergence():
    key = (3, 2, (3, 2, 3), True)
    c = PJ.mass_mesh(key)
    m = c["mesh"]
    G = PC.context(M, c)
    b = _columns(c, 3, seed=8)
    b[1] = 0.0
    x, its, res, rc = G.mass_solve(b, masked=True)
    assert rc == M.MI_OK and np.all(x[1] == 0.0) and res[1] == 0.0 and its > 2
    b0 = np.zeros((2, m.n))
    b0[:, m.constrained] = 7.0  # ignored on constrained dofs: still a zero column
    x, its, res, rc = G.mass_solve(b0, masked=True)
    assert rc == M.MI_OK and its == 0 and np.all(x == 0.0) and np.all(res == 0.0)
    with pytest.raises(M.MiError) as e:
        G.mass_solve(b, masked=True, max_it=2)
    assert e.value.code == M.MI_ENOCONV_LIN
    x, its, res, rc = e.value.partial
    assert its == 2 and res[0] > 1e-12 and res[2] > 1e-12 and res[0] < 1.0 and np.abs(x[0]).max() > 0.0 and np.all(x[1] == 0.0)
    G.close()


def test_modes_of_the_context():
    """no matrix is needed: "fine_level" 1 and a "linear_operator" 1 set-up return the bits of a plain context"""
    key = (3, 3, (3, 2, 3), True)
    c = PJ.mass_mesh(key)
    x = _columns(c)
    G = PC.context(M, c)
    y, (s, its, res, _) = G.mass_apply(x, masked=True), G.mass_solve(x, masked=True)
    G.close()
    F = PC.context(M, c)
    F.set_tuning("fine_level", 1)
    assert F.mass_apply(x, masked=True).tobytes() == y.tobytes()
    assert F.mass_solve(x, masked=True)[0].tobytes() == s.tobytes()
    F.close()
    L = PC.context(M, c)
    L.set_tuning("linear_operator", 1)
    L.linear_setup(0.5)
    assert L.mass_apply(x, masked=True).tobytes() == y.tobytes()
    assert L.mass_solve(x, masked=True)[0].tobytes() == s.tobytes()
    L.close()


def test_refusals():
    c = PC.make_mesh(3, 2, (2, 2, 4), False)
    m = c["mesh"]
    G = PC.context(M, c)
    L, dp = M.lib(), C.POINTER(C.c_double)
    x = np.zeros((7, m.n))
    y = np.full((7, m.n), 3.0)
    xp, yp = x.ctypes.data_as(dp), y.ctypes.data_as(dp)
    assert L.mi_mass_apply(G.h, 7, 0, xp, yp) == M.MI_EINVAL and "nrhs" in L.mi_last_error(G.h).decode()
    assert L.mi_mass_apply(G.h, -1, 0, xp, yp) == M.MI_EINVAL
    assert L.mi_mass_apply(G.h, 1, 2, xp, yp) == M.MI_EINVAL
    assert L.mi_mass_apply(G.h, 1, 0, None, yp) == M.MI_EINVAL and L.mi_mass_apply(G.h, 1, 0, xp, None) == M.MI_EINVAL
    assert L.mi_mass_apply(None, 1, 0, xp, yp) == M.MI_EINVAL
    assert L.mi_mass_apply(G.h, 0, 0, None, None) == M.MI_OK
    assert L.mi_mass_solve(G.h, 7, 1, xp, yp, 1e-12, 10, None, None) == M.MI_EINVAL
    assert L.mi_mass_solve(G.h, 1, 1, None, yp, 1e-12, 10, None, None) == M.MI_EINVAL
    assert L.mi_mass_solve(G.h, 1, 1, xp, yp, -1.0, 10, None, None) == M.MI_EINVAL
    assert L.mi_mass_solve(G.h, 0, 1, None, None, 1e-12, 10, None, None) == M.MI_OK
    assert np.all(y == 3.0)  # a refused call writes nothing
    G.close()
    T = PC.context(M, c, slabs=2)
    assert T.comm_info()[0] == 2
    assert L.mi_mass_apply(T.h, 1, 0, xp, yp) == M.MI_EINVAL and "one slab only" in L.mi_last_error(T.h).decode()
    assert L.mi_mass_solve(T.h, 1, 0, xp, yp, 1e-12, 10, None, None) == M.MI_EINVAL
    T.close()
