"""CPU: anchors tests/golden/explicit_reference.py, the numpy reference tests/test_gpu_explicit.py holds the device's explicit
time integrator to.

  force                the residual-only, vectorised force equals Solid.assemble's right-hand side with a = 0 (1e-13 of its maximum)
  lumped weights       W > 0, sum W = volume, rho W = the row sums of the mirror's consistent mass
  linearised answer    from u = eps phi_1 (lowest mode of K_T(0) phi = lambda M_L phi by dense eigh, eps = 1e-7), v = 0, the modal
                       coefficient c_n = phi_1^T M_L u_n / eps obeys c_{n+1} - 2 cos(theta) c_n + c_{n-1} = 0 with cos(theta) = 1 -
                       lambda_1 dt^2 / 2: pins the factor 1/2, the mass and the sign of the force.  Measured 1e-14 .. 7.1e-12 on the seven SMALL
                       cases at dt = 1/2 dt_crit (the floor is the O(eps) nonlinearity); asserted 1e-8
  reversibility        n steps, flip v, n steps at finite amplitude return to the start; the bound is 100 x the error recorded
                       below (REVERSIBILITY_MEASURED)
  stability estimate   the 40-step Ritz value theta: 0.9 lambda_max <= theta <= lambda_max (1 + 1e-12) against dense eigh.  The 0.9 is a
                       condition (with the safety factor 0.8 it keeps 0.8 * 2 / sqrt(theta) below the true limit), not a measurement
  rounding sensitivity two reference runs of 10 steps, one with the force multiplied by 1 + 1e-15 randn each step, differ by <= 1e-13
                       of each field's maximum on every GPU case: the 1e-12 tolerance of the device comparison has a tenfold margin
                       over summation-order effects
  fold case            the velocity field of the GPU fold test inverts a cell at a step k >= 3 with det F well away from 0 before
                       and at that step, so the device's flag and the reference's agree on k
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import explicit_reference as ER  # noqa: E402
import mirror as Mi  # noqa: E402

# |state after n steps, v flipped, n steps more - start| / max|u|, n = 10 at 1/2 dt_crit, measured with this file: 2.2e-15 .. 5.4e-15 over the SMALL cases
REVERSIBILITY_MEASURED = 5.4e-15


@pytest.mark.parametrize("name", ["2d_q2_61", "q1_222", "q2_311p", "2d_q3_21"])
def test_force_is_the_mirrors_residual_without_inertia(name):
    R = ER.reference(name)
    u, _, _ = R.initial()
    S = Mi.Solid(R.mesh, mu=ER.MU, nu=ER.NU, rho=ER.RHO, body=ER.BODY[:R.dim])
    S.stress[:] = R.stress
    S.u[:] = u
    _, rhs = S.assemble(np.zeros(R.mesh.n))
    F = R.force(u)
    err = np.abs(F - rhs).max() / np.abs(rhs).max()
    print("%s: |force - Solid.assemble| / max = %.2e" % (name, err))
    assert np.abs(rhs).max() > 0 and err <= 1e-13


@pytest.mark.parametrize("name", list(ER.CASES))
def test_lumped_weights(name):
    R = ER.reference(name)
    m, dim, p = R.mesh, R.dim, R.p
    assert np.all(R.W > 0)
    volume = R.JxW.sum()
    assert abs(R.W.sum() / dim - volume) <= 1e-13 * volume
    # row sums of the mirror's consistent mass: sum_b sum_q N_a N_b JxW per cell, from shape_at / q1_jacobian point by point
    nodes = Mi.feq_nodes(p)
    qx, qw = Mi.gauss01(p + 2)
    rows = np.zeros(m.nnodes)
    for conn, verts, _ in m.cells:
        Me = np.zeros((m.npc, m.npc))
        for q in np.ndindex(*([p + 2] * dim)):
            qi = q[::-1]
            xi = np.array([qx[k] for k in qi])
            N, _ = Mi.shape_at(dim, p, nodes, xi)
            Me += np.outer(N, N) * np.linalg.det(Mi.q1_jacobian(dim, verts, xi)) * np.prod([qw[k] for k in qi])
        np.add.at(rows, conn, Me.sum(axis=1))
    assert np.abs(ER.RHO * np.repeat(rows, dim) - R.mass).max() <= 1e-13 * R.mass.max()


@pytest.mark.parametrize("name", ER.SMALL)
def test_linearised_known_answer(name):
    R = ER.reference(name)
    zero = np.zeros(R.mesh.n)
    K, mf, free = R.dense_pencil(zero)
    s = 1.0 / np.sqrt(mf)
    w, V = np.linalg.eigh(K * s[:, None] * s[None, :])
    phi = np.zeros(R.mesh.n)
    phi[free] = V[:, 0] * s  # M_L-normalised
    dt = 0.5 * 2.0 / np.sqrt(w[-1])
    cos_t = 1.0 - w[0] * dt * dt / 2
    eps = 1e-7
    # no load: the recurrence is that of the homogeneous problem
    stress, body = R.stress, R.body
    R.stress, R.body = np.zeros_like(stress), np.zeros_like(body)
    try:
        u, v = eps * phi, zero.copy()
        a = R.minv * R.force(u)
        c = [phi @ (R.mass * u) / eps]
        for _ in range(12):
            u, v, a = R.step(u, v, a, dt)
            c.append(phi @ (R.mass * u) / eps)
    finally:
        R.stress, R.body = stress, body
    c = np.array(c)
    defect = np.abs(c[2:] - 2 * cos_t * c[1:-1] + c[:-2]).max()
    print("%s: recurrence defect %.2e (lambda_1 %.4g, dt %.3e)" % (name, defect, w[0], dt))
    assert abs(c[0] - 1.0) < 1e-12 and defect <= 1e-8


@pytest.mark.parametrize("name", ER.SMALL)
def test_time_reversibility(name):
    R = ER.reference(name)
    dt = ER.dt_half_crit(name)
    u0, v0, a0 = R.initial()
    u, v, a = R.run(u0, v0, a0, dt, 10)[-1]
    u, v, a = R.run(u, -v, a, dt, 10)[-1]
    scale = max(np.abs(u0).max(), np.abs(u - u0).max())
    err = max(np.abs(u - u0).max() / np.abs(u0).max(), np.abs(v + v0).max() / np.abs(v0).max())
    print("%s: return error %.2e" % (name, err))
    assert scale > 0 and err <= 100 * REVERSIBILITY_MEASURED


@pytest.mark.parametrize("name", ER.SMALL)
def test_stability_estimate(name):
    R = ER.reference(name)
    u, _, _ = R.initial()
    K, mf, _ = R.dense_pencil(u)
    lam = ER.lambda_max_dense(K, mf)
    theta = R.lanczos(R.tangent(u), 40)
    print("%s: theta / lambda_max = %.12f, dt_crit %.4e" % (name, theta / lam, 2 / np.sqrt(theta)))
    assert 0.9 * lam <= theta <= lam * (1 + 1e-12)


@pytest.mark.parametrize("name", list(ER.CASES))
def test_rounding_sensitivity(name):
    R = ER.reference(name)
    dt = ER.dt_half_crit(name)
    u0, v0, a0 = R.initial()
    assert 1e-3 < np.abs(u0).max() < 1e-2 and np.abs(v0).max() <= 8.0 + 1e-12
    A = R.run(u0, v0, a0, dt, ER.STEPS)[-1]
    B = R.run(u0, v0, a0, dt, ER.STEPS, noise=np.random.default_rng(7))[-1]
    rel = [np.abs(x - y).max() / np.abs(x).max() for x, y in zip(A, B)]
    print("%s: dt %.3e, sensitivity u %.1e v %.1e a %.1e" % (name, dt, *rel))
    assert max(rel) <= 1e-13


@pytest.mark.parametrize("name", ["q2_311p", "q3_211", "2d_q2_61"])
def test_fold_case_is_decisive(name):
    R = ER.reference(name)
    dt = ER.dt_half_crit(name)
    u0, _, _ = R.initial()
    v = ER.fold_velocity(R.mesh.coords, dt)
    a = R.minv * R.force(u0)
    k, before, at = R.fold_step(u0, v, a, dt, 12)
    print("%s: folds at step %d, min det F before %.3f, at %.3f" % (name, k, before, at))
    assert k >= 3 and before > 0.02 and at < -0.02
