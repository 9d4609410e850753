"""CPU anchor of tests/golden/reactions_reference.py, the numpy reference the device's nodal forces and resultants (mi_reactions)
are held to (test_gpu_reactions.py).  No device, no library:

  (1) model 0: internal + inertia - body of the reference equals -r_e of mirror.cell summed over the cells, on EVERY dof, and
      -(forces) equals the right-hand side of mirror.Solid.assemble on the free dofs (traction included), to 1e-12 of the largest
      term's max -- on the cheap cases (mirror.cell forms K_e: 3D Q3 and Q4 cost minutes there)
  (2) model 0: the reference's load equals mirror.neumann_cell: the difference of two Solid.assemble right-hand sides with and
      without traction on the free dofs
  (3) model 1: internal = Linear.K @ d and inertia = Linear.M @ a, to 1e-12 of their max
  (4) the two round-off identities, on every case of the GPU file: sum_all internal = 0 and sum_all (x_i - x0) x internal_i = 0
      with the CURRENT positions x_i = X_i + u_i (model 0; X_i for model 1), each <= 1e-14 of the sum of the absolute values of its
      addends; translation and rotation invariance of the internal virtual work
  (5) the model-0 moment taken about X_i instead is >= 1e-5 of that scale on every perturbed case: the identity tells a kernel
      that uses the wrong positions from a right one
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import reactions_cases as RC  # noqa: E402
import reactions_reference as R  # noqa: E402
import stress_cases as SC  # noqa: E402

MU, NU, RHO = RC.MU, RC.NU, RC.RHO
CHEAP = SC.GENERIC_MESHES[:5] + [SC.Q2_MESHES[0]]
ALL_MESHES = SC.Q3_MESHES + SC.Q2_MESHES + SC.GENERIC_MESHES
LINEAR_MESHES = SC.GENERIC_MESHES + [SC.Q2_MESHES[1], SC.Q3_MESHES[1]]


def _solid(c, traction):
    m = c["mesh"]
    S = Mi.Solid(m, mu=MU, nu=NU, rho=RHO, body=RC.BODY[:m.dim] + (0.0,) * (3 - m.dim), dt=RC.DT)
    S.u, S.a = c["u"].copy(), c["acc"].copy()
    S.stress = traction.copy()
    return S


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", CHEAP)
def test_model0_terms_are_the_mirrors_residual(mesh, perturbed):
    c = RC.case(*mesh, perturbed)
    m, dim = c["mesh"], c["dim"]
    T, res, det = RC.ref(c, R.NEOHOOKE)
    assert det >= 0.4
    scale = np.abs(T).max()
    S = _solid(c, c["traction"])
    re = np.zeros(m.n)
    for conn, verts, _ in m.cells:
        d = m.dofs(conn)
        re[d] += Mi.cell(dim, m.p, verts, c["u"][d], c["acc"][d], MU, NU, RHO, S.a1, S.body)[1]
    e1 = np.abs(T[0] + T[1] - T[2] + re).max() / scale
    _, rhs = S.assemble(np.zeros(m.n))
    _, rhs0 = _solid(c, np.zeros(m.n)).assemble(np.zeros(m.n))
    free = ~m.constrained
    e2 = np.abs(rhs + res["forces"])[free].max() / scale
    e3 = np.abs((rhs - rhs0) - T[3])[free].max() / scale
    print("cells %.2e, assembled rhs %.2e, load %.2e of the largest term" % (e1, e2, e3))
    assert e1 <= 1e-12 and e2 <= 1e-12 and e3 <= 1e-12
    assert np.abs(T[3]).max() > 0 and np.abs(T[3][m.constrained]).max() > 0  # interface nodes meet the clamp: load on constrained dofs


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mesh", LINEAR_MESHES)
def test_model1_terms_are_K_d_and_M_a(mesh, perturbed):
    c = RC.case(*mesh, perturbed)
    m = c["mesh"]
    T, _, _ = RC.ref(c, R.LINEAR)
    L = Mi.Linear(m, mu=MU, nu=NU, rho=RHO, dt=RC.DT)
    Kd, Ma = L.K @ c["u"], L.M @ ((c["v"] - c["v_old"]) / RC.DT)
    e1, e2 = np.abs(T[0] - Kd).max() / np.abs(Kd).max(), np.abs(T[1] - Ma).max() / np.abs(Ma).max()
    print("K d %.2e, M a %.2e" % (e1, e2))
    assert e1 <= 1e-12 and e2 <= 1e-12
    assert np.array_equal(T[3], c["f_old"]) and not T[2].any()


@pytest.mark.parametrize("mesh,perturbed,model", SC.REFERENCE_CASES)
def test_internal_forces_have_no_resultant_and_no_moment(mesh, perturbed, model):
    c = RC.case(*mesh, perturbed)
    for about in (None, RC.ABOUT[:c["dim"]]):
        T, res, _ = RC.ref(c, model, about)
        ef = np.abs(res["internal"]).max() / res["internal_abs"]
        em = np.abs(res["internal_moment"]).max() / res["internal_moment_scale"].max()
        print("about %s: sum %.2e of sum|internal|, moment %.2e of its absolute sum" % (about, ef, em))
        assert ef <= 1e-14 and em <= 1e-14
    if model == R.NEOHOOKE and perturbed:
        wrong = R.resultants(c["mesh"], R.LINEAR, c["u"], T)  # the positions of model 1: X_i
        ew = np.abs(wrong["internal_moment"]).max() / res["internal_moment_scale"].max()
        print("moment about X_i: %.2e of the scale" % ew)
        assert ew >= 1e-5
