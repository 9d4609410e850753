"""The inputs of the reaction tests, shared by test_mirror_reactions.py (CPU) and test_gpu_reactions.py (the device against the
reference): the meshes, material, roles and displacement states of stress_cases.py (imported, not edited -- x- clamped, x+ / y+
the interface, z- clamped in z: every case has fully and partly constrained nodes and interface nodes that meet the clamp),
plus, seeded per case:

  acceleration  3 randn on every dof               (model 1: v_old = randn, v = v_old + DT * that acceleration)
  body force    (0.3, -9.81, 1.0)
  traction      1e3 randn on the interface nodes   (model 1: the load vector MI_L_OLD_STRESS = 1e3 randn on every dof)

Every case is built once and left unchanged; ref(case, model, about) is computed once.
"""
import numpy as np

import reactions_reference as R
import stress_cases as SC

MU, NU, RHO = SC.MU, SC.NU, SC.RHO
BODY = (0.3, -9.81, 1.0)
DT = 0.005
ABOUT = (0.13, -0.21, 0.34)  # a point off the mesh and off the origin for the moment tests
(L_DISPLACEMENT, L_OLD_DISPLACEMENT, L_VELOCITY, L_OLD_VELOCITY, L_OLD_STRESS) = range(5)  # the MI_L_* slots of include/mi_elasticity.h

_refs = {}


def case(dim, p, reps, perturbed):
    c = SC.case(dim, p, reps, perturbed)
    if "acc" not in c:
        m = c["mesh"]
        rng = np.random.default_rng(7000 + 100 * dim + 10 * p + sum(reps) + int(perturbed))
        c["acc"] = 3.0 * rng.standard_normal(m.n)
        c["traction"] = np.zeros(m.n)
        ids = m.interface_nodes
        c["traction"].reshape(-1, dim)[ids] = 1e3 * rng.standard_normal((len(ids), dim))
        c["v_old"] = rng.standard_normal(m.n)
        c["v"] = c["v_old"] + DT * c["acc"]
        c["f_old"] = 1e3 * rng.standard_normal(m.n)
    return c


def ref_terms(c, model):
    m = c["mesh"]
    if model == R.NEOHOOKE:
        return R.terms(m, model, c["u"], c["acc"], MU, NU, RHO, body=BODY, traction=c["traction"])
    return R.terms(m, model, c["u"], (c["v"] - c["v_old"]) / DT, MU, NU, RHO, load=c["f_old"])


def ref(c, model, about=None):
    """(terms[4, n], resultants about `about`, smallest det F) of the reference"""
    if ("terms", id(c), model) not in _refs:
        _refs[("terms", id(c), model)] = ref_terms(c, model)
    T, det = _refs[("terms", id(c), model)]
    key = (id(c), model, about)
    if key not in _refs:
        _refs[key] = R.resultants(c["mesh"], model, c["u"], T, about)
    return T, _refs[key], det
