"""Meshes, pairs of meshes and source states shared by test_mirror_projection.py, test_gpu_mass.py and
test_gpu_state_project.py.  The meshes are those of point_eval_cases.py (edges 0.1, 0.13, 0.07 per cell, plain or with the
vertices moved by 0.05 hmin randn; x- clamped, z- clamped in z, so the components' free sets differ).

MASS_MESHES: (dim, p, reps, perturbed) -- the smallest on which each kernel can go wrong: 3 x 2 x 3 (all eight colours, nodes
shared across faces, edges and corners), one cell, 3 x 2 in 2D, each plain and perturbed, and 6 x 5 x 4 Q2, whose 3861 dofs
per column are four workgroups of the column algebra (1024 entries each), so a column's sums pass through several partials.

Pairs: (name, src, dst, sub) with src / dst = (dim, p, reps, perturbed, refine).  EXACT_PAIRS are those on which the composite
rule integrates the load exactly (src.reps = sub * dst.reps on boxes, or equal lattices with sub = 1)."""
import numpy as np

import mirror as Mi
import point_eval_cases as PC

REPS = {2: (3, 2), 3: (3, 2, 3)}
MASS_MESHES = ([(3, p, (3, 2, 3), pert) for p in (1, 2, 3, 4) for pert in (False, True)] +
               [(3, p, (1, 1, 1), pert) for p in (1, 2, 3, 4) for pert in (False, True)] +
               [(2, p, (3, 2), pert) for p in (1, 2, 3, 4) for pert in (False, True)] + [(3, 2, (6, 5, 4), False)])


def mesh_id(key):
    dim, p, reps, pert = key
    return "%dD-Q%d-%s%s" % (dim, p, "x".join(map(str, reps)), "-perturbed" if pert else "")


def mass_mesh(key, roles=None):
    dim, p, reps, pert = key
    return PC.make_mesh(dim, p, reps, pert, roles=roles)


EXACT_PAIRS = [
    ("identity", (3, 2, (3, 2, 3), True, 1), (3, 2, (3, 2, 3), True, 1), 1),
    ("refine-Q2", (3, 2, (3, 2, 3), False, 1), (3, 2, (3, 2, 3), False, 2), 1),
    ("coarsen-Q2", (3, 2, (2, 1, 2), False, 2), (3, 2, (2, 1, 2), False, 1), 2),
    ("coarsen-Q3", (3, 3, (2, 1, 2), False, 2), (3, 3, (2, 1, 2), False, 1), 2),
    ("degree-drop", (3, 3, (3, 2, 3), False, 1), (3, 2, (3, 2, 3), False, 1), 1),
    ("degree-drop-perturbed", (3, 3, (3, 2, 3), True, 1), (3, 2, (3, 2, 3), True, 1), 1),
    ("coarsen-2D-Q1-sub3", (2, 1, (3, 2), False, 3), (2, 1, (3, 2), False, 1), 3),
]
SAMPLING_LOSES = ("coarsen-Q2", "coarsen-Q3", "degree-drop", "degree-drop-perturbed")  # sampling is worse than projecting
NON_NESTED = ("non-nested", (3, 2, (3, 2, 3), False, 1), (3, 2, (2, 2, 2), False, 1), 1)  # the same box in 2 x 2 x 2 cells


def pair_id(case):
    return case[0]


_boxes = {}


def _mesh(spec, roles, like=None):
    dim, p, reps, pert, refine = spec
    if like is None:
        return PC.make_mesh(dim, p, reps, pert, roles=roles, refine=refine)
    # the box of `like` in reps cells (no lattice of point_eval_cases: non-nested)
    key = (spec, tuple(roles or PC.ROLES[:2 * dim]), like["hi"])
    if key not in _boxes:
        r = list(PC.ROLES[:2 * dim] if roles is None else roles)
        _boxes[key] = dict(dim=dim, p=p, reps=tuple(reps), lo=like["lo"], hi=like["hi"], perturb=None, roles=r,
                           mesh=Mi.Mesh(dim, p, reps, like["lo"], like["hi"], r))
    return _boxes[key]


def pair(case, roles=None):
    """(src, dst, sub): the dicts of point_eval_cases.make_mesh"""
    name, s, d, sub = case
    cs = _mesh(s, roles)
    return cs, _mesh(d, roles, like=cs if name == "non-nested" else None), sub


def source_state(c, seed=11):
    """ten random vectors with zeros on the constrained dofs (the recipe of test_gpu_state_transfer.py)"""
    m = c["mesh"]
    return np.random.default_rng(seed + m.n).standard_normal((10, m.n)) * ~m.constrained
