"""GPU: the executables' MI_REACTIONS=1 and MI_VTK_REACTIONS=1 -- support reactions and load resultants (mi_reactions) as
reactions.log beside the displacement log and as the point-data vector `reaction_force` of the .vtk files.

The cases and _run of test_host_gpu_stress.py: block_neo_3d_q2 on elasticity3d (neo-Hookean: model 0) and fsi3_linear_2d_shipped
on elasticity (model 1).  Without the switches the file lists are what they were.  A switched .vtk file is the plain file plus a
trailing `VECTORS reaction_force` block: zero on free nodes, and summed over the nodes it is the logged reaction of that time at
1e-6 of the largest entry (the file carries 12 digits).  The unbalanced resultant is no column of the log, so the force identity
reaction + unbalanced = inertia - body - load is checked in the form the columns allow: the unbalanced resultant is a sum of
n_free numbers none larger than max_unbalanced, so |reaction - (inertia - body - load)| <= n_free max_unbalanced per component,
plus 1e-6 of the row's largest entry.

max_unbalanced against the solver's tolerance.  Model 0: the Newton loop stops when the residual norm is <= `Tolerance force` of
the step's first residual norm or <= 5e-9 (nonlinear_elasticity.cc:459-463); a max is bounded by the 2-norm, so
max_unbalanced <= max(5e-9, tol_f res_0) + 1e-12 of the row's largest entry, with res_0 read from the first row of the step's Newton
table (four digits: a factor 1.001).  Model 1: the shipped case runs the theta scheme with theta = 0.5, for which one call is no
equilibrium statement (include/mi_elasticity.h), so that run serves the file lists, the VTK block and the shape of the log; the
same case with `set theta = 1` holds every row to max_unbalanced <= abs_tol / dt + the round-off term, which makes the force
identity's slack n_free max_unbalanced as small there as it is for model 0.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_host_gpu_stress import CASES, HOST, _run  # noqa: E402

pytestmark = pytest.mark.gpu

COLUMNS = 17  # t, reaction 3, reaction moment 3, load 3, inertia 3, body 3, max_unbalanced


def _run_stdout(name, exe, d, env, edit=None):
    """_run of test_host_gpu_stress.py, returning the executable's output as well (the Newton tables); edit: parameters.prm -> the
    text the run reads"""
    d.mkdir()
    for f in ("parameters.prm", "precice-config.xml"):
        txt = open(os.path.join(CASES, name, f)).read()
        (d / f).write_text(edit(txt) if edit and f == "parameters.prm" else txt)
    out = subprocess.run([os.path.join(HOST, exe)], cwd=d, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return sorted(os.listdir(d / "out")), out.stdout


def _log(d):
    lines = open(d / "reactions.log").read().split("\n")
    assert lines[0].startswith("# t reaction_x") and "max_unbalanced" in lines[0]
    rows = np.array([l.split() for l in lines[1:] if l], dtype=float)
    assert rows.shape[1] == COLUMNS
    return rows


def _reaction_block(path, dim):
    txt = open(path).read().split("\n")
    i = next(k for k, l in enumerate(txt) if l.startswith("POINTS"))
    npts = int(txt[i].split()[1])
    pts = np.array([l.split() for l in txt[i + 1:i + 1 + npts]], dtype=float)[:, :dim]
    j = next(k for k, l in enumerate(txt) if l.startswith("VECTORS displacement"))
    disp = np.array([l.split() for l in txt[j + 1:j + 1 + npts]], dtype=float)[:, :dim]
    k = next(k for k, l in enumerate(txt) if l.startswith("VECTORS reaction_force"))
    assert [l for l in txt[k + 1 + npts:] if l] == []  # the trailing block
    return pts - disp, np.array([l.split() for l in txt[k + 1:k + 1 + npts]], dtype=float)


def _check_vtk(plain, switched, mesh, row):
    a, b = open(plain).read(), open(switched).read()
    assert "reaction_force" not in a
    assert b.startswith(a) and b[len(a):].startswith("VECTORS reaction_force double\n")
    dim = mesh.dim
    X, r = _reaction_block(switched, dim)
    key = {tuple(np.round(x, 7) + 0.0): k for k, x in enumerate(mesh.coords)}
    idx = np.array([key[tuple(np.round(x, 7) + 0.0)] for x in X])
    nodal = np.zeros((mesh.nnodes, 3))
    nodal[idx] = r  # the same node in neighbouring patches carries the same numbers
    assert np.array_equal(nodal[idx], r)
    con = np.zeros((mesh.nnodes, 3), bool)
    con[:, :dim] = mesh.constrained.reshape(-1, dim)
    assert not nodal[~con].any() and np.abs(nodal[con]).max() > 0
    err = np.abs(nodal.sum(axis=0) - row[1:4]).max() / np.abs(row[1:]).max()
    print("%s: sum of reaction_force against the logged reaction: %.2e of the row's largest entry" % (os.path.basename(str(switched)), err))
    assert err <= 1e-6


def _check_identity(rows, n_free):
    for row in rows:
        reaction, load, inertia, body, mu = row[1:4], row[7:10], row[10:13], row[13:16], row[16]
        gap = np.abs(reaction - (inertia - body - load)).max()
        print("t = %g: |reaction - (inertia - body - load)| %.3e, n_free max_unbalanced %.3e" % (row[0], gap, n_free * mu))
        assert np.isfinite(row).all() and gap <= n_free * mu + 1e-6 * np.abs(row[1:]).max()


def test_reactions_nonlinear_3d(tmp_path):
    name = "block_neo_3d_q2"
    plain = _run(name, "elasticity3d", tmp_path / "off", {})
    assert _run(name, "elasticity3d", tmp_path / "vtk", {"MI_VTK_REACTIONS": "1"}) == plain
    files, stdout = _run_stdout(name, "elasticity3d", tmp_path / "log", {"MI_REACTIONS": "1"})
    assert files == plain
    assert sorted(os.listdir(tmp_path / "log")) == sorted(os.listdir(tmp_path / "off") + ["reactions.log"])
    assert sorted(os.listdir(tmp_path / "vtk")) == sorted(os.listdir(tmp_path / "off"))
    rows = _log(tmp_path / "log")
    assert len(rows) == 2 and np.allclose(rows[:, 0], [0.005, 0.01])
    m = Mi.Mesh(3, 2, (3, 2, 2), (0.0, 0.0, 0.0), (0.3, 0.2, 0.2), [1, 7, 7, 7, 7, 7])
    n_free = int((~m.constrained).sum())
    _check_identity(rows, n_free)
    assert np.abs(rows[:, 1:4]).max() > 0
    # the .vtk of time step 2 (output interval 2) carries the reaction of the second row; the one of the start is at rest
    _check_vtk(tmp_path / "off" / "out" / "solution-001.vtk", tmp_path / "vtk" / "out" / "solution-001.vtk", m, rows[1])
    a, b = open(tmp_path / "off" / "out" / "solution-000.vtk").read(), open(tmp_path / "vtk" / "out" / "solution-000.vtk").read()
    assert b.startswith(a) and b[len(a):].startswith("VECTORS reaction_force double\n")
    assert not _reaction_block(tmp_path / "vtk" / "out" / "solution-000.vtk", 3)[1].any()
    # max_unbalanced against the Newton criterion of each step, from the executable's own table
    prm = open(os.path.join(CASES, name, "parameters.prm")).read()
    tol_f = float(re.search(r"set Tolerance force\s*=\s*(\S+)", prm).group(1))
    steps = stdout.split("CONVERGED!")[:-1]
    assert len(steps) == len(rows)
    for step, row in zip(steps, rows):
        first = re.search(r"\|\s+\d+\s+\S+\s+\S+\s+(\S+)", step)
        res0 = float(first.group(1))
        bound = max(5e-9, tol_f * res0 * 1.001) + 1e-12 * np.abs(row[1:]).max()
        print("t = %g: max_unbalanced %.3e, Newton bound %.3e (first residual %.3e)" % (row[0], row[16], bound, res0))
        assert row[16] <= bound


def test_reactions_linear_2d(tmp_path):
    name = "fsi3_linear_2d_shipped"
    plain = _run(name, "elasticity", tmp_path / "off", {}, interval=2)
    assert _run(name, "elasticity", tmp_path / "on", {"MI_REACTIONS": "1", "MI_VTK_REACTIONS": "1"}, interval=2) == plain
    assert sorted(os.listdir(tmp_path / "on")) == sorted(os.listdir(tmp_path / "off") + ["reactions.log"])
    rows = _log(tmp_path / "on")
    assert len(rows) == 4
    d = O.scenario_desc("FSI3", 2, degree=3)
    m = Mi.Mesh(2, 3, tuple(d.reps)[:2], tuple(d.lo)[:2], tuple(d.hi)[:2], list(d.face_role)[:4])
    _check_identity(rows, int((~m.constrained).sum()))
    assert not rows[:, 13:16].any()  # the linear model's body force is part of its load vector
    assert not rows[:, [3, 4, 5, 9, 12]].any()  # 2D: no z force, no x / y moment
    for k, f in ((1, "solution-001.vtk"), (3, "solution-002.vtk")):
        _check_vtk(tmp_path / "off" / "out" / f, tmp_path / "on" / "out" / f, m, rows[k])


def test_reactions_linear_2d_balance_at_theta_one(tmp_path):
    """the shipped case with `set theta = 1` in its Discretization section: one call is then an equilibrium statement, so every
    row holds max_unbalanced <= abs_tol / dt + 1e-12 sqrt(n_free) (the row's largest entry) -- the bound of test_gpu_reactions.py's
    theta = 1 test with the executable's own tolerance: `Solver type = Direct` passes abs_tol = 1e-14 to mi_linear_step
    (linear_elasticity.cc:241), whose residual norm is then <= abs_tol (0 from the factorisation); the terms' scale is the row's
    largest resultant, the only scale the log carries.  With that the force identity is tight too: a wrong time level, theta weight
    or model argument in the executable's log shows as O(1) of the row."""
    name = "fsi3_linear_2d_shipped"

    def theta_one(prm):
        assert "set theta" not in prm
        return re.sub(r"(subsection Discretization\n)", r"\1  set theta = 1\n", prm, count=1)

    _, stdout = _run_stdout(name, "elasticity", tmp_path / "one", {"MI_REACTIONS": "1"}, edit=theta_one)
    prm = (tmp_path / "one" / "parameters.prm").read_text()
    assert "set theta = 1" in prm and re.search(r"set Solver type\s*=\s*Direct", prm)
    dt = float(re.search(r"set Time step size\s*=\s*(\S+)", prm).group(1))
    rows = _log(tmp_path / "one")
    assert len(rows) == 4
    d = O.scenario_desc("FSI3", 2, degree=3)
    m = Mi.Mesh(2, 3, tuple(d.reps)[:2], tuple(d.lo)[:2], tuple(d.hi)[:2], list(d.face_role)[:4])
    n_free = int((~m.constrained).sum())
    for row in rows:
        largest = np.abs(row[1:]).max()
        bound = 1e-14 / dt + 1e-12 * np.sqrt(n_free) * largest
        print("t = %g: max_unbalanced %.3e, bound %.3e, largest entry %.3e" % (row[0], row[16], bound, largest))
        assert largest > 0 and row[16] <= bound
    _check_identity(rows, n_free)


def test_reactions_on_a_team_are_a_notice(tmp_path):
    """MI_SLABS=2: mi_reactions runs on one slab only, so the executable says so -- once for the log, once per written .vtk file --
    and writes neither the log nor the vector"""
    name = "block_neo_3d_q2"
    files, stdout = _run_stdout(name, "elasticity3d", tmp_path / "two", {"MI_SLABS": "2", "MI_REACTIONS": "1", "MI_VTK_REACTIONS": "1"})
    assert "reactions.log" not in os.listdir(tmp_path / "two")
    vtk = [f for f in files if f.endswith(".vtk")]
    assert vtk and stdout.count("MI_REACTIONS ignored: mi_reactions runs on one slab only") == 1
    assert stdout.count("MI_VTK_REACTIONS: mi_reactions runs on one slab only") == len(vtk)
    for f in vtk:
        assert "reaction_force" not in open(tmp_path / "two" / "out" / f).read()
