"""GPU: the executables' MI_VTK_STRESS_ERROR=1 and MI_STRESS_ERROR=1 -- the stress error indicator (mi_stress_error) as CELL_DATA
`stress_error` of the .vtk files and as four further keys of every line of steps.jsonl.

The cases of test_host_gpu_stress.py: block_neo_3d_q2 on elasticity3d (neo-Hookean: model 0) and fsi3_linear_2d_shipped on
elasticity with an output every second step (model 1).  The file is parsed, the nodal u rebuilt from its `displacement` point
data, and the cell array compared with tests/golden/stress_error_reference.py of THAT u at the gate test_host_gpu_stress.py
applies to what it reads back from a file: 1e-6 of the largest value, here of the largest sqrt(eta_K^2 + n_K^2) (the file
carries 12 significant digits of u).  With MI_VTK_LINEAR_CELLS every sub-cell carries its element's string.  The step log's
keys of the step the file belongs to are held to the same reference.  Without the switches: the file is the switched file up
to `CELL_DATA`, and a line of the log is the switched line up to its first new key.
"""
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_host_gpu_stress import _run

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import stress_error_reference as R  # noqa: E402
import stress_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_KEYS = ["stress_error", "stress_norm", "stress_error_relative", "stress_error_max_cell"]


def _parse(path, dim):
    txt = open(path).read().split("\n")
    i = next(k for k, l in enumerate(txt) if l.startswith("POINTS"))
    npts = int(txt[i].split()[1])
    pts = np.array([l.split() for l in txt[i + 1:i + 1 + npts]], dtype=float)[:, :dim]
    j = next(k for k, l in enumerate(txt) if l.startswith("VECTORS displacement"))
    disp = np.array([l.split() for l in txt[j + 1:j + 1 + npts]], dtype=float)[:, :dim]
    ncell_records = int(next(l for l in txt if l.startswith("CELLS")).split()[1])
    c = [k for k, l in enumerate(txt) if l.startswith("CELL_DATA")]
    assert len(c) == 1 and txt[c[0] + 1] == "SCALARS stress_error double 1" and txt[c[0] + 2] == "LOOKUP_TABLE default"
    n = int(txt[c[0]].split()[1])
    assert n == ncell_records
    col = txt[c[0] + 3:c[0] + 3 + n]
    assert txt[c[0] + 3 + n:] == [""]  # the array ends the file
    return pts, disp, col


def _reference(path, mesh, mu, nu, model):
    dim = mesh.dim
    pts, disp, col = _parse(path, dim)
    key = {tuple(np.round(x, 7) + 0.0): k for k, x in enumerate(mesh.coords)}
    idx = np.array([key[tuple(np.round(x, 7) + 0.0)] for x in pts - disp])
    assert len(set(idx)) == mesh.nnodes
    u = np.zeros((mesh.nnodes, dim))
    u[idx] = disp
    assert np.abs(u).max() > 0
    return col, R.stress_error(mesh, u.reshape(-1), mu, nu, model)


def _check_cells(col, ref, per_cell, what):
    ncells = len(ref["eta_cell"])
    assert len(col) == ncells * per_cell
    for c in range(ncells):  # every sub-cell of an element: the element's string
        assert len(set(col[c * per_cell:(c + 1) * per_cell])) == 1, c
    got = np.array(col[::per_cell], dtype=float)
    scale = np.sqrt(ref["eta2_cell"] + ref["n2_cell"]).max()
    worst = np.abs(got - ref["eta_cell"]).max() / scale
    print("%s: eta_K %.2e of the largest sqrt(eta_K^2 + n_K^2) = %.3e; eta_K in [%.3e, %.3e]" % (
        what, worst, scale, ref["eta_cell"].min(), ref["eta_cell"].max()))
    assert scale > 0 and worst < 1e-6
    assert int(np.argmax(got)) == ref["max_cell"]


def _check_unswitched(plain, switched):
    a, b = open(plain).read(), open(switched).read()
    assert "CELL_DATA" not in a and "stress_error" not in a
    assert b.startswith(a) and b[len(a):].startswith("CELL_DATA ")


def test_vtk_and_step_log_nonlinear_3d(tmp_path):
    name, on = "block_neo_3d_q2", {"MI_VTK_STRESS_ERROR": "1", "MI_STRESS_ERROR": "1"}
    files = _run(name, "elasticity3d", tmp_path / "on", on)
    assert files == _run(name, "elasticity3d", tmp_path / "off", {})  # no extra file
    _run(name, "elasticity3d", tmp_path / "lin", dict(on, MI_VTK_LINEAR_CELLS="1"))
    m = Mi.Mesh(3, 2, (3, 2, 2), (0.0, 0.0, 0.0), (0.3, 0.2, 0.2), [0] * 6)
    col, ref = _reference(tmp_path / "on" / "out" / "solution-001.vtk", m, 0.5e6, 0.4, S.NEOHOOKE)
    _check_cells(col, ref, 1, "Lagrange cells")
    col_lin, _ = _reference(tmp_path / "lin" / "out" / "solution-001.vtk", m, 0.5e6, 0.4, S.NEOHOOKE)
    _check_cells(col_lin, ref, 8, "linear sub-cells")
    assert col_lin[::8] == col
    for f in ("solution-000.vtk", "solution-001.vtk"):
        _check_unswitched(tmp_path / "off" / "out" / f, tmp_path / "on" / "out" / f)
    assert all(float(v) == 0 for v in _parse(tmp_path / "on" / "out" / "solution-000.vtk", 3)[2])  # the state at rest
    # the step log: the line of the step solution-001 belongs to (output interval 2) against the same reference
    lines_on, lines_off = (open(tmp_path / d / "out" / "steps.jsonl").read().split("\n") for d in ("on", "off"))
    assert len(lines_on) == len(lines_off) > 2
    for a, b in zip(lines_on, lines_off):
        if b:
            assert not any(k in b for k in NEW_KEYS) and b.endswith("}")
            assert a.startswith(b[:-1] + ', "stress_error": ') and sorted(set(json.loads(a)) - set(json.loads(b))) == sorted(NEW_KEYS)
    step = next(s for s in map(json.loads, filter(None, lines_on)) if s["timestep"] == 2)
    tot = np.sqrt(ref["error"] ** 2 + ref["norm"] ** 2)
    print("step log: eta %.6e (ref %.6e) n %.6e (ref %.6e) relative %.6e max_cell %d" % (
        step["stress_error"], ref["error"], step["stress_norm"], ref["norm"], step["stress_error_relative"], step["stress_error_max_cell"]))
    assert abs(step["stress_error"] - ref["error"]) < 1e-6 * tot and abs(step["stress_norm"] - ref["norm"]) < 1e-6 * tot
    assert abs(step["stress_error_relative"] - ref["relative"]) < 1e-6
    assert step["stress_error_max_cell"] == ref["max_cell"]


def test_vtk_linear_2d(tmp_path):
    name, on = "fsi3_linear_2d_shipped", {"MI_VTK_STRESS_ERROR": "1", "MI_VTK_LINEAR_CELLS": "1"}
    files = _run(name, "elasticity", tmp_path / "lin", on, interval=2)
    assert files == _run(name, "elasticity", tmp_path / "off", {"MI_VTK_LINEAR_CELLS": "1"}, interval=2)
    _run(name, "elasticity", tmp_path / "on", {"MI_VTK_STRESS_ERROR": "1"}, interval=2)
    d = O.scenario_desc("FSI3", 2, degree=3)
    m = Mi.Mesh(2, 3, tuple(d.reps)[:2], tuple(d.lo)[:2], tuple(d.hi)[:2], [0] * 4)
    col, ref = _reference(tmp_path / "on" / "out" / "solution-002.vtk", m, 0.5e6, 0.4, S.LINEAR)
    _check_cells(col, ref, 1, "Lagrange cells")
    col_lin, _ = _reference(tmp_path / "lin" / "out" / "solution-002.vtk", m, 0.5e6, 0.4, S.LINEAR)
    _check_cells(col_lin, ref, 9, "linear sub-cells")
    assert col_lin[::9] == col
    _check_unswitched(tmp_path / "off" / "out" / "solution-002.vtk", tmp_path / "lin" / "out" / "solution-002.vtk")
