"""GPU: the executables' MI_PROBES=<file> -- displacement and velocity at arbitrary points (mi_evaluate_points) as one row of
probes.log per completed time window, beside displacement.log.

Cases: fsi3_neo_2d_implicit on elasticity (Solid<2>, Q1, three coupling iterations per window: a row is written for the converged
iteration only) and fsi3_linear_3d_shipped on elasticity3d (ElastoDynamics<3>, Q3), each with an output at the last step.  The
probe file lists the interface nodes' coordinates and one cell centre.  The u columns at the interface points are the rows of
displacement.log to 1e-12 of the largest entry (the finite-element field at a node is the nodal value); the cell centre equals
Context.evaluate on the final state rebuilt from the last .vtk file to 1e-9 of the largest displacement (the file carries 12
significant digits).  Without the variable every file is byte for byte that of a plain run and no probes.log exists; a probe
outside the mesh ends the run with a message that names the point.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_pkg
from test_host_gpu import CASES, HOST
from test_host_gpu_stress import _parse, _run

M = load_pkg()
pytestmark = pytest.mark.gpu

LO, HI, REPS = (0.24899, 0.19, -0.005), (0.6, 0.21, 0.005), (18, 3, 1)  # the FSI3 flap of both models
ROLES = {2: [M.FACE_CLAMPED, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_INTERFACE, 0, 0],
         3: [M.FACE_CLAMPED, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_INTERFACE, M.FACE_ZCLAMP, M.FACE_ZCLAMP]}


def _files(d):
    out = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(d / f)}
    for f in sorted(os.listdir(d / "out")):
        out["out/" + f] = open(d / "out" / f, "rb").read()
    return out


def _rows(path):
    return np.array([l.split() for l in open(path) if not l.startswith("#")], dtype=float)


def _check(name, exe, dim, degree, windows, tmp_path):
    G = M.Context(dim=dim, degree=degree, reps=REPS[:dim], lo=LO[:dim], hi=HI[:dim], face_role=ROLES[dim])
    _, xyz = G.interface()
    h = (np.array(HI) - np.array(LO)) / np.array(REPS)
    centre = (np.array(LO) + h * (np.array([7, 1, 0]) + 0.5))[:dim]  # the centre of cell (7, 1[, 0])
    pts = np.vstack([xyz, centre])
    probe_file = tmp_path / "probes.txt"
    probe_file.write_text("# interface nodes, then a cell centre\n\n" + "".join(" ".join("%.17g" % v for v in x) + "\n" for x in pts))
    _run(name, exe, tmp_path / "on", {"MI_PROBES": str(probe_file)}, interval=windows)
    _run(name, exe, tmp_path / "off", {}, interval=windows)
    # without the variable: the same files, byte for byte, and no probes.log
    f_on, f_off = _files(tmp_path / "on"), _files(tmp_path / "off")
    assert "probes.log" in f_on and "probes.log" not in f_off
    del f_on["probes.log"]
    assert sorted(f_on) == sorted(f_off)
    for f in f_off:
        assert f_on[f] == f_off[f], f
    # the u columns at the interface nodes: the rows of displacement.log
    probes, disp = _rows(tmp_path / "on" / "probes.log"), _rows(tmp_path / "on" / "displacement.log")
    npts = len(pts)
    assert probes.shape == (windows, 1 + 2 * dim * npts) and disp.shape == (windows, 1 + dim * len(xyz))
    assert np.abs(probes[:, 0] - disp[:, 0]).max() < 1e-12
    per = probes[:, 1:].reshape(windows, npts, 2, dim)
    u, v = per[:, :, 0, :], per[:, :, 1, :]
    scale = np.abs(disp[:, 1:]).max()
    err = np.abs(u[:, :-1, :].reshape(windows, -1) - disp[:, 1:]).max() / scale
    print("%s: u at the interface nodes against displacement.log %.2e (largest entry %.3e)" % (name, err, scale))
    assert scale > 0 and err < 1e-12
    assert np.all(np.isfinite(v)) and np.abs(v).max() > 0
    # the cell centre: Context.evaluate on the final state, rebuilt from the last file
    vtk_pts, vtk_disp, _ = _parse(tmp_path / "on" / "out" / "solution-001.vtk", dim)
    coords = G.coords
    key = {tuple(np.round(x, 7) + 0.0): k for k, x in enumerate(coords)}
    idx = np.array([key[tuple(np.round(x, 7) + 0.0)] for x in vtk_pts - vtk_disp])
    assert len(set(idx)) == G.nnodes
    state = np.zeros((G.nnodes, dim))
    state[idx] = vtk_disp
    G.set(M.V_U, state.reshape(-1))
    want, _, cell, nout = G.evaluate(M.V_U, centre[None, :])
    err = np.abs(u[-1, -1] - want[0]).max() / np.abs(state).max()
    print("%s: u at the cell centre %s against Context.evaluate on the final state %.2e" % (name, u[-1, -1], err))
    assert nout == 0 and cell[0] == 7 + 18 * 1 and err < 1e-9
    if degree == 1 and dim == 2:  # a Q1 value lies between its cell's nodal extremes
        corners = state[[7 + 19 * 1, 8 + 19 * 1, 7 + 19 * 2, 8 + 19 * 2]]
        assert np.all(u[-1, -1] >= corners.min(axis=0) - 1e-12) and np.all(u[-1, -1] <= corners.max(axis=0) + 1e-12)
    G.close()


def test_probe_log_nonlinear_2d(tmp_path):
    _check("fsi3_neo_2d_implicit", "elasticity", 2, 1, 2, tmp_path)


def test_probe_log_linear_3d(tmp_path):
    _check("fsi3_linear_3d_shipped", "elasticity3d", 3, 3, 4, tmp_path)


def test_probe_outside_the_mesh_ends_the_run(tmp_path):
    name = "fsi3_neo_2d_implicit"
    for f in ("parameters.prm", "precice-config.xml"):
        (tmp_path / f).write_text(open(os.path.join(CASES, name, f)).read())
    (tmp_path / "probes.txt").write_text("0.3 0.2\n0.7 0.2\n")
    out = subprocess.run([os.path.join(HOST, "elasticity")], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, MI_PROBES=str(tmp_path / "probes.txt")))
    assert out.returncode != 0
    assert "MI_PROBES: probe 2 of" in out.stderr and "(0.69999999999999996, 0.20000000000000001) lies outside the mesh" in out.stderr
    assert not os.path.exists(tmp_path / "probes.log")
