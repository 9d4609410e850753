"""GPU: the executables' MI_PROBES_STRESS=raw|recovered -- the stress (mi_evaluate_stress) of every probe of MI_PROBES behind its
displacement and velocity in probes.log -- and MI_VTK_PRINCIPAL=1, the principal values of the nodal stress (mi_principal_stress)
as point data `principal_stress` of the .vtk files.  In the pattern of test_host_gpu_probes.py and test_host_gpu_stress.py.

Cases: fsi3_neo_2d_implicit on elasticity (Solid<2>, Q1: model 0) and fsi3_linear_3d_shipped on elasticity3d (ElastoDynamics<3>,
Q3: model 1), each with an output at the last step; probes: a cell centre, an off-centre point and an interface node.  A row is
1 + npts (2 dim + ncomp + 1) numbers.  The displacement and velocity columns are, string for string, those of a run with MI_PROBES
alone, whose probes.log has the header and the width it always had.  The stress columns of the last row equal
Context.evaluate_stress on the final state rebuilt from the last .vtk file to 1e-6 of max|sigma|: test_host_gpu_stress.py's gate
for a stress computed from a state read back from a file (12 significant digits of u).  principal_stress: descending, and the
eigenvalues of the tensor the same file's stress_* arrays hold to 1e-10 of max|sigma| (12 digits of either).
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_pkg
from test_host_gpu import CASES, HOST
from test_host_gpu_probes import HI, LO, REPS, ROLES, _rows
from test_host_gpu_stress import _parse, _run

M = load_pkg()
pytestmark = pytest.mark.gpu

MU, NU = 0.5e6, 0.4  # both cases' parameters.prm


def _check(name, exe, dim, degree, windows, model, tmp_path):
    G = M.Context(dim=dim, degree=degree, reps=REPS[:dim], lo=LO[:dim], hi=HI[:dim], face_role=ROLES[dim], mu=MU, nu=NU)
    _, xyz = G.interface()
    h = (np.array(HI) - np.array(LO)) / np.array(REPS)
    centre = (np.array(LO) + h * (np.array([7, 1, 0]) + 0.5))[:dim]  # the centre of cell (7, 1[, 0])
    off = (np.array(LO) + h * (np.array([2, 0, 0]) + np.array([0.31, 0.77, 0.4])))[:dim]
    pts = np.vstack([centre, off, xyz[len(xyz) // 2]])
    npts, ncomp = len(pts), dim * (dim + 1) // 2
    probe_file = tmp_path / "probes.txt"
    probe_file.write_text("".join(" ".join("%.17g" % v for v in x) + "\n" for x in pts))
    _run(name, exe, tmp_path / "plain", {"MI_PROBES": str(probe_file)}, interval=windows)
    plain_lines = open(tmp_path / "plain" / "probes.log").read().split("\n")
    assert plain_lines[0] == ("# t, then displacement and velocity (%d numbers each) of each of %d probes of %s, per completed time window"
                              % (dim, npts, probe_file))
    plain = [l.split() for l in plain_lines[1:] if l]
    assert len(plain) == windows and all(len(r) == 1 + 2 * dim * npts for r in plain)
    # the final state, rebuilt from the last file
    vtk_pts, vtk_disp, _ = _parse(tmp_path / "plain" / "out" / "solution-001.vtk", dim)
    key = {tuple(np.round(x, 7) + 0.0): k for k, x in enumerate(G.coords)}
    idx = np.array([key[tuple(np.round(x, 7) + 0.0)] for x in vtk_pts - vtk_disp])
    state = np.zeros((G.nnodes, dim))
    state[idx] = vtk_disp
    G.set(M.V_U, state.reshape(-1))
    smax = np.abs(G.stress_field(model)[0]).max()
    assert smax > 0
    for kind, word in ((M.STRESS_AT_RAW, "raw"), (M.STRESS_AT_RECOVERED, "recovered")):
        d = tmp_path / word
        _run(name, exe, d, {"MI_PROBES": str(probe_file), "MI_PROBES_STRESS": word}, interval=windows)
        lines = open(d / "probes.log").read().split("\n")
        assert lines[0].startswith("# t, then displacement and velocity") and word + " stress of model %d" % model in lines[0]
        rows = [l.split() for l in lines[1:] if l]
        per = 2 * dim + ncomp + 1
        assert len(rows) == windows and all(len(r) == 1 + per * npts for r in rows)
        for r, p in zip(rows, plain):  # t, u and v: the strings of the run without the variable
            assert r[0] == p[0]
            for k in range(npts):
                assert r[1 + per * k:1 + per * k + 2 * dim] == p[1 + 2 * dim * k:1 + 2 * dim * (k + 1)], k
        # every other file of the run: byte for byte
        for f in sorted(os.listdir(d / "out")):
            assert open(d / "out" / f, "rb").read() == open(tmp_path / "plain" / "out" / f, "rb").read(), f
        last = np.array(rows[-1][1:], dtype=float).reshape(npts, per)
        want = G.evaluate_stress(pts, model=model, kind=kind)
        es = np.abs(last[:, 2 * dim:2 * dim + ncomp] - want["sigma"]).max() / smax
        ev = np.abs(last[:, -1] - want["von_mises"]).max() / smax
        print("%s %s: stress %.2e, von Mises %.2e of max|sigma| = %.3e" % (name, word, es, ev, smax))
        assert want["n_outside"] == 0 and np.abs(want["sigma"]).max() > 0
        assert es < 1e-6 and ev < 1e-6
    G.close()


def test_stress_probes_nonlinear_2d(tmp_path):
    _check("fsi3_neo_2d_implicit", "elasticity", 2, 1, 2, M.STRESS_NEOHOOKE, tmp_path)


def test_stress_probes_linear_3d(tmp_path):
    _check("fsi3_linear_3d_shipped", "elasticity3d", 3, 3, 4, M.STRESS_LINEAR, tmp_path)


def test_bad_value_ends_the_run(tmp_path):
    name = "fsi3_neo_2d_implicit"
    for f in ("parameters.prm", "precice-config.xml"):
        (tmp_path / f).write_text(open(os.path.join(CASES, name, f)).read())
    (tmp_path / "probes.txt").write_text("0.3 0.2\n")
    out = subprocess.run([os.path.join(HOST, "elasticity")], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, MI_PROBES=str(tmp_path / "probes.txt"), MI_PROBES_STRESS="nodal"))
    assert out.returncode != 0
    assert "MI_PROBES_STRESS: 'nodal' is neither raw nor recovered" in out.stderr
    assert not os.path.exists(tmp_path / "probes.log")


def _principal(path, dim):
    txt = open(path).read().split("\n")
    npts = int(next(l for l in txt if l.startswith("POINTS")).split()[1])
    k = txt.index("SCALARS principal_stress double %d" % dim)
    assert txt[k + 1] == "LOOKUP_TABLE default"
    return txt[k + 2:k + 2 + npts]


def test_vtk_principal_stress_3d(tmp_path):
    name, dim = "block_neo_3d_q2", 3
    files = _run(name, "elasticity3d", tmp_path / "both", {"MI_VTK_STRESS": "1", "MI_VTK_PRINCIPAL": "1"})
    assert files == _run(name, "elasticity3d", tmp_path / "stress", {"MI_VTK_STRESS": "1"})
    assert files == _run(name, "elasticity3d", tmp_path / "alone", {"MI_VTK_PRINCIPAL": "1"})
    assert files == _run(name, "elasticity3d", tmp_path / "off", {})
    for f in files:
        both, stress = open(tmp_path / "both" / "out" / f).read(), open(tmp_path / "stress" / "out" / f).read()
        alone, off = open(tmp_path / "alone" / "out" / f).read(), open(tmp_path / "off" / "out" / f).read()
        if not f.endswith(".vtk"):  # (the step log beside them)
            assert both == stress == alone == off
            continue
        assert "principal_stress" not in stress and "principal_stress" not in off  # without the variable: what it was
        assert both.startswith(stress) and both[len(stress):].startswith("SCALARS principal_stress double 3\nLOOKUP_TABLE default\n")
        assert alone.startswith(off) and alone[len(off):] == both[len(stress):]  # the field is computed for this alone
    path = tmp_path / "both" / "out" / "solution-001.vtk"
    _, _, fields = _parse(path, dim)
    lam = np.array([l.split() for l in _principal(path, dim)], dtype=float)
    sig = np.array([np.array(fields["stress_" + c], dtype=float) for c in ("xx", "yy", "zz", "xy", "xz", "yz")]).T
    assert lam.shape == (len(sig), 3) and np.all(lam[:, 0] >= lam[:, 1]) and np.all(lam[:, 1] >= lam[:, 2])
    full = np.zeros((len(sig), 3, 3))
    for k, (d, e) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
        full[:, d, e] = full[:, e, d] = sig[:, k]
    err = np.abs(lam - np.linalg.eigvalsh(full)[:, ::-1]).max() / np.abs(sig).max()
    print("principal_stress against the eigenvalues of the file's stress arrays: %.2e of max|sigma| = %.3e" % (err, np.abs(sig).max()))
    assert np.abs(sig).max() > 0 and err < 1e-10
