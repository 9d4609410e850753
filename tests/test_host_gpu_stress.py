"""GPU: the executables' MI_VTK_STRESS=1 -- nodal stress fields (mi_stress_field) as further point data of the same .vtk files.

The smallest 3D case of the existing VTK test (block_neo_3d_q2 on elasticity3d, neo-Hookean: model 0) and one 2D linear case
(fsi3_linear_2d_shipped on elasticity with an output every second step: model 1).  The file is parsed, the nodal u rebuilt from
its `displacement` point data, and stress_* / von_mises compared with tests/golden/stress_reference.py of THAT u at the gate
test_host_gpu.py applies to the strain values it reads back from a file: 1e-6 of the largest value (the file carries 12
significant digits of u and of the stress; both bound the comparison).  Patch points that are the same node of neighbouring cells
carry identical strings (nodal values, continuous across cells -- unlike strain_*).  Without the switch: no such array, and the
file is the switched file up to its first stress array.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import stress_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dealii-adapter_amd", "host")
CASES = os.path.join(ROOT, "tests", "cases")


def _run(name, exe, d, env, interval=None):
    d.mkdir()
    prm = open(os.path.join(CASES, name, "parameters.prm")).read()
    if interval is not None:
        prm = re.sub(r"set Output interval\s*=\s*\d+", "set Output interval       = %d" % interval, prm)
    (d / "parameters.prm").write_text(prm)
    (d / "precice-config.xml").write_text(open(os.path.join(CASES, name, "precice-config.xml")).read())
    out = subprocess.run([os.path.join(HOST, exe)], cwd=d, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return sorted(os.listdir(d / "out"))


def _parse(path, dim):
    txt = open(path).read().split("\n")
    i = next(k for k, l in enumerate(txt) if l.startswith("POINTS"))
    npts = int(txt[i].split()[1])
    pts = np.array([l.split() for l in txt[i + 1:i + 1 + npts]], dtype=float)[:, :dim]
    j = next(k for k, l in enumerate(txt) if l.startswith("VECTORS displacement"))
    disp = np.array([l.split() for l in txt[j + 1:j + 1 + npts]], dtype=float)[:, :dim]
    fields = {l.split()[1]: txt[k + 2:k + 2 + npts] for k, l in enumerate(txt)
              if l.startswith("SCALARS stress_") or l.startswith("SCALARS von_mises")}
    return pts, disp, fields


def _check(path, mesh, mu, nu, model):
    dim = mesh.dim
    pts, disp, fields = _parse(path, dim)
    names = ["stress_" + "xyz"[d] + "xyz"[e] for d, e in S.PAIRS[dim]]
    assert sorted(fields) == sorted(names + ["von_mises"])
    key = {tuple(np.round(x, 7) + 0.0): k for k, x in enumerate(mesh.coords)}
    idx = np.array([key[tuple(np.round(x, 7) + 0.0)] for x in pts - disp])
    assert len(set(idx)) == mesh.nnodes
    # the same node in neighbouring patches: the same strings, in every array
    for name, col in fields.items():
        seen = {}
        for node, s in zip(idx, col):
            assert seen.setdefault(node, s) == s, (name, node)
    u = np.zeros((mesh.nnodes, dim))
    u[idx] = disp
    assert np.abs(u).max() > 0
    sigma, vm, _, det = S.nodal_stress(mesh, u.reshape(-1), mu, nu, model)
    assert det > 0.4
    got = np.array([np.array(fields[n], dtype=float) for n in names]).T
    scale = np.abs(sigma).max()
    worst = np.abs(got - sigma[idx]).max() / scale
    worst_vm = np.abs(np.array(fields["von_mises"], dtype=float) - vm[idx]).max() / scale
    print("%s: stress %.2e, von Mises %.2e of max|sigma| = %.3e" % (os.path.basename(str(path)), worst, worst_vm, scale))
    assert scale > 0 and worst < 1e-6 and worst_vm < 1e-6


def _check_unswitched(plain, switched):
    a, b = open(plain).read(), open(switched).read()
    assert not any(l.startswith("SCALARS stress_") or l.startswith("SCALARS von_mises") for l in a.split("\n"))
    assert b.startswith(a) and b[len(a):].startswith("SCALARS stress_xx ")


def test_vtk_stress_nonlinear_3d(tmp_path):
    name = "block_neo_3d_q2"
    files = _run(name, "elasticity3d", tmp_path / "on", {"MI_VTK_STRESS": "1"})
    assert files == _run(name, "elasticity3d", tmp_path / "off", {})  # no extra file
    m = Mi.Mesh(3, 2, (3, 2, 2), (0.0, 0.0, 0.0), (0.3, 0.2, 0.2), [0] * 6)
    _check(tmp_path / "on" / "out" / "solution-001.vtk", m, 0.5e6, 0.4, S.NEOHOOKE)
    for f in ("solution-000.vtk", "solution-001.vtk"):
        _check_unswitched(tmp_path / "off" / "out" / f, tmp_path / "on" / "out" / f)
    pts, disp, fields = _parse(tmp_path / "on" / "out" / "solution-000.vtk", 3)
    assert np.all(disp == 0) and all(float(v) == 0 for col in fields.values() for v in col)  # the state at rest


def test_vtk_stress_on_an_rccl_team_is_a_notice(tmp_path):
    """four rank threads through the library's RCCL branch (against the RCCL test double, as test_host_gpu.py runs them):
    mi_stress_field is refused there, so the executable says so in one line per written file and writes no stress array"""
    frccl = os.path.join(ROOT, "tests", "fake_rccl")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-adapter_amd"), "-j4", "all"])
    subprocess.check_call(["make", "-C", frccl, "libmi_elasticity_fakerccl.so", "ranks"])
    name = "fsi3_neo_3d_q3"
    for f in ("parameters.prm", "precice-config.xml"):
        (tmp_path / f).write_text(open(os.path.join(CASES, name, f)).read())
    r = subprocess.run([os.path.join(frccl, "elasticity_ranks3d"), "4"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MI_VTK_STRESS="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vtk = sorted(f for f in os.listdir(tmp_path / "out") if f.endswith(".vtk"))
    assert vtk and r.stdout.count("MI_VTK_STRESS: mi_stress_field runs in one process only") == len(vtk)
    for f in vtk:
        assert "SCALARS stress_" not in open(tmp_path / "out" / f).read() and "SCALARS von_mises" not in open(tmp_path / "out" / f).read()


def test_vtk_stress_linear_2d(tmp_path):
    name = "fsi3_linear_2d_shipped"
    files = _run(name, "elasticity", tmp_path / "on", {"MI_VTK_STRESS": "1"}, interval=2)
    assert files == _run(name, "elasticity", tmp_path / "off", {}, interval=2)
    d = O.scenario_desc("FSI3", 2, degree=3)
    m = Mi.Mesh(2, 3, tuple(d.reps)[:2], tuple(d.lo)[:2], tuple(d.hi)[:2], [0] * 4)
    _check(tmp_path / "on" / "out" / "solution-002.vtk", m, 0.5e6, 0.4, S.LINEAR)
    _check_unswitched(tmp_path / "off" / "out" / "solution-002.vtk", tmp_path / "on" / "out" / "solution-002.vtk")
