"""GPU: the `elasticity3d` executable on a 3D Q2 linear case, assembled and with MI_LINEAR_OPERATOR=2 (the tuning key
"linear_operator" 2: mf_linear_q2).  The case is the shipped 3D linear case with `Polynomial degree = 2`, written into the
test's own directory."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_host_gpu import CASES, HOST, _check_rows

pytestmark = pytest.mark.gpu

SHIPPED = "fsi3_linear_3d_shipped"


def _run_q2(tmp_path, env=None):
    prm = open(os.path.join(CASES, SHIPPED, "parameters.prm")).read()
    prm, n = re.subn(r"(set\s+Polynomial degree\s*=\s*)\d+", r"\g<1>2", prm)
    assert n == 1
    (tmp_path / "parameters.prm").write_text(prm)
    (tmp_path / "precice-config.xml").write_text(open(os.path.join(CASES, SHIPPED, "precice-config.xml")).read())
    out = subprocess.run([os.path.join(HOST, "elasticity3d")], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **env) if env else None)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    rows = [np.array(l.split(), dtype=float) for l in open(tmp_path / "displacement.log") if not l.startswith("#")]
    return out.stdout, rows


def test_executable_matrix_free_linear_operators_q2(tmp_path):
    """plain and with MI_LINEAR_OPERATOR=2: the same output rows, the second log names mf_linear_q2, nothing is ignored"""
    (tmp_path / "asm").mkdir()
    (tmp_path / "mf").mkdir()
    out0, rows0 = _run_q2(tmp_path / "asm")
    out2, rows2 = _run_q2(tmp_path / "mf", env={"MI_LINEAR_OPERATOR": "2"})
    assert "Linear operators: matrix-free" in out2 and "mf_linear_q2" in out2
    assert "MI_LINEAR_OPERATOR ignored" not in out0 + out2
    assert "matrix-free" not in out0
    assert len(rows0) >= 3
    _check_rows(rows2, [(r[0], r[1:].reshape(-1, 3)) for r in rows0], 3)
