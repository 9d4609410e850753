"""GPU: the executable's switch MI_LINEAR_PRECOND=1 (handed on as the tuning key "linear_precond") on the shipped 3D linear case.

The case is 3D Q3 with "Solver type = Direct"; MI_LINEAR_OPERATOR=1 takes both runs to the PCG route (nothing to factorise), so
the run without the switch is the Jacobi-PCG and the run with it the multigrid-PCG, on the same matrix-free operators."""
import re

import numpy as np
import pytest

from test_host_gpu import _run_case

pytestmark = pytest.mark.gpu


def _iterations(stdout):
    return [int(v) for v in re.findall(r"No of iterations:\s+(\d+)", stdout)]


def test_executable_multigrid_preconditioned_linear_model(tmp_path):
    name = "fsi3_linear_3d_shipped"
    (tmp_path / "jacobi").mkdir()
    (tmp_path / "mg").mkdir()
    out0, rows0 = _run_case(name, "elasticity3d", tmp_path / "jacobi", env={"MI_LINEAR_OPERATOR": "1"})
    out1, rows1 = _run_case(name, "elasticity3d", tmp_path / "mg", env={"MI_LINEAR_OPERATOR": "1", "MI_LINEAR_PRECOND": "1"})
    assert "Linear operators: matrix-free" in out0 and "Linear operators: matrix-free" in out1
    assert "multigrid V-cycle" in out1 and "MI_LINEAR_PRECOND ignored" not in out1
    assert "multigrid V-cycle" not in out0
    assert len(rows0) == len(rows1) >= 3
    for a, b in zip(rows0, rows1):
        assert abs(a[0] - b[0]) < 1e-12
        assert np.abs(a[1:] - b[1:]).max() <= 1e-7 * np.abs(a[1:]).max()
    its0, its1 = _iterations(out0), _iterations(out1)
    print("CG iterations per step: Jacobi %s, multigrid %s" % (its0, its1))
    assert len(its0) == len(its1) >= 3 and all(i > 1 for i in its1)
    assert sum(its1) < sum(its0)
