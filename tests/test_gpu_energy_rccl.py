"""GPU: mi_energy through the library's RCCL branch (rank threads against the RCCL test double, as test_gpu_fake_rccl.py):
two ranks on Q2 2 x 2 x 4, every rank reports the same numbers, equal to the undecomposed context's to 1e-13 (the slabs'
sums are added in another order).  The emulated-team cases of test_gpu_energy.py cover which cells a slab owns; here only
the all-reduce call differs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl")
pytestmark = pytest.mark.gpu


def test_energy_through_the_rccl_branch():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-adapter_amd"), "-j4", "all"])
    subprocess.check_call(["make", "-C", FAKE])
    out = subprocess.run([sys.executable, os.path.join(FAKE, "run_ranks_energy.py"), "2", "3", "2", "2,2,4"], capture_output=True,
                         text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and lines, (out.stdout[-2000:], out.stderr[-3000:])
    r = json.loads(lines[-1])
    assert r["ok"], r
    assert r["ranks"][0] == r["ranks"][1]
    ref = r["single"]
    assert ref[0] > 0 and ref[1] > 0
    for k, scale in enumerate((ref[0], ref[1], r["body_scale"])):
        assert abs(r["ranks"][0][k] - ref[k]) <= 1e-13 * scale, (k, r)
