"""GPU: mi::Device::project_state (host/include/mi/device_vector.h) through the device case of host/test_host.cc, built as
test_host_device: six quadratic fields on a 4 x 2 x 4 Q2 box projected onto the same box in 2 x 1 x 2 cells with sub = 2 come
back as themselves (both spaces hold them, the pair is exact), the integral of |w|^2 is kept, a bad sub is refused."""
import os
import subprocess

import pytest

from conftest import load_pkg

M = load_pkg()
pytestmark = pytest.mark.gpu

HOST = os.path.join(M.PKG_DIR, "host")


def test_device_project_state(tmp_path):
    exe = os.path.join(HOST, "test_host_device")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_host_device"])
    out = subprocess.run([exe, "project"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "HOST DEVICE TESTS OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("vector ") == 6
