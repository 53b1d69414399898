"""CPU: AddressSanitizer + UBSan run of the Poisson header's host build (tests/stub/poisson_capi.cpp with its driver):
depths 1-5 on a small cloud with spoilt rows, then 0, 1 and 2 samples.  Host code only: sanitizers do not run on the GPU."""
import os
import struct
import subprocess

import numpy as np

from tests.test_poisson_cpu import STUB, sphere_cloud


def test_poisson_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "poisson_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DPOISSON_MAIN", "-o", exe, STUB])
    xyz, nrm = sphere_cloud(3000, 9)
    xyz[3] = [np.nan, 0, 0]
    xyz[4] = xyz[5]
    nrm[7] = 0
    nrm[8, 1] = np.inf
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(xyz)))
        f.write(xyz.astype("<f4").tobytes())
        f.write(nrm.astype("<f4").tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("depth 1: ")
    assert "n 0: 0 vertices 0 triangles" in r.stdout
