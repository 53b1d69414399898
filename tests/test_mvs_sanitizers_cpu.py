"""CPU: AddressSanitizer + UBSan run of the stereo header's host build (tests/stub/mvs_capi.cpp with its driver): the
five-view scene with colour at levels 0 and 1 and windows 1, 3 and 7, then one source, n_best above the sources, an odd
size through the pyramid and a black view.  Host code only: sanitizers do not run on the GPU."""
import os
import struct
import subprocess

import numpy as np

from tests.test_mvs_cpu import DMAX, DMIN, STUB, scene


def test_mvs_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mvs_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DMVS_MAIN", "-o", exe, STUB])
    gray, depth, K, P = scene("sphere")
    gray = gray[:, :45, :71]
    bgr = np.stack([gray, 255 - gray, gray // 2], -1)
    n, rows, cols = gray.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", n, rows, cols, 1))
        f.write(np.concatenate([K.ravel(), P.ravel(), np.full(n, DMIN), np.full(n, DMAX)]).astype("<f8").tobytes())
        f.write(np.ascontiguousarray(gray).tobytes())
        f.write(np.ascontiguousarray(bgr).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("level 0 window 1: ")
    assert "starved: 0 points" in r.stdout and "one source: " in r.stdout
