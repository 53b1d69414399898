"""CPU: AddressSanitizer + UBSan run of the dendrometry header's host build (tests/stub/dendro_capi.cpp with its driver): a
planted tree with NaN points and a second label through five option sets, an empty selection, the refusals, and hand-made
slices of 0 .. 1025 points (rings, collinear, identical).  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_dendro_cpu import STUB


def test_dendro_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dendro_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DDENDRO_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("variant 0: slices 95 ") and r.stdout.endswith("done\n")
    assert "ring 257: stem 1 inliers 257 " in r.stdout and "ring 9: stem 0 inliers 0 " in r.stdout
