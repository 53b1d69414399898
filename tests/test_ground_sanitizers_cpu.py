"""CPU: AddressSanitizer + UBSan run of the ground-plane header's host build (tests/stub/ground_capi.cpp with its driver, a
stand-alone program run as a child process): a tree on a noisy ground disc with NaN points and a wall under its own label
through seven option sets (1 and 4096 iterations, 0 and 8 refits, camera centres, a hint, a zero north hint), an empty
selection, 1 .. 3 points, a sphere shell, collinear and identical points, and the refusals.  Host code only: sanitizers do
not run on the GPU."""
import os
import subprocess

from tests.test_ground_cpu import STUB


def test_ground_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ground_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DGROUND_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("variant 0: selected 17000 inliers ") and r.stdout.endswith("done\n")
    assert "variant 1: selected 17000 inliers 0 below 0 above 0 winner -1 flags 2 " in r.stdout          # one iteration: no plane
    assert "variant 6: " in r.stdout and " flags 8 " in r.stdout and "points 3: flags 0 inliers 3" in r.stdout
