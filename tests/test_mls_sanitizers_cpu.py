"""CPU: AddressSanitizer + UBSan run of the smoothing header's host build (tests/stub/mls_capi.cpp with its driver, a
stand-alone program run as a child process): a noisy sheet with NaN and infinite rows at the three orders by both neighbour
searches, a Gaussian whose far weights underflow, a radius that leaves every point alone, the clouds of 0, 1 and 2 points,
clusters of 2, 3, 5, 6, 63, 64, 65 and 129 points, identical and collinear points, a singular fit, a far outlier and the
refusals.  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.mls_scenes import STUB


def test_mls_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mls_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DMLS_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("sheet: order 0 search 1 rc 0 out 4925 ") and r.stdout.endswith("done\n")
    assert r.stdout.count("sheet: ") == 6 and "tiny radius: order 2 search 0 rc 0 out 0 dropped 4925 " in r.stdout
    assert "same: order 2 search 0 rc 0 out 70 dropped 0 plane_only 0 degenerate 70 " in r.stdout
    assert "line: order 2 search 0 rc 0 out 40 dropped 0 plane_only 0 degenerate 40 " in r.stdout
    assert "singular: order 2 search 0 rc 0 out 17 dropped 0 plane_only 0 degenerate 0 failed 1 " in r.stdout
    assert "cluster: order 2 search 0 rc 0 out 5 dropped 0 plane_only 5 " in r.stdout and "refusals -3 -3 -3 -3 -3\n" in r.stdout
