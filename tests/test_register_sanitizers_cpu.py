"""CPU: AddressSanitizer + UBSan run of the registration header's host build (tests/stub/register_capi.cpp with its driver, a
stand-alone program run as a child process): the search over a box of points with duplicates and NaN rows from sources inside,
outside and far outside it against a plain loop (scene 1), a planted motion with and without scale, whole and as a partial
overlap with strangers under max_dist (scenes 3 and 4), the loop's edges -- no iteration, one, eps, source == target, no
source, no target, a target of NaN rows, collinear and identical points, a source farther away than max_dist -- and rule 1's
refusals (scene 5).  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_register_cpu import STUB


def test_register_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "register_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DREGISTER_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and r.stdout.startswith("nearest max_dist inf: kept 298\n") and r.stdout.endswith("done\n")
    assert "nearest max_dist 0.01: kept 0\n" in r.stdout
    for v in range(6):
        assert f"variant {v}: n_src " in r.stdout
    assert " pairs 2000 converged 1 flags 0 " in r.stdout and "variant 4: n_src 1474 " in r.stdout and " pairs 1074 converged 1 flags 0 " in r.stdout
