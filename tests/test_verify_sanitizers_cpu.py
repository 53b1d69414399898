"""CPU: AddressSanitizer + UBSan run of the verification header's host build (tests/stub/verify_capi.cpp with its driver, a
stand-alone program run as a child process): pairs of 300, 5 and 0 matches over three images (one without features, slack in
xy_ptr) under every `has` code, min_inliers below, at and above the inlier count, the compaction from E against the one from
a mask, the empty inputs and the refusals.  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_verify_cpu import STUB


def test_verify_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "verify_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DVERIFY_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and r.stdout.endswith("done\n")
    assert "min_inliers 0: kept 3 no_model 1 in 605 out 405 counts 200 5 0 200\n" in r.stdout
    assert "min_inliers 200: kept 2 no_model 1 in 605 out 400 counts 200 0 0 200\n" in r.stdout
    assert "min_inliers 201: kept 0 no_model 1 in 605 out 0 counts 0 0 0 0\n" in r.stdout
    assert "mask == E: out 400\n" in r.stdout
