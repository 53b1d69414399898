"""CPU: AddressSanitizer + UBSan run of the alignment header's host build (tests/stub/align_capi.cpp with its driver, a
stand-alone program run as a child process): the lock-step batch against single runs with starts that converge, hit the limit,
end FEW and end DEGENERATE, the vote on one and on three threads, the whole alignment of a plot under a 137 degree yaw at
scale 2.3, one scale, one yaw, 4 and 128 bins, one sample a side, the empty cases and the refusals.  Host code only:
sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_align_cpu import STUB


def test_align_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "align_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DALIGN_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and r.stdout.endswith("done\n")
    assert "batch 0: iterations 1 pairs 1500 converged 1 flags 0\n" in r.stdout and "batch 1: iterations 6 pairs 1500 converged 0 flags 0\n" in r.stdout
    assert "batch 2: iterations 0 pairs 0 converged 0 flags 1\n" in r.stdout
    assert r.stdout.count("align: flags 0 winner 6 of 16 (same 2) pairs 235 scale 2.30000\n") == 2
    assert "edge 3: flags 2 candidates 0\n" in r.stdout
