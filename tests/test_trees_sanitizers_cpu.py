"""CPU: AddressSanitizer + UBSan run of the tree-extraction header's host build (tests/stub/trees_capi.cpp with its driver, a
stand-alone program run as a child process): four trees on a noisy ground disc, rotated, two of them touching, with NaN
points and one tree under its own label, through eight option sets (labels and four threads, max_trees with a short stem
table, max_path, other grid sizes, a scale, no stem, nothing above), an empty cloud and an empty selection, one point, a
20-long pole, both grid caps and the refusals.  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_trees_cpu import STUB


def test_trees_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "trees_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DTREES_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("variant 0: selected 32000 above ") and r.stdout.endswith("done\n")
    assert r.stdout.splitlines()[0].split(" voxels ")[0].endswith(" trees 4") and "variant 1: selected 26000 " in r.stdout
    assert "variant 2: " in r.stdout and " trees 2 " in r.stdout and " flags 4 " in r.stdout              # max_trees
    assert " trees 0 voxels 0 labelled 0 max_cost 0 flags 2\n" in r.stdout and " flags 1\n" in r.stdout   # no stem; nothing above
    assert "one point: selected 1 above 1 band 1 trees 1 voxels 1 labelled 1 max_cost 0 flags 0" in r.stdout
    assert "pole: selected 4000 " in r.stdout and " trees 1 " in r.stdout
