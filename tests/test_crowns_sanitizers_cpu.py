"""CPU: AddressSanitizer + UBSan run of the crowns header's host build (tests/stub/crowns_capi.cpp with its driver, a
stand-alone program run as a child process): both planted crown layouts as rasters with empty cells through seven option sets
(two cells, 0.1 m without smoothing, 64 passes, a scale, one wide window with a tight crown, the tree cap), each followed by
the points of rule 10 with a NaN and an infinite height; 1 x 1, one-row, one-column, empty, all-empty and no-canopy rasters; a
plateau; the window's cap and the refusals.  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_crowns_cpu import STUB


def test_crowns_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "crowns_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DCROWNS_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("scene 0 variant 0: raster 56 x 56 canopy ") and r.stdout.endswith("done\n")
    assert r.stdout.count(" trees 6 ") >= 6 and "scene 1 variant 0: " in r.stdout and r.stdout.count(" flags 4\n") == 2   # the tree cap
    assert "one cell: raster 1 x 1 canopy 1 summits 1 trees 1 cells 1 " in r.stdout and "one row: raster 300 x 1 " in r.stdout
    assert "plateau: raster 40 x 40 canopy 1600 summits 1 trees 1 " in r.stdout and "cap: raster 40 x 40 " in r.stdout
