"""CPU: AddressSanitizer + UBSan run of the terrain header's host build (tests/stub/terrain_capi.cpp with its driver, a
stand-alone program run as a child process): three trees on an undulating slope with holes under the crowns, rotated, with NaN
points and a tree under its own label, through nine option sets (labels, two cells, the linear table, a scale, no window, a
fill that leaves holes, no fill and no relaxation, slope 0 with wide windows), an empty selection, 1 and 3 points, a one-row
raster, the raster's cap and the refusals.  Host code only: sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_terrain_cpu import STUB


def test_terrain_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "terrain_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DTERRAIN_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("variant 0: raster 48 x 48 selected 25025 ") and r.stdout.endswith("done\n")
    assert "variant 5: raster 48 x 48 selected 25025 ground 25025 windows 0 " in r.stdout and " flags 4\n" in r.stdout   # no window
    assert "variant 7: " in r.stdout and " rounds 0 flags 2\n" in r.stdout and "three points: raster 15 x 1 selected 3 ground 2 " in r.stdout
