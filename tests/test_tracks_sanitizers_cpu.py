"""CPU: AddressSanitizer + UBSan run of the tracks header's host build (tests/stub/tracks_capi.cpp with its driver, a
stand-alone program run as a child process): a 12-image match graph from world ids with false matches and an image without
features, through three min_len values; empty inputs and every refusal; then a ring scene triangulated with the cheirality
option, under distortion, with a NaN pixel, with every second view unposed and with one posed view.  Host code only:
sanitizers do not run on the GPU."""
import os
import subprocess

from tests.test_tracks_cpu import STUB


def test_tracks_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tracks_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DTRACKS_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and r.stdout.startswith("min_len 0: nodes ") and r.stdout.endswith("done\n")
    assert "graphs done\n" in r.stdout and all(f"variant {v}: kept " in r.stdout for v in range(5))
    lines = r.stdout.splitlines()
    tracks = [int(l.split(" tracks ")[1].split()[0]) for l in lines[:3]]
    assert tracks[0] == tracks[1] > tracks[2] > 0                     # min_len 0 asks for 2; 4 drops the short ones
    assert " conflicting 0 " not in lines[0]                          # the false matches made conflicts
    assert lines[-2].startswith("variant 4: kept 0 unused ")
