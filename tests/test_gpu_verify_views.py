"""GPU: the two-view verification inside the track consolidation of the C++ host mirror (csrc/host/SfmTracks.cpp:
StructFromMotion::consolidateTracks(minViews, verify) over sfmhip_verify_lists / sfmhip_tracks_build_from_verified) through
sfm_tracks_selftest --verify, on the ring scene of tests/test_gpu_tracks_views.py with a share of its matches pointed at a
displaced pixel: the train index of one match in forty is replaced by another feature of that image, as a ratio test that let
a wrong neighbour through would leave it.  Without the switch those matches join features of different world points and whole
components are dropped as conflicting; with it they fail the pair's epipolar test first.  The run without the switch prints
what it printed before the switch existed."""
import re
import struct
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import build
from tests.test_gpu_incr_views import _read_out, _ring_scene

pytestmark = pytest.mark.gpu

SHARE = 0.025


def _displace(src, dst, seed=9, share=SHARE):
    """rewrite a scene file with `share` of every pair's matches pointed at another feature of the train image"""
    g = np.random.default_rng(seed)
    raw = open(src, "rb").read()
    (n_img,), o = struct.unpack_from("<i", raw, 0), 4 + 72 + 40
    n_feat = []
    for _ in range(n_img):
        (n,) = struct.unpack_from("<i", raw, o)
        n_feat.append(n)
        o += 4 + 16 * n
    out = bytearray(raw[:o + 4])
    (n_pairs,) = struct.unpack_from("<i", raw, o)
    o += 4
    moved = 0
    for _ in range(n_pairs):
        q, t, m = struct.unpack_from("<iii", raw, o)
        qt = np.frombuffer(raw, np.int32, 2 * m, o + 12).reshape(-1, 2).copy()
        bad = g.random(m) < share
        qt[bad, 1] = (qt[bad, 1] + 1 + g.integers(0, n_feat[t] - 1, int(bad.sum()))) % n_feat[t]   # (never the index it had)
        moved += int(bad.sum())
        out += struct.pack("<iii", q, t, m) + qt.tobytes()
        o += 12 + 8 * m
    assert o == len(raw)
    open(dst, "wb").write(bytes(out))
    return moved


def _track_line(stdout):
    m = re.search(r"consolidateTracks: (\d+) tracks \((\d+) conflicting, (\d+) short\)", stdout)
    assert m, stdout[-2000:]
    return tuple(int(x) for x in m.groups())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    exe = build.build_tracks_demo()
    d = tmp_path_factory.mktemp("verify_views")
    clean, scene = str(d / "ring.bin"), str(d / "ring_displaced.bin")
    _ring_scene(clean)
    moved = _displace(clean, scene)
    out = {}
    for name, extra in (("plain", []), ("verify", ["--verify"])):
        r = subprocess.run([exe, "--scene", scene, str(d / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        out[name] = (r, _read_out(str(d / name) + ".after"))
    return moved, out


def test_verify_switch_drops_fewer_components(runs):
    moved, out = runs
    plain, ver = _track_line(out["plain"][0].stdout), _track_line(out["verify"][0].stdout)
    m = re.search(r"verified: pairs (\d+) kept (\d+) no_model (\d+) matches (\d+) -> (\d+)\n", out["verify"][0].stdout)
    assert m, out["verify"][0].stdout[-2000:]
    pairs, kept, no_model, m_in, m_out = (int(x) for x in m.groups())
    print(f"MEASURE verify views: displaced {moved}; tracks {plain[0]} -> {ver[0]}, conflicting {plain[1]} -> {ver[1]}; pairs {pairs} kept {kept}, "
          f"matches {m_in} -> {m_out}")
    assert moved > 20 and plain[1] > 0                                 # the input does lose components without the switch
    assert ver[1] < plain[1] and ver[0] > plain[0]
    # the 13 pairs of views one or two apart hold every match; a displaced match survives only within 1 px of its epipolar
    # line, about 2 px of a 480 px image, so nine in ten of them gone is a loose statement of "nearly all"
    assert pairs == 28 and kept == 13 and m_out <= m_in - moved * 0.9
    assert "verify: " in out["verify"][0].stdout
    seen = [vf for tr in out["verify"][1]["tracks"] for vf in tr]
    assert len(seen) == len(set(seen))


def test_the_run_without_the_switch_prints_what_it_printed(runs):
    _, out = runs
    r = out["plain"][0]
    assert "verify: " not in r.stdout and "verified: " not in r.stdout and "verify" not in r.stderr
    assert re.search(r"consolidateTracks: \d+ tracks \(\d+ conflicting, \d+ short\), \d+ points for \d+\n", r.stdout)
    assert f"consolidated: {len(out['plain'][1]['xyz'])}\n" in r.stdout
