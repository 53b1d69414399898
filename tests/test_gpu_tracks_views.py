"""GPU: the track consolidation of the C++ host mirror (csrc/host/SfmTracks.cpp: StructFromMotion::consolidateTracks over
sfmhip_tracks_build / sfmhip_tracks_triangulate) through sfm_tracks_selftest, on the ring scene of tests/test_gpu_incr_views.py:
eight cameras, every point seen by three consecutive views, exact correspondences.  Before the consolidation every point of
the cloud has two views, as addMoreViews leaves it; after it there are points with three, no (view, feature) belongs to two
points, the largest point error against ground truth stays within 10 x that of the unconsolidated cloud of the same run, and
adjustBundle on the consolidated cloud converges.  Then the ten temple frames, structure only: there the tracks are built from
a match plan's lists on the device."""
import os
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import build
from tests.test_gpu_incr_views import TEMPLE, _read_out, _ring_scene, _similarity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    return build.build_tracks_demo()


def _world_ids(n_views=8, n_points=1600, seed=3):
    """the world point of every (view, feature) of _ring_scene, by replaying its draws"""
    g = np.random.default_rng(seed)
    X = g.uniform(-1, 1, (n_points, 3))
    first = np.arange(n_points) % (n_views + 2) - 2
    ids = []
    for v in range(n_views):
        i = np.flatnonzero((first <= v) & (v <= first + 2))
        ids.append(i[g.permutation(len(i))])
    return X, ids


def _worst_point_error(o, X, ids):
    """the largest distance of a cloud point from its world point after the similarity alignment of the whole cloud"""
    world = np.array([ids[tr[0][0]][tr[0][1]] for tr in o["tracks"]])
    for tr, w in zip(o["tracks"], world):
        assert all(ids[v][f] == w for v, f in tr)              # exact correspondences: a track is one world point
    s, R, t = _similarity(o["xyz"], X[world])
    return float(np.linalg.norm(s * o["xyz"] @ R.T + t - X[world], axis=1).max())


@pytest.fixture(scope="module")
def run(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("tracks_views")
    scene, out = str(d / "ring.bin"), str(d / "ring")
    _, X = _ring_scene(scene)
    r = subprocess.run([exe, "--scene", scene, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    Xr, ids = _world_ids()
    assert np.array_equal(X, Xr)
    return r, _read_out(out + ".before"), _read_out(out + ".after"), X, ids


def test_consolidation_joins_the_views_of_a_point(run):
    r, before, after, X, ids = run
    assert before["good"] == after["good"] == set(range(8))
    assert all(len(tr) == 2 for tr in before["tracks"])                              # the parent's cloud
    lens = np.array([len(tr) for tr in after["tracks"]])
    # 1600 points in windows of three views starting at view -2 .. 7: 6 of 10 windows lie inside the arc, 2 are cut to two views
    assert (lens == 3).sum() == 960 and (lens == 2).sum() == 320 and len(lens) == 1280
    seen = [vf for tr in after["tracks"] for vf in tr]
    assert len(seen) == len(set(seen))                                              # no (view, feature) in two points
    assert all([v for v, _ in tr] == sorted({v for v, _ in tr}) for tr in after["tracks"])
    assert f"consolidated: {len(after['xyz'])}\n" in r.stdout


def test_consolidated_cloud_is_as_close_to_the_truth(run):
    """worst point error after the similarity alignment: the unconsolidated cloud of the same run is the yardstick, 10 x it the
    bound (DESIGN.md f-16 records both figures)"""
    r, before, after, X, ids = run
    eb, ea = _worst_point_error(before, X, ids), _worst_point_error(after, X, ids)
    print(f"MEASURE ring worst point error before {eb:.3e} after {ea:.3e}")
    assert ea <= 10 * eb


def test_bundle_adjustment_converges_on_the_consolidated_cloud(run):
    r, before, after, X, ids = run
    assert "Bundle adjustment failed" not in r.stderr.split("consolidated: ")[-1]
    last = r.stdout.split("consolidated: ")[-1]
    assert "Bundle adjustment: iterations " in last
    assert sum(len(tr) for tr in after["tracks"]) / len(after["tracks"]) > 2


def test_temple_frames_through_the_resident_image_set(exe, tmp_path):
    """structure only (there is nothing to measure the temple against): with descriptors present the tracks come from one match
    plan on the resident image set, read on the device (sfmhip_tracks_build_from_plan)"""
    out = str(tmp_path / "temple")
    r = subprocess.run([exe, "--images", TEMPLE, os.path.join(TEMPLE, "camera_calibration_template.xml"), out],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    before, after = _read_out(out + ".before"), _read_out(out + ".after")
    assert before["good"] == after["good"] and len(after["xyz"]) > 0 and np.isfinite(after["xyz"]).all()
    seen = [vf for tr in after["tracks"] for vf in tr]
    assert len(seen) == len(set(seen)) and {v for v, _ in seen} <= after["good"]
    lens = np.array([len(tr) for tr in after["tracks"]])
    assert lens.min() >= 2 and lens.max() <= len(after["good"])
    print(f"MEASURE temple consolidated {len(before['xyz'])} -> {len(after['xyz'])} points, {lens.mean():.2f} views per point, "
          f"longest {lens.max()}, registered {len(after['good'])}")
