"""The edge scenes of tests/dendro_scenes.py on the CPU: each through the g++ build of csrc/dendro.h (tests/stub/dendro_capi.cpp)
and through the Python transcription of tests/test_dendro_cpu.py, the same bytes, and the planted fact of every scene asserted
on the stub's output -- the slice populations, S = 4 096 and the capped slice's count, the finite points under the ground, the
clamped extent, both ends of extent_q, n_selected.  tests/test_gpu_dendro_edges.py runs the same scenes on the device and relies
on these facts.  No GPU."""
import functools

import numpy as np
import pytest

from tests import dendro_scenes as scenes
from tests.test_dendro_cpu import (MAX_SLICES, NO_CROWN, assert_same_result, dn, py_hypothesis, py_run, stub_opts,  # noqa: F401
                                   stub_run)

EDGE_ITERS = [3, 4, 5, 15, 16, 17, 4081, 4095]      # around a wave's 4 and a workgroup's 16 hypotheses, and the last workgroup of 256
PREFIX = 20000                                      # of the 270 000-point cloud: what the transcription walks


@functools.lru_cache(maxsize=None)
def built(name):
    """A scene of tests/dendro_scenes.py, built once for the module (and shared with the GPU file)."""
    return getattr(scenes, name)()


def stub_equals_transcription(dn, xyz, kw, labels=None, label=0):
    o = stub_opts(dn, **kw)
    res, rows, frame = stub_run(dn, xyz, labels, label, o, want_frame=True)
    want, wrows, wframe = py_run(xyz, labels, label, o)
    assert np.array_equal(frame.view(np.uint32), wframe.view(np.uint32))
    assert rows.tobytes() == wrows.tobytes()
    assert_same_result(res, want)
    return res, rows


def check_slice_stack(res, rows, planted, min_slice_pts=10):
    """The planted facts of slice_stack() on a stub or device result."""
    pops = planted["pops"]
    assert rows["count"].tolist() == pops and res.n_slices == len(pops) and res.n_selected == planted["n"]
    fitted = np.array(pops) >= min_slice_pts
    assert (rows["inliers"][~fitted] == 0).all() and (rows["inliers"][fitted] > 0).all()


# ---------------------------------------------------------------- slice populations on the kernels' strides
def test_slice_stack(dn):
    xyz, kw, planted = built("slice_stack")
    res, rows = stub_equals_transcription(dn, xyz, kw)
    check_slice_stack(res, rows, planted)
    assert planted["pops"] == [9, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
    assert rows["stem"].tolist() == [0, 0, 0] + [1] * 13 and res.flags == 0
    assert (rows["count"][12], rows["count"][13]) == (2047, 2048)               # rule 7 interpolates between these two
    assert abs(res.dbh - 2 * scenes.RING_R) < 1e-3                              # (sigma 0.005 over about 1 365 ring points a slice)
    assert np.abs(rows["radius"][3:] - scenes.RING_R).max() < 5e-3


@pytest.mark.parametrize("min_slice_pts", [64, 65])
def test_slice_stack_gate_on_a_lane_edge(dn, min_slice_pts):
    xyz, kw, planted = built("slice_stack")
    res, rows = stub_equals_transcription(dn, xyz, dict(kw, min_slice_pts=min_slice_pts))
    check_slice_stack(res, rows, planted, min_slice_pts)
    k = planted["pops"].index(min_slice_pts)                                    # the slice whose population IS the gate
    assert rows["stem"][k] == 1 and rows["stem"][:k].sum() == 0 and rows["stem"][k:].all()
    assert np.isnan(rows["radius"][:k]).all()


@pytest.mark.parametrize("iters", EDGE_ITERS)
def test_slice_stack_iteration_counts(dn, iters):
    xyz, kw, planted = built("slice_stack")
    res, rows = stub_equals_transcription(dn, xyz, dict(kw, ransac_iters=iters))
    check_slice_stack(res, rows, planted)


def test_last_hypotheses_of_the_edge_counts_are_live(dn):
    """Iteration iters - 1 of the DBH slice is a valid circle at some of the edge counts, so a kernel that dropped or added a
    hypothesis at a tile edge would see another candidate list."""
    xyz, kw, _ = built("slice_stack")
    en = xyz[np.abs(xyz[:, 2] - 1.25) < 0.01][:, :2]                            # slice 12, ascending input index
    assert len(en) == 2047
    o = stub_opts(dn, **kw)
    live = [it for it in EDGE_ITERS if py_hypothesis(en, o, 12, it - 1, 0.02, 1.5) is not None]
    assert len(live) >= 2, live


# ---------------------------------------------------------------- the slice cap
def test_capped_slices(dn):
    xyz, kw, planted = built("capped_slices")
    res, rows = stub_equals_transcription(dn, xyz, kw)
    assert res.n_slices == planted["S"] == MAX_SLICES == len(rows)
    assert rows["count"][-1] == planted["top_count"] == 646 and res.n_selected == len(xyz) == rows["count"].sum()
    above = xyz[:, 2].astype(np.float64) / scenes.CAP_SLICE >= MAX_SLICES                       # what the clamp collects
    assert int(above.sum()) > 600 and int((np.floor(xyz[:, 2].astype(np.float64) / scenes.CAP_SLICE) == MAX_SLICES - 1).sum()) < 10
    lo, hi = planted["dbh_slices"]
    # (the capped slice's 646 crown points hold a circle of 20 inliers too: the refit runs on the last row of the table)
    assert np.nonzero(rows["stem"])[0].tolist() == [lo, hi, MAX_SLICES - 1]
    assert rows["count"][lo] >= planted["ring"] and rows["count"][hi] >= planted["ring"]
    assert res.flags == NO_CROWN and abs(res.dbh - 2 * scenes.RING_R) < 1e-4
    # the extent stage ran over every slice: a number wherever a slice holds a point, the capped one included
    assert np.array_equal(np.isfinite(rows["extent"]), rows["count"] > 0) and np.isfinite(rows["extent"][-1])
    assert (rows["count"] == 0).sum() > 1000
    # ... and with a run of one the capped slice is the crown base
    res1, rows1 = stub_equals_transcription(dn, xyz, planted["crown_kw"])
    assert res1.flags == 0 and res1.crown_base_slice == MAX_SLICES - 1 and rows1.tobytes() == rows.tobytes()
    assert 2.0 < res1.spread_ew < 4.0 and 1.5 < res1.spread_ns < 3.0                            # the shell above 8.19 only


def test_single_slice_and_default_slices_on_the_capped_cloud(dn):
    """The options the device's reuse test runs after S = 4 096 on the same handle."""
    xyz, kw, _ = built("capped_slices")
    res, rows = stub_equals_transcription(dn, xyz, dict(slice=20.0))
    assert res.n_slices == 1 and rows[0]["count"] == len(xyz)
    res, rows = stub_equals_transcription(dn, xyz, {})
    assert res.n_slices == 91
    lab, label = thirty_labels(xyz)
    res, rows = stub_equals_transcription(dn, xyz, kw, lab, label)
    assert res.n_selected == 30 and 1 < res.n_slices < MAX_SLICES


def thirty_labels(xyz):
    """Labels that select the 30 trunk points of lowest index under 2.0 (label 7 among 3s)."""
    lab = np.full(len(xyz), 3, np.int32)
    lab[np.nonzero(xyz[:, 2] < 2.0)[0][:30]] = 7
    return lab, 7


# ---------------------------------------------------------------- under the ground, the last bin, extent_q's ends
def test_below_ground(dn):
    xyz, kw, planted = built("below_ground")
    res, rows = stub_equals_transcription(dn, xyz, kw)
    under = xyz[:, 2].astype(np.float64) - scenes.BELOW_GROUND < 0.0
    assert np.isfinite(xyz).all() and int(under.sum()) == planted["under"] == 1913
    assert res.n_selected == planted["n"] == 30000 and rows["count"].sum() == 30000 - 1913 and res.flags == 0
    assert res.ground == scenes.BELOW_GROUND
    assert np.nanmax(rows["extent"]) == planted["last_extent"] == 1.024                         # bin 1 023, the clamp
    far = np.hypot(xyz[:, 0], xyz[:, 1]) > 1.1                                                   # ... and points really lie past it
    assert int(far.sum()) > 1000
    trunk = slice(0, 30)                                                                        # heights 0.75 .. 3.75
    assert (rows["extent"][trunk] > scenes.RING_R).all()                                        # q = 1: the farthest point
    tiny, trows = stub_equals_transcription(dn, xyz, planted["tiny_q_kw"])
    assert (trows["extent"][trunk] < scenes.RING_R).all()                                       # need = 1: the nearest
    assert all(trows[f].tobytes() == rows[f].tobytes() for f in ("count", "stem", "inliers", "mask", "ce", "cn", "radius", "rms"))
    assert tiny.flags == 0 and np.nanmax(trows["extent"]) == 1.024                              # (a crown slice is a hollow ring)


# ---------------------------------------------------------------- beyond one trip of dnd_keys' grid
def test_past_the_key_grid(dn):
    xyz, kw, planted = built("past_the_key_grid")
    assert len(xyz) == planted["n"] > scenes.KEY_GRID
    res, rows, _ = stub_run(dn, xyz, opts=stub_opts(dn, **kw))
    assert res.flags == 0 and res.n_selected == len(xyz) == rows["count"].sum() and res.n_slices == 91
    assert rows["stem"][:30].all() and rows["count"][:30].min() > 2048
    stub_equals_transcription(dn, xyz[:PREFIX], kw)
