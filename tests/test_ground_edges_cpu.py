"""The edge scenes of tests/ground_scenes.py on the CPU: each through the g++ build of csrc/ground.h (tests/stub/ground_capi.cpp)
and through the Python transcription of tests/test_ground_cpu.py, the same bytes, and the planted fact of every scene asserted
on the stub's output -- n_selected on and around 64, 256, 1 024, 2 048 and 8 192 with and without masked rows, the iteration
counts around a wave's 4 and a workgroup's 16 hypotheses, the tie among iterations of every wave and stride of gnd_pick (won by
iteration 0 on the grid, by a chosen later iteration on tie_slab()), the camera centres that turn the plane over.  tests/test_gpu_ground_edges.py runs the same cases on the device and relies on these
facts.  No GPU."""
import functools

import numpy as np
import pytest

from tests import ground_scenes as scenes
from tests.test_ground_cpu import (assert_same_result, gn, grid_plane, py_hypothesis, py_run, result_bytes, stub_opts,  # noqa: F401
                                   stub_run)

EDGE_ITERS = [15, 16, 17, 63, 64, 65, 255, 256, 257, 4081, 4095]
REFIT8_SIZES = [2047, 2048, 2049, 8193]
MASKED = [(1024, 1500), (8193, 10007)]             # (n_sel, n): the list on an edge, the cloud on none
TIE_ITERS = [257, 512, 4095]
TIE_KW = dict(inlier_tol=0.1, refit_rounds=0)


@functools.lru_cache(maxsize=None)
def disc(n):
    """ground_disc(n), built once for the module (and shared with the GPU file)."""
    return scenes.ground_disc(n)


@functools.lru_cache(maxsize=None)
def masked(n_sel, n):
    return scenes.ground_disc_masked(n_sel, n)


def stub_equals_transcription(gn, xyz, kw, labels=None, label=0, cams=None):
    o = stub_opts(gn, **kw)
    res = stub_run(gn, xyz, labels, label, o, cams)
    assert_same_result(res, py_run(xyz, labels, label, o, cams))
    return res


def check_disc(res, planted):
    """The planted facts of a ground_disc on a stub or device result."""
    n = planted["n"]
    assert res.flags == 0 and res.n_selected == n and res.winner >= 0
    if n >= 63:            # (with 3 or 4 points the plane may pass through the column)
        # the patch's noise is a third of the tolerance: all but a few per thousand of its points are inliers, the column is above
        assert np.dot(res.up[:], planted["up"]) > 0.999 and res.inliers >= 0.98 * planted["n_plane"]
        assert res.above >= n - planted["n_plane"] and res.below <= n // 100


def cams_under(planted, m):
    """m camera centres: the majority (all of one, two of three) UNDER the disc's plane."""
    R_up = np.asarray(planted["up"])
    side = np.array([-2.0, -3.0, 1.5])[:m]
    return np.array([[0.3 * k, -0.2 * k, 0.0] for k in range(m)]) + side[:, None] * R_up[None, :]


# ---------------------------------------------------------------- the selection's size on every edge
@pytest.mark.parametrize("n", scenes.SIZES)
def test_disc_sizes(gn, n):
    xyz, kw, planted = disc(n)
    assert len(xyz) == n and np.isfinite(xyz).all()
    for refits in (0, 2):
        check_disc(stub_equals_transcription(gn, xyz, dict(kw, refit_rounds=refits)), planted)


@pytest.mark.parametrize("n", REFIT8_SIZES)
def test_disc_eight_refits(gn, n):
    xyz, kw, planted = disc(n)
    check_disc(stub_equals_transcription(gn, xyz, dict(kw, refit_rounds=8)), planted)


@pytest.mark.parametrize("n_sel,n", MASKED)
def test_masked_disc(gn, n_sel, n):
    xyz, lab, label, kw, planted = masked(n_sel, n)
    assert len(xyz) == n and n % 64 != 0 and (planted["n_bad"], planted["n_other"]) == ((n - n_sel + 1) // 2, (n - n_sel) // 2)
    finite = np.isfinite(xyz).all(1)
    assert int((~finite).sum()) == planted["n_bad"] and int((finite & (lab == label)).sum()) == n_sel
    assert int((lab != label).sum()) == planted["n_other"] and finite[lab != label].all()
    res = stub_equals_transcription(gn, xyz, kw, lab, label)
    assert res.flags == 0 and res.n_selected == n_sel and res.winner >= 0
    # the masked rows change nothing: the list is the disc's
    keep = finite & (lab == label)
    assert result_bytes(stub_run(gn, xyz[keep], opts=stub_opts(gn, **kw))) == result_bytes(res)


# ---------------------------------------------------------------- iteration counts on the hypothesis tiles
@pytest.mark.parametrize("iters", EDGE_ITERS)
def test_iteration_counts(gn, iters):
    xyz, kw, planted = disc(3000)
    check_disc(stub_equals_transcription(gn, xyz, dict(kw, ransac_iters=iters)), planted)


# ---------------------------------------------------------------- the tie across gnd_pick's waves and strides
@pytest.mark.parametrize("iters", TIE_ITERS)
def test_tie_beyond_the_first_256(gn, iters):
    """An exact plane: every hypothesis that is not skipped counts all 900 points.  Valid ones exist in each of gnd_pick's four
    waves and in its second and later strides of 256, and iteration 0 is valid: it must win."""
    xyz = grid_plane().astype(np.float32)
    o = stub_opts(gn, ransac_iters=iters, **TIE_KW)
    valid = [j for j in range(iters) if py_hypothesis(xyz.astype(np.float64), o, j, None, -1.0) is not None]
    assert valid[0] == 0 and valid[-1] >= 256 and {(j % 256) // 64 for j in valid} == {0, 1, 2, 3}
    assert {(j % 256) // 64 for j in valid if j >= 256} == ({0} if iters == 257 else {0, 1, 2, 3})
    res = stub_equals_transcription(gn, xyz, dict(TIE_KW, ransac_iters=iters))
    assert res.winner == 0 and res.inliers == 900 and res.flags == 0


@functools.lru_cache(maxsize=None)
def tie_slab():
    return scenes.tie_slab()


@pytest.mark.parametrize("seed", sorted(scenes.TIE_SLAB_WINNERS))
def test_tie_won_in_each_wave_and_stride(gn, seed):
    """The same tie with the first of the tied iterations in gnd_pick's wave 1, 2, 3 and in its second stride."""
    xyz, kw, planted = tie_slab()
    want = planted["winners"][seed]
    o = stub_opts(gn, seed=seed, **kw)
    P = xyz.astype(np.float64)
    full = []                                                        # the iterations that count every plane point
    for j in range(kw["ransac_iters"]):
        hyp = py_hypothesis(P, o, j, None, -1.0)
        if hyp is not None and int((np.abs((P - hyp[0]) @ np.array(hyp[1])) <= kw["inlier_tol"]).sum()) >= planted["n_plane"]:
            full.append(j)
    assert full[0] == want and len(full) >= 2
    res = stub_equals_transcription(gn, xyz, dict(kw, seed=seed))
    assert res.winner == want and res.inliers == planted["n_plane"] and res.flags == 0 and tuple(res.up) == (0.0, 0.0, 1.0)


def test_tie_winners_cover_the_waves_and_the_second_stride():
    w = scenes.TIE_SLAB_WINNERS.values()
    assert {(j % 256) // 64 for j in w if j < 256} == {1, 2, 3} and {(j % 256) // 64 for j in w if j >= 256} >= {1, 3}


# ---------------------------------------------------------------- camera centres
@pytest.mark.parametrize("n_cam", [1, 3])
def test_camera_centres_turn_the_plane_over(gn, n_cam):
    xyz, kw, planted = disc(8193)
    cams = cams_under(planted, n_cam)
    res = stub_equals_transcription(gn, xyz, dict(kw, below_max=1.0), cams=cams)
    assert res.flags == 0 and np.dot(res.up[:], planted["up"]) < -0.999
    assert res.inliers >= 0.98 * planted["n_plane"] and res.below >= 8193 - planted["n_plane"] and res.above <= 81
    # ... and with the default below_max a plane with the column under it is not admissible
    assert stub_equals_transcription(gn, xyz, kw, cams=cams).winner == -1


# ---------------------------------------------------------------- what the device's reuse test selects
def test_pick_of_64_after_the_whole_disc(gn):
    xyz, kw, planted = disc(16385)
    lab = scenes.pick_labels(planted, 64)
    res = stub_equals_transcription(gn, xyz, kw, lab, 1)
    assert res.flags == 0 and res.n_selected == 64 and res.inliers >= 46 and res.above >= 16
