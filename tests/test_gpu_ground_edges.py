"""GPU: csrc/ground.hip at the shapes its kernels can break at (the scenes: tests/ground_scenes.py) -- a selection list of 3 and 4
points and on, one before and one past a wave (64), a refit pass (256), gnd_score's LDS chunk (1 024), for_own_points' batch of
256 * 8 = 2 048 and gnd_score's point block of 8 192 (at 8 193 its second block holds one point), the same with masked rows so
that only the list is on the edge, iteration counts around a wave's 4 and a workgroup's 16 hypotheses, a tie that crosses
gnd_pick's four waves and its stride of 256 (won by iteration 0, and, on another scene, by an iteration of each later wave and
of the second stride), one and three camera centres, and a handle reused with a shorter list.  Every case
is compared bit for bit on the result with the g++ build of the same header (tests/stub/ground_capi.cpp), which
tests/test_ground_edges_cpu.py holds to the Python transcription on the same cases; the planted fact of each scene is asserted
on the device's output too."""
import pytest

from sfm_danpipeline_amd import ground
from sfm_danpipeline_amd.cloud import Cloud
from tests import ground_scenes as scenes
from tests.test_ground_cpu import gn, grid_plane, result_bytes, stub_opts  # noqa: F401
from tests.test_ground_edges_cpu import EDGE_ITERS, MASKED, REFIT8_SIZES, TIE_ITERS, TIE_KW, cams_under, check_disc, disc, masked, tie_slab
from tests.test_gpu_ground import assert_equal

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the selection's size on every edge
@pytest.mark.parametrize("n", scenes.SIZES)
def test_disc_sizes(ctx, gn, n):
    xyz, kw, planted = disc(n)
    with Cloud(xyz) as c:
        for refits in (0, 2):
            check_disc(assert_equal(gn, xyz, opts=stub_opts(gn, **dict(kw, refit_rounds=refits)), cloud=c), planted)


@pytest.mark.parametrize("n", REFIT8_SIZES)
def test_disc_eight_refits(ctx, gn, n):
    xyz, kw, planted = disc(n)
    check_disc(assert_equal(gn, xyz, opts=stub_opts(gn, **dict(kw, refit_rounds=8))), planted)


@pytest.mark.parametrize("n_sel,n", MASKED)
def test_masked_disc(ctx, gn, n_sel, n):
    xyz, lab, label, kw, planted = masked(n_sel, n)
    res = assert_equal(gn, xyz, lab, label, stub_opts(gn, **kw))
    assert res.flags == 0 and res.n_selected == n_sel and res.winner >= 0


# ---------------------------------------------------------------- iteration counts on the hypothesis tiles
@pytest.mark.parametrize("iters", EDGE_ITERS)
def test_iteration_counts(ctx, gn, iters):
    xyz, kw, planted = disc(3000)
    check_disc(assert_equal(gn, xyz, opts=stub_opts(gn, **dict(kw, ransac_iters=iters))), planted)


# ---------------------------------------------------------------- the tie across gnd_pick's waves and strides
@pytest.mark.parametrize("iters", TIE_ITERS)
def test_tie_beyond_the_first_256(ctx, gn, iters):
    xyz = grid_plane().astype("float32")
    res = assert_equal(gn, xyz, opts=stub_opts(gn, ransac_iters=iters, **TIE_KW))
    assert res.winner == 0 and res.inliers == 900 and tuple(res.up) == (0.0, 0.0, 1.0)


@pytest.mark.parametrize("seed", sorted(scenes.TIE_SLAB_WINNERS))
def test_tie_won_in_each_wave_and_stride(ctx, gn, seed):
    xyz, kw, planted = tie_slab()
    res = assert_equal(gn, xyz, opts=stub_opts(gn, seed=seed, **kw))
    assert res.winner == planted["winners"][seed] and res.inliers == planted["n_plane"]


# ---------------------------------------------------------------- camera centres
@pytest.mark.parametrize("n_cam", [1, 3])
def test_camera_centres_turn_the_plane_over(ctx, gn, n_cam):
    xyz, kw, planted = disc(8193)
    cams = cams_under(planted, n_cam)
    with Cloud(xyz) as c:
        res = assert_equal(gn, xyz, opts=stub_opts(gn, **dict(kw, below_max=1.0)), cams=cams, cloud=c)
        assert res.flags == 0 and res.below >= 8193 - planted["n_plane"] and sum(u * v for u, v in zip(res.up, planted["up"])) < -0.999
        assert assert_equal(gn, xyz, opts=stub_opts(gn, **kw), cams=cams, cloud=c).winner == -1
        check_disc(assert_equal(gn, xyz, opts=stub_opts(gn, **kw), cloud=c), planted)       # (and none again after three)


# ---------------------------------------------------------------- a shorter list after a longer one on the same handle
def test_handle_reuse_with_a_shorter_list(ctx, gn):
    xyz, kw, planted = disc(16385)
    lab = scenes.pick_labels(planted, 64)
    o = stub_opts(gn, **kw)
    with Cloud(xyz) as c:
        check_disc(assert_equal(gn, xyz, opts=o, cloud=c), planted)
        small = assert_equal(gn, xyz, lab, 1, o, cloud=c)
        assert small.flags == 0 and small.n_selected == 64
        check_disc(assert_equal(gn, xyz, opts=o, cloud=c), planted)
    with Cloud(xyz) as c:
        assert result_bytes(ground.ground_plane(c, lab, 1, o)) == result_bytes(small)
