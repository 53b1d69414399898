"""GPU: csrc/dendro.hip at the shapes its kernels can break at (the scenes: tests/dendro_scenes.py) -- slice populations on and
around min_slice_pts, dnd_ransac's 64-lane stride and 1 024-pair LDS chunk and dnd_refit's 256-thread pass, the ransac / refit
gate on a lane edge, iteration counts around a wave's 4 and a workgroup's 16 hypotheses, a cloud beyond one trip of dnd_keys'
grid-stride loop, S = MAX_SLICES with a populated capped slice and the extent stage running, finite points under a given ground,
the extent histogram's last bin and both ends of extent_q, and a handle reused with fewer slices or fewer points than the call
before.  Every case is compared bit for bit -- the whole slice table and the result -- with the g++ build of the same header
(tests/stub/dendro_capi.cpp), which tests/test_dendro_edges_cpu.py holds to the Python transcription on the same scenes; the
planted fact of each scene is asserted on the device's output too."""
import numpy as np
import pytest

from sfm_danpipeline_amd import dendro
from sfm_danpipeline_amd.cloud import Cloud
from tests import dendro_scenes as scenes
from tests.test_dendro_cpu import MAX_SLICES, NO_CROWN, dn, result_bytes, stub_opts  # noqa: F401
from tests.test_dendro_edges_cpu import EDGE_ITERS, built, check_slice_stack, thirty_labels
from tests.test_gpu_dendro import assert_equal

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- slice populations on the kernels' strides
def test_slice_stack(ctx, dn):
    xyz, kw, planted = built("slice_stack")
    res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **kw), both=True)
    check_slice_stack(res, rows, planted)
    assert rows["stem"].tolist() == [0, 0, 0] + [1] * 13 and res.flags == 0


@pytest.mark.parametrize("min_slice_pts", [64, 65])
def test_slice_stack_gate_on_a_lane_edge(ctx, dn, min_slice_pts):
    xyz, kw, planted = built("slice_stack")
    res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **dict(kw, min_slice_pts=min_slice_pts)), both=True)
    check_slice_stack(res, rows, planted, min_slice_pts)
    k = planted["pops"].index(min_slice_pts)
    assert rows["stem"][:k].sum() == 0 and rows["stem"][k:].all()


@pytest.mark.parametrize("iters", EDGE_ITERS)
def test_slice_stack_iteration_counts(ctx, dn, iters):
    xyz, kw, planted = built("slice_stack")
    res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **dict(kw, ransac_iters=iters)))
    check_slice_stack(res, rows, planted)


# ---------------------------------------------------------------- the slice cap
def test_capped_slices(ctx, dn):
    xyz, kw, planted = built("capped_slices")
    with Cloud(xyz) as c:
        res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **kw), cloud=c, both=True)
        assert res.n_slices == MAX_SLICES == len(rows) and rows["count"][-1] == planted["top_count"] and res.flags == NO_CROWN
        assert np.nonzero(rows["stem"])[0].tolist() == list(planted["dbh_slices"]) + [MAX_SLICES - 1]
        assert np.array_equal(np.isfinite(rows["extent"]), rows["count"] > 0)
        res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **planted["crown_kw"]), cloud=c, both=True)
        assert res.flags == 0 and res.crown_base_slice == MAX_SLICES - 1


# ---------------------------------------------------------------- under the ground, the last bin, extent_q's ends
def test_below_ground(ctx, dn):
    xyz, kw, planted = built("below_ground")
    with Cloud(xyz) as c:
        res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **kw), cloud=c, both=True)
        assert res.n_selected == planted["n"] and rows["count"].sum() == planted["n"] - planted["under"] and res.flags == 0
        assert np.nanmax(rows["extent"]) == planted["last_extent"]
        tiny, trows = assert_equal(dn, xyz, opts=stub_opts(dn, **planted["tiny_q_kw"]), cloud=c, both=True)
        assert (trows["extent"][:30] < scenes.RING_R).all() and (rows["extent"][:30] > scenes.RING_R).all()


# ---------------------------------------------------------------- beyond one trip of dnd_keys' grid
def test_past_the_key_grid(ctx, dn):
    xyz, kw, planted = built("past_the_key_grid")
    assert len(xyz) > scenes.KEY_GRID
    res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, **kw))
    assert res.n_selected == len(xyz) == rows["count"].sum() and res.flags == 0 and rows["stem"][:30].all()


# ---------------------------------------------------------------- a smaller call after a larger one on the same handle
def fresh(xyz, labels=None, label=0, opts=None):
    with Cloud(xyz) as c:
        return dendro.measure_profile(c, labels, label, opts)


def test_handle_reuse_with_fewer_slices_and_fewer_points(ctx, dn):
    xyz, kw, planted = built("capped_slices")
    lab, label = thirty_labels(xyz)
    calls = [(None, 0, kw, MAX_SLICES), (None, 0, dict(slice=20.0), 1), (None, 0, {}, 91),       # S = 4 096, then 1, then 91
             (None, 0, kw, MAX_SLICES), (lab, label, kw, None), (lab, label, {}, None)]         # every point, then 30 of them
    with Cloud(xyz) as c:
        for labels, which, okw, S in calls:
            o = stub_opts(dn, **okw)
            res, rows = assert_equal(dn, xyz, labels, which, o, cloud=c)
            fres, frows = fresh(xyz, labels, which, o)
            assert rows.tobytes() == frows.tobytes() and result_bytes(res) == result_bytes(fres)
            assert res.n_slices == (S or res.n_slices) and res.n_selected == (30 if labels is not None else len(xyz))
