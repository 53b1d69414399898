"""GPU: the crown delineation (csrc/crowns.hip) against the g++ build of the same header
(tests/stub/crowns_capi.cpp), byte for byte: labels, the smoothed raster, every field of the top rows and of the result, and from
the cloud entry tree_of.  The shapes are the smallest at which the kernels can go wrong: rasters of one cell, one row, one
column, none, all empty and all low; sides of TILE - 1, TILE and TILE + 1 with empty cells at the tile corners and tops in the
raster's corners and on the tile seams; 0, 1, 2 and 64 smoothing passes; windows of R2 = 2, of the cap and past every edge; a
plateau and heights that tie across a seam; an ascent and a parent chain longer than a batch of doubling rounds; the tree cap
and a short table; the cloud entry before, after and between the other calls on a handle; then both planted scenes, the plot
inventory against the chain of the stubs, and the host mirror's self-test with --crowns."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, crowns, dendro, ground, terrain, trees
from sfm_danpipeline_amd.cloud import Cloud
from tests.crown_scenes import APART, TOUCHING, scene
from tests.test_crowns_cpu import (ARRAYS, BATCH, NAN, NO_CANOPY, OVERFLOW, REFUSALS, cn, flat_opts, random_raster, result_bytes, same_run,  # noqa: F401
                                   show, staircase, stub_cloud_run, stub_opts, stub_run)
from tests.test_dendro_cpu import dn, result_bytes as dendro_bytes, stub_opts as dendro_opts, stub_run as dendro_run  # noqa: F401
from tests.test_ground_cpu import gn, result_bytes as ground_bytes, stub_opts as ground_opts, stub_run as ground_run  # noqa: F401
from tests.test_gpu_segment import _write_pcd
from tests.test_terrain_cpu import (result_bytes as terrain_bytes, stub_opts as terrain_opts, stub_run as terrain_run, tn,  # noqa: F401
                                    transcription_cases as terrain_cases)
from tests.test_trees_cpu import same_run as same_trees, stub_opts as trees_opts, tr  # noqa: F401

pytestmark = pytest.mark.gpu
TILE = crowns.TILE
CLOUD_ARRAYS = ARRAYS + ("tree_of",)


def device_run(Z, c, opts=None, cap=None):
    """The raster entry in the stub's form."""
    labels, smooth, tops, res = crowns.chm_crowns(Z, c, opts, cap)
    return dict(labels=labels, smooth=smooth, tops=tops, res=res)


def assert_equal(cn, Z, c, opts=None, cap=65536):
    """One device call on a raster against the stub: the same bytes.  Returns the device's run."""
    want, got = stub_run(cn, Z, c, opts, cap=cap), device_run(Z, c, opts, cap)
    assert same_run(got, want), (show(got), show(want), [k for k in ARRAYS if got[k].tobytes() != want[k].tobytes()])
    return got


def device_cloud_run(cloud, opts=None, cap=None):
    """The cloud entry in the stub's form, after a terrain call on the handle."""
    tree_of, tops, res = crowns.crowns(cloud, opts, cap)
    smooth, labels = crowns.raster(cloud)
    return dict(labels=labels, smooth=smooth, tree_of=tree_of, tops=tops, res=res)


def assert_cloud_equal(cn, cloud, t, opts, cap=65536):
    """crowns on a handle whose last terrain call is the stub run `t`, against the stubs: the same bytes."""
    want, got = stub_cloud_run(cn, t, opts, cap), device_cloud_run(cloud, opts, cap)
    assert same_run(got, want, CLOUD_ARRAYS), (show(got), show(want), [k for k in CLOUD_ARRAYS if got[k].tobytes() != want[k].tobytes()])
    return got


def terrain_both(tn, cloud, xyz, labels=None, label=0, opts=None):
    """The terrain on the device (kept on the handle) and by its stub, which agree (tests/test_gpu_terrain.py): the stub's run."""
    t = terrain_run(tn, xyz, labels, label, opts)
    is_ground, hag, res = terrain.terrain(cloud, labels, label, opts)
    assert hag.tobytes() == t["hag"].tobytes() and terrain_bytes(res) == terrain_bytes(t["res"])
    return t


def test_tile_and_batch_are_the_headers(cn):
    assert cn.crn_tile() == TILE == 64 and cn.crn_batch() == crowns.BATCH == BATCH


def test_one_cell_one_row_one_column_and_nothing(ctx, cn):
    assert result_bytes(crowns.default_opts()) == result_bytes(stub_opts(cn))
    r = assert_equal(cn, np.full((1, 1), 5.0, np.float32), 0.5)
    assert r["res"].n_trees == 1 and r["labels"][0, 0] == 0 and r["tops"]["cells"][0] == 1
    line = (3.0 + 2.0 * np.sin(np.arange(300) / 9.0)).astype(np.float32)
    line[5::37] = NAN
    r = assert_equal(cn, line[None, :], 0.5)
    assert (r["res"].De, r["res"].Dn) == (300, 1) and r["res"].n_trees >= 2
    r = assert_equal(cn, line[:, None], 0.5)
    assert (r["res"].De, r["res"].Dn) == (1, 300) and r["res"].n_trees >= 2
    for shape in ((0, 0), (0, 7), (3, 0)):
        r = assert_equal(cn, np.zeros(shape, np.float32), 0.5)
        assert r["res"].flags == NO_CANOPY and len(r["tops"]) == 0
    for Z in (np.full((9, 70), NAN), np.full((9, 70), 1.5, np.float32)):
        r = assert_equal(cn, Z, 0.5)
        assert r["res"].flags == NO_CANOPY and r["res"].n_canopy == 0 and (r["labels"] == -1).all()


def seamed(width, seed):
    """A width x (width + 3) raster of rolling heights: empty cells around the corners of the tiles, a peak in each corner of
    the raster and on the tile seams, and a run of equal heights across a seam."""
    rng = np.random.default_rng(seed)
    De, Dn = width, width + 3
    x, y = np.meshgrid(np.arange(De), np.arange(Dn))
    Z = (6.0 + 2.0 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.uniform(0, 0.3, x.shape)).astype(np.float32)
    Z[rng.uniform(size=Z.shape) < 0.05] = NAN
    for cx in (TILE - 1, TILE):
        for cy in (TILE - 1, TILE):
            if cx < De and cy < Dn:
                Z[cy, cx] = NAN
    if De > TILE - 4:
        Z[20, TILE - 4:min(TILE + 4, De)] = 9.5                                       # equal heights across the seam
        Z[40, min(TILE, De - 1)] = Z[41, min(TILE, De) - 1] = 12.0                           # equal peaks on either side of it
    Z[0, 0], Z[0, -1], Z[-1, 0], Z[-1, -1] = 15.0, 14.0, 13.0, 14.0
    return Z


@pytest.mark.parametrize("width", [TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("passes", [0, 1, 2, 64])
def test_tile_edges_and_smoothing_passes(ctx, cn, width, passes):
    Z = seamed(width, 10 * width + passes)
    r = assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=passes))
    assert (r["res"].De, r["res"].Dn) == (width, width + 3) and r["res"].n_trees >= 4
    if passes == 0:
        corners = {0, width - 1, (width + 2) * width, (width + 3) * width - 1}
        assert corners <= set(r["tops"]["cell_id"])


@pytest.mark.parametrize("kw", [dict(r_min=0.1, r_max=0.1, win_a=0.0, win_b=0.0),        # R2 = 2
                                dict(r_min=32.0, r_max=32.0),                            # the cap: 64 cells, R2 = 4096
                                dict(r_min=20.0, r_max=20.0, crown_frac=0.0),            # past every edge of a 65-cell raster
                                dict(r_min=0.6, win_b=1.0, r_max=32.0, max_crown_radius=4.0)])   # a window per height
def test_windows_from_the_least_to_the_cap(ctx, cn, kw):
    Z = seamed(TILE + 1, 77)
    r = assert_equal(cn, Z, 0.5, stub_opts(cn, **kw))
    assert r["tops"]["R2"].min() >= 2 and r["tops"]["R2"].max() <= 4096
    if kw["r_max"] == 0.1:
        assert (r["tops"]["R2"] == 2).all() and r["res"].n_trees > 20
    if kw["r_min"] == 32.0:
        assert (r["tops"]["R2"] == 4096).all()


def test_cap_of_the_window_and_refusals_on_the_device(ctx, cn):
    Z = seamed(TILE - 1, 5)
    for kw in REFUSALS + [dict(r_max=32.1)]:
        assert stub_run(cn, Z, 0.5, stub_opts(cn, **kw)) is None
        with pytest.raises(_lib.SfmHipError):
            crowns.chm_crowns(Z, 0.5, crowns.default_opts(**kw))
    for c in (0.0, -1.0, float("nan")):
        with pytest.raises(_lib.SfmHipError):
            crowns.chm_crowns(Z, c)
    o, res = crowns.default_opts(), crowns.CrownsResult()
    assert _lib.lib().sfmhip_chm_crowns(ctx.h, None, 4097, 4096, 1.0, C.byref(o), None, None, 0, None, C.byref(res)) != 0   # > 2^24 cells


def test_plateau_and_ties_across_a_seam(ctx, cn):
    r = assert_equal(cn, np.full((TILE + 3, 2 * TILE + 1), 7.0, np.float32), 0.5, stub_opts(cn, smooth_passes=0))
    assert (r["res"].n_summits, r["res"].n_trees) == (1, 1) and r["tops"]["cell_id"][0] == 0
    Z = random_raster(21, TILE + 2, 2 * TILE + 5, holes=0.1, levels=5)
    assert assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0))["res"].n_trees > 5
    assert assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=1, r_max=3.0))["res"].n_trees > 1


def spiral(side=65):
    """A ridge one cell wide that winds from the raster's corner to its middle, rising all the way, with furrows of low canopy
    one cell wide between its turns: the ascent from the corner follows the whole ridge.  (Z, the ridge's length)."""
    Z = np.full((side, side), 2.5, np.float32)
    on = np.zeros((side, side), bool)
    x, y, dx, dy, steps = 0, 0, 1, 0, 0

    def free(px, py):
        return 0 <= px < side and 0 <= py < side and not on[py, px]

    while True:
        on[y, x] = True
        steps += 1
        Z[y, x] = 3.0 + 0.01 * steps
        for _ in range(2):
            ahead_clear = not (0 <= x + 2 * dx < side and 0 <= y + 2 * dy < side) or not on[y + 2 * dy, x + 2 * dx]
            if free(x + dx, y + dy) and ahead_clear:
                break
            dx, dy = -dy, dx                                                          # turn clockwise (y grows downwards)
        else:
            return Z, steps
        x, y = x + dx, y + dy


def test_ascent_longer_than_a_batch_of_doubling_rounds(ctx, cn):
    """A chain of m cells takes ceil(log2 m) rounds: 4 097 cells and the spiral's ridge take more than the BATCH rounds of one
    read-back."""
    ramp = (3.0 + np.arange(4097) * 0.001).astype(np.float32)[None, :]
    r = assert_equal(cn, ramp, 1.0, flat_opts(cn, 2))
    assert (r["res"].n_summits, r["res"].n_trees) == (1, 1) and r["tops"]["cell_id"][0] == 4096 and (r["labels"] == 0).all()
    assert 4096 > 2 ** BATCH
    r = assert_equal(cn, ramp[:, ::-1].T.copy(), 1.0, flat_opts(cn, 2))
    assert r["tops"]["cell_id"][0] == 0 and r["res"].n_labelled_cells == 4097
    Z, steps = spiral()
    r = assert_equal(cn, Z, 1.0, flat_opts(cn, 1.5))
    assert steps > 1000 and r["res"].n_summits == 1 and (r["labels"] == 0).all()              # the corner climbs to the middle


def test_parent_chain_longer_than_a_batch_of_doubling_rounds(ctx, cn):
    r = assert_equal(cn, staircase(41), 1.0, flat_opts(cn, 3))
    assert (r["res"].n_summits, r["res"].n_trees, r["res"].max_depth) == (41, 1, 40) and 40 > 2 ** BATCH and (r["labels"] == 0).all()
    r = assert_equal(cn, np.repeat(staircase(41), 3, axis=0), 1.0, flat_opts(cn, 3))
    assert r["res"].n_trees == 1 and r["res"].max_depth >= 40


def test_max_trees_of_one_overflow_and_a_short_table(ctx, cn):
    Z = seamed(TILE, 3)
    full = assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0))
    n = full["res"].n_trees
    assert n > 4
    r = assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0, max_trees=1))
    assert r["res"].n_trees == n and r["res"].flags == OVERFLOW and len(r["tops"]) == 1 and set(np.unique(r["labels"])) == {-1, 0}
    r = assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0, max_trees=n - 1))
    assert r["res"].flags == OVERFLOW and len(r["tops"]) == n - 1
    assert assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0, max_trees=n))["res"].flags == 0
    r = assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0), cap=3)                 # cap < n_trees: three rows, nothing else changes
    assert len(r["tops"]) == 3 and r["res"].n_trees == n and r["labels"].tobytes() == full["labels"].tobytes()
    assert len(assert_equal(cn, Z, 0.5, stub_opts(cn, smooth_passes=0), cap=0)["tops"]) == 0


# ---------------------------------------------------------------- the cloud entry
def test_before_any_terrain_call_and_with_nothing_selected(ctx, cn, tn):
    xyz, member = scene(1, APART, n_ground=3000, per=600)
    with Cloud(xyz) as c:
        with pytest.raises(_lib.SfmHipError):
            crowns.crowns(c)
        with pytest.raises(_lib.SfmHipError):
            crowns.raster(c)
        lab = np.zeros(len(xyz), np.int32)
        t = terrain_both(tn, c, xyz, lab, 1, terrain_opts(tn))                        # nobody has label 1
        r = assert_cloud_equal(cn, c, t, stub_opts(cn))
        assert r["res"].flags == NO_CANOPY and (r["res"].De, r["res"].Dn) == (0, 0) and (r["tree_of"] == -1).all() and len(r["tree_of"]) == len(xyz)
        with pytest.raises(_lib.SfmHipError):
            terrain.terrain(c, opts=terrain.default_opts(cell=1e-3))                  # a raster over its cap: the call leaves nothing to work on
        with pytest.raises(_lib.SfmHipError):
            crowns.crowns(c)


@pytest.mark.parametrize("name", ["plain", "labels", "nan", "rot_scale"])
def test_labels_nan_points_a_rotated_frame_and_a_scale(ctx, cn, tn, gn, name):
    xyz, lab, label, o = terrain_cases(tn, gn)[name]
    with Cloud(xyz) as c:
        t = terrain_both(tn, c, xyz, lab, label, o)
        r = assert_cloud_equal(cn, c, t, stub_opts(cn, scale=o.scale))
    assert r["res"].n_trees >= 1 and r["res"].n_labelled > 0 and (r["tree_of"][np.isnan(t["hag"])] == -1).all()
    assert r["res"].n_labelled == (r["tree_of"] >= 0).sum() == r["tops"]["points"].sum()


def test_two_calls_other_options_another_cell_and_the_handle_shared(ctx, cn, tn, tr):
    """crowns twice, with other options, after a second terrain call with another cell, and around trees and dendrometry calls on
    one handle: each gives what it gives alone."""
    xyz, member = scene(2, TOUCHING, n_ground=8000, per=1500)
    with Cloud(xyz) as c:
        t = terrain_both(tn, c, xyz, opts=terrain_opts(tn))
        a = assert_cloud_equal(cn, c, t, stub_opts(cn))
        b = assert_cloud_equal(cn, c, t, stub_opts(cn))
        assert same_run(a, b, CLOUD_ARRAYS) and a["res"].n_trees == 5
        assert_cloud_equal(cn, c, t, stub_opts(cn, smooth_passes=0, crown_frac=0.8, ground_clear=9.0, max_trees=2))
        assert_cloud_equal(cn, c, t, stub_opts(cn), cap=2)
        t2 = terrain_both(tn, c, xyz, opts=terrain_opts(tn, cell=0.2))                # a larger raster
        assert_cloud_equal(cn, c, t2, stub_opts(cn, smooth_passes=1))
        t3 = terrain_both(tn, c, xyz, opts=terrain_opts(tn, cell=1.5))                # a smaller one
        assert_cloud_equal(cn, c, t3, stub_opts(cn))
        t = terrain_both(tn, c, xyz, opts=terrain_opts(tn))
        topts = trees.default_opts(ground=0.0)
        s1 = trees.trees(c, None, 0, topts)
        d1 = dendro.measure(c, a["tree_of"], 0, dendro.default_opts(ground=0.0))
        again = assert_cloud_equal(cn, c, t, stub_opts(cn))
        assert same_run(again, a, CLOUD_ARRAYS)
        assert same_trees(trees.trees(c, None, 0, topts), s1)
        assert dendro_bytes(dendro.measure(c, a["tree_of"], 0, dendro.default_opts(ground=0.0))) == dendro_bytes(d1)
        dtm, kind, chm = terrain.raster(c)                                            # the terrain's rasters are as the call left them
        assert chm.tobytes() == t["chm"].tobytes() and dtm.tobytes() == t["dtm"].tobytes()


@pytest.mark.parametrize("cell,passes", [(0.5, 2), (0.25, 2), (0.1, 0)])
@pytest.mark.parametrize("name", ["apart", "touching"])
def test_planted_scenes(ctx, cn, tn, name, cell, passes):
    trees_ = APART if name == "apart" else TOUCHING
    xyz, member = scene(1, trees_)
    with Cloud(xyz) as c:
        t = terrain_both(tn, c, xyz, opts=terrain_opts(tn, cell=cell))
        r = assert_cloud_equal(cn, c, t, stub_opts(cn, smooth_passes=passes))
    assert r["res"].n_trees == len(trees_) == len(r["tops"]) and (r["tree_of"][member < 0] == -1).all()
    if cell == 0.1:
        assert r["res"].n_summits > 50 and r["res"].max_depth >= 2


def stub_chain(cn, tn, gn, dn, xyz, scale):
    """The inventory by the four stubs: (ground, terrain run, crowns run, [dendro result per crown])."""
    g = ground_run(gn, xyz, opts=ground_opts(gn, inlier_tol=0.5 / scale))
    assert g.flags == 0
    o = terrain_opts(tn, scale=scale)
    assert tn.ter_opts_from_ground(C.byref(g), C.byref(o)) == 0
    t = terrain_run(tn, xyz, opts=o)
    run = stub_cloud_run(cn, t, stub_opts(cn, scale=scale))
    d = dendro_opts(dn, scale=scale, ground=0.0)
    return g, t, run, [dendro_run(dn, t["norm"], run["tree_of"], j, d)[0] for j in range(len(run["tops"]))]


def rotated_scene():
    from tests.test_dendro_cpu import rotation
    scale = 0.37
    xyz, member = scene(3, APART)
    return ((xyz.astype(np.float64) @ rotation(12).T) / scale).astype(np.float32), member, scale


def test_inventory_equals_the_chain_of_the_stubs(ctx, cn, tn, gn, dn):
    xyz, member, scale = rotated_scene()
    g, t, run, per_tree = stub_chain(cn, tn, gn, dn, xyz, scale)
    with Cloud(xyz) as c:
        got = crowns.inventory(c, ground.default_opts(inlier_tol=0.5 / scale), None, terrain.default_opts(scale=scale),
                               crowns.default_opts(scale=scale), dendro.default_opts(scale=scale))
    assert ground_bytes(got[0]) == ground_bytes(g) and got[2].tobytes() == t["hag"].tobytes() and terrain_bytes(got[3]) == terrain_bytes(t["res"])
    assert got[4].tobytes() == run["tree_of"].tobytes() and got[5].tobytes() == run["tops"].tobytes() and result_bytes(got[6]) == result_bytes(run["res"])
    assert got[6].n_trees == 6 == len(got[7])
    heights = sorted(ht for _, _, ht, _ in APART)
    for j in range(6):
        assert dendro_bytes(got[7][j]) == dendro_bytes(per_tree[j])
    assert np.allclose(sorted(d.total_height for d in got[7]), heights, atol=0.25)


def test_host_mirror_selftest_crowns(ctx, cn, tn, gn, dn, tmp_path):
    """sfm_dendro_selftest --crowns on a PCD of the rotated scene, brought to metres, prints six trees and writes the chain's bytes."""
    exe = build.build_dendro_demo()
    xyz, member, scale = rotated_scene()
    xyz = (xyz.astype(np.float64) * scale).astype(np.float32)
    pcd, out = str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, np.full(len(xyz), 0x00406020, np.uint32))
    r = subprocess.run([exe, pcd, out, "--crowns=0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Crowns=6 ") for ln in lines) and sum(ln.startswith("Tree ") for ln in lines) == 6, r.stdout[-2000:]
    g, t, run, per_tree = stub_chain(cn, tn, gn, dn, xyz, 1.0)
    want = (np.int32(6).tobytes() + run["tops"].tobytes() + b"".join(dendro_bytes(d) for d in per_tree) + run["tree_of"].tobytes()
            + result_bytes(run["res"]) + terrain_bytes(t["res"]))
    raw = open(out, "rb").read()
    assert len(raw) == len(want) and raw == want
