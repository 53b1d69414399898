"""GPU: the terrain model (csrc/terrain.hip) against the g++ build of the same header
(tests/stub/terrain_capi.cpp), byte for byte: is_ground, hag, the three rasters, every field of the result and the normalised
cloud's download.  The shapes are the smallest at which the kernels can go wrong: 1 and 3 points, nothing selected, a one-row
and a one-column raster, rasters of TILE - 1, TILE and TILE + 1 cells a side with empty cells at the tile corners under
windows of half-width 1, TILE - 1, TILE, TILE + 1 and wider than the raster, holes that need more than one batch of fill
rounds and more rounds than there are, cells of 1, 64, 65 and 4 097 points, labels, NaN points, a rotated frame and a scale,
the raster's cap and the refusals, the handle called twice, with other options and shared with the other cloud calls; then a
planted scene of 1.2 x 10^5 points, the plot inventory against the chain of the stubs, and the host mirror's self-test with
--terrain."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, dendro, ground, terrain, trees
from sfm_danpipeline_amd.cloud import Cloud
from tests.terrain_scenes import CENTRES, scene
from tests.test_dendro_cpu import dn, result_bytes as dendro_bytes, stub_opts as dendro_opts, stub_run as dendro_run  # noqa: F401
from tests.test_ground_cpu import gn, result_bytes as ground_bytes, stub_opts as ground_opts, stub_run as ground_run  # noqa: F401
from tests.test_gpu_segment import _write_pcd
from tests.test_terrain_cpu import (ARRAYS, NO_WINDOW, NONE_SELECTED, REFUSALS, UNFILLED, at, result_bytes, ring_with_a_hole, same_run,  # noqa: F401
                                    show, stub_opts, stub_run, tn, transcription_cases)
from tests.test_trees_cpu import same_run as same_trees, stub_opts as trees_opts, stub_run as trees_run, tr  # noqa: F401

pytestmark = pytest.mark.gpu
TILE = terrain.TILE


def device_run(cloud, labels=None, label=0, opts=None):
    """One device call in the stub's form: the per-point outputs, the rasters, the normalised cloud's download, the result."""
    is_ground, hag, res = terrain.terrain(cloud, labels, label, opts)
    dtm, kind, chm = terrain.raster(cloud)
    with terrain.normalize(cloud) as nc:
        assert nc.n == cloud.n
        norm = nc.download()
    return dict(is_ground=is_ground, hag=hag, norm=norm, dtm=dtm, kind=kind, chm=chm, res=res)


def assert_equal(tn, xyz, labels=None, label=0, opts=None, cloud=None):
    """One device call against the stub: the same bytes.  Returns the device's run."""
    if cloud is None:
        with Cloud(xyz) as c:
            return assert_equal(tn, xyz, labels, label, opts, c)
    want = stub_run(tn, xyz, labels, label, opts)
    got = device_run(cloud, labels, label, opts)
    assert same_run(got, want), (show(got), show(want), [k for k in ARRAYS if got[k].tobytes() != want[k].tobytes()])
    return got


def test_tile_width_is_the_headers(tn):
    assert tn.ter_tile() == TILE == 64


def test_one_point_three_points_and_nothing_selected(ctx, tn):
    r = assert_equal(tn, at((1, 2, 3)))
    assert (r["res"].De, r["res"].Dn, r["res"].n_ground) == (1, 1, 1) and r["hag"][0] == 0
    r = assert_equal(tn, at((0, 0, 1.0), (0.1, 0.2, 1.25), (0.3, 0.1, 5.0)))
    assert list(r["is_ground"]) == [1, 0, 0] and list(r["hag"]) == [0.0, 0.25, 4.0]
    pts = at((0, 0, 0), (1, 1, 1))
    r = assert_equal(tn, pts, np.zeros(2, np.int32), 1)
    assert r["res"].flags == NONE_SELECTED and r["dtm"].shape == (0, 0) and np.isnan(r["norm"]).all()
    assert assert_equal(tn, at((np.nan, 0, 0), (0, np.inf, 1)))["res"].flags == NONE_SELECTED


def test_one_row_and_one_column_raster(ctx, tn):
    rng = np.random.default_rng(8)
    row = np.column_stack([rng.uniform(0, 40, 300), rng.uniform(0, 0.4, 300), rng.normal(0, 0.05, 300)]).astype(np.float32)
    row[:2, :2] = (0, 0), (39.9, 0.45)
    row[::7, 2] += 3.0
    r = assert_equal(tn, row)
    assert (r["res"].De, r["res"].Dn) == (80, 1) and 0 < r["res"].n_ground < 300
    r = assert_equal(tn, row[:, [1, 0, 2]])
    assert (r["res"].De, r["res"].Dn) == (1, 80)


def lattice(width, seed, cell=0.5):
    """A point in most cells of a width x (width + 3) raster, none in the cells around the corners of the opening's
    tiles, heights that undulate with spikes: every cell of the opened rasters depends on its whole window."""
    rng = np.random.default_rng(seed)
    De, Dn = width, width + 3
    x, y = np.meshgrid(np.arange(De), np.arange(Dn))
    keep = rng.uniform(size=x.shape) < 0.7
    for cx in (TILE - 1, TILE):
        for cy in (TILE - 1, TILE):
            if cx < De and cy < Dn:
                keep[cy, cx] = False
    keep[0, 5] = keep[5, 0] = keep[Dn - 1, 7] = keep[7, De - 1] = True              # the raster keeps its size
    x, y = x[keep], y[keep]
    h = np.sin(x / 9.0) + np.cos(y / 7.0) + rng.normal(0, 0.05, len(x)) + 4.0 * (rng.uniform(size=len(x)) < 0.1)
    pts = np.column_stack([(x + rng.uniform(0.1, 0.9, len(x))) * cell, (y + rng.uniform(0.1, 0.9, len(x))) * cell, h])
    pts[(x == 0) & (y == 5), 0], pts[(x == 5) & (y == 0), 1] = 0.0, 0.0
    return pts.astype(np.float32), (De, Dn)


def one_window(tn, k, cell=0.5, **kw):
    """Options whose table holds exactly the window of half-width k."""
    if k == 1:
        return stub_opts(tn, cell=cell, exponential=1, base=1000, max_window=3 * cell, **kw)
    return stub_opts(tn, cell=cell, exponential=0, base=k, max_window=(2 * k + 1) * cell, **kw)


@pytest.mark.parametrize("width", [TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("k", [1, TILE - 1, TILE, TILE + 1, 3 * TILE])
def test_windows_at_the_tile_edges(ctx, tn, width, k):
    pts, (De, Dn) = lattice(width, 100 * width + k)
    r = assert_equal(tn, pts, opts=one_window(tn, k, slope=0.05, max_distance=0.5))
    assert (r["res"].De, r["res"].Dn, r["res"].n_windows) == (De, Dn, 1) and 0 < r["res"].n_ground < len(pts)


def test_every_window_of_a_table_and_two_tiles_a_side(ctx, tn):
    pts, (De, Dn) = lattice(2 * TILE + 5, 7)
    r = assert_equal(tn, pts, opts=stub_opts(tn, max_window=80.0, slope=0.3))
    assert r["res"].n_windows == 7 and (r["res"].De, r["res"].Dn) == (De, Dn)
    assert assert_equal(tn, pts, opts=stub_opts(tn, max_window=1.0))["res"].flags & NO_WINDOW


def test_holes_across_the_fill_batches(ctx, tn):
    # 20 empty rings inside a ring of ground: more than one batch of 16 rounds; and a point high above the third ring
    pts = np.concatenate([ring_with_a_hole(41)[:-1], at((1.95, 1.95, 20.0))])
    r = assert_equal(tn, pts)
    assert r["res"].fill_rounds == 21 and r["res"].n_kind0 == 0 and r["res"].n_kind2 == 39 * 39 and r["is_ground"][-1] == 0
    for rounds, left in ((2, 35), (3, 33), (16, 7), (17, 5), (20, 0), (0, 39)):
        r = assert_equal(tn, pts, opts=stub_opts(tn, fill_rounds=rounds))
        assert r["res"].fill_rounds == rounds and r["res"].n_kind0 == left * left and bool(r["res"].flags & UNFILLED) == (left > 0)
        assert np.isnan(r["hag"][-1]) == (rounds < 3)
    assert_equal(tn, pts, opts=stub_opts(tn, relax_sweeps=0))
    assert_equal(tn, pts, opts=stub_opts(tn, relax_sweeps=1))
    assert_equal(tn, ring_with_a_hole(21), opts=stub_opts(tn, fill_rounds=3))          # a kind-0 corner in a stencil


def test_cells_of_1_64_65_and_4097_points(ctx, tn):
    rng = np.random.default_rng(9)
    parts = []
    for j, m in enumerate((1, 64, 65, 4097)):
        p = np.column_stack([rng.uniform(0.05, 0.45, m) + 1.0 * (j + 1), rng.uniform(0.05, 0.45, m), 1e3 + rng.uniform(0, 0.1, m)])
        parts.append(p)
    pts = np.concatenate(parts)
    pts = pts[rng.permutation(len(pts))]
    pts = np.concatenate([[[0.0, 0.0, 1e3]], pts]).astype(np.float32)                 # (the raster's origin: a cell of 1 too)
    r = assert_equal(tn, pts)
    assert r["res"].n_ground == len(pts) and r["res"].n_kind1 == 5 and (r["res"].De, r["res"].Dn) == (9, 1)
    assert sorted(np.bincount((pts[:, 0].astype(np.float64) / 0.5).astype(int))[[0, 2, 4, 6, 8]]) == [1, 1, 64, 65, 4097]
    lab = (np.arange(len(pts)) % 3).astype(np.int32)
    assert 0 < assert_equal(tn, pts, lab, 1)["res"].n_ground < len(pts)


@pytest.mark.parametrize("name", ["plain", "labels", "nan", "rot_scale"])
def test_labels_nan_points_a_rotated_frame_and_a_scale(ctx, tn, gn, name):
    xyz, lab, label, o = transcription_cases(tn, gn)[name]
    assert assert_equal(tn, xyz, lab, label, o)["res"].flags == 0


@pytest.mark.parametrize("kw", REFUSALS)
def test_refusals_on_the_device(ctx, tn, kw):
    pts = at((0, 0, 0), (1, 1, 1))
    assert stub_run(tn, pts, opts=stub_opts(tn, **kw)) is None
    with pytest.raises(_lib.SfmHipError), Cloud(pts) as c:
        terrain.terrain(c, opts=terrain.default_opts(**kw))


def test_the_cap_of_the_raster_and_raster_before_any_call(ctx, tn):
    assert result_bytes(terrain.default_opts()) == result_bytes(stub_opts(tn))
    over = at((0, 0, 0), (4096, 4095, 0))
    assert stub_run(tn, over, opts=stub_opts(tn, cell=1.0)) is None
    with Cloud(over) as c:
        with pytest.raises(_lib.SfmHipError):
            terrain.raster(c)                                                         # no call yet
        with pytest.raises(_lib.SfmHipError):
            terrain.normalize(c)
        with pytest.raises(_lib.SfmHipError):
            terrain.terrain(c, opts=terrain.default_opts(cell=1.0))
        with pytest.raises(_lib.SfmHipError):
            terrain.raster(c)                                                         # a refused call leaves no rasters
    o = stub_opts(tn, cell=1.0, fill_rounds=1, relax_sweeps=0, max_window=3.0)
    r = assert_equal(tn, at((0, 0, 0), (4095, 4095, 0)), opts=o)                      # 2^24 cells
    assert r["res"].De * r["res"].Dn == 1 << 24 and r["res"].n_kind2 == 6


def test_two_calls_other_options_and_the_handle_shared(ctx, tn, tr, gn):
    """terrain twice, with other options, and before and after ground_plane and trees on one handle: each gives what it gives alone."""
    xyz, member, _, _ = scene(3, n_tree=1500, n_ground=6000)
    topts = trees_opts(tr, ground=-1.0)
    with Cloud(xyz) as c:
        a = assert_equal(tn, xyz, opts=stub_opts(tn), cloud=c)
        b = assert_equal(tn, xyz, opts=stub_opts(tn), cloud=c)
        assert same_run(a, b)
        assert_equal(tn, xyz, opts=stub_opts(tn, cell=0.2, fill_rounds=2), cloud=c)   # a larger raster, holes left
        assert_equal(tn, xyz, opts=stub_opts(tn, cell=1.5, exponential=0), cloud=c)   # a smaller one
        g1 = ground.ground_plane(c, opts=ground.default_opts(inlier_tol=0.5))
        t1 = trees.trees(c, None, 0, topts)
        assert same_run(assert_equal(tn, xyz, opts=stub_opts(tn), cloud=c), a)
        assert_equal(tn, xyz, (member == 2).astype(np.int32), 0, stub_opts(tn), cloud=c)
        assert ground_bytes(ground.ground_plane(c, opts=ground.default_opts(inlier_tol=0.5))) == ground_bytes(g1)
        assert same_trees(trees.trees(c, None, 0, topts), t1) and same_trees(t1, trees_run(tr, xyz, opts=topts))


def big_scene():
    scale = 0.37
    xyz, member, above, _ = scene(1, 1.0, 0.25, n_tree=16000, n_ground=44000, rot=12, scale=scale)
    return xyz, member, scale


def stub_chain(tn, tr, gn, dn, xyz, scale):
    """The inventory by the four stubs: (ground, terrain run, trees run, [dendro result per tree])."""
    g = ground_run(gn, xyz, opts=ground_opts(gn, inlier_tol=0.5 / scale))
    assert g.flags == 0
    o = stub_opts(tn, scale=scale)
    assert tn.ter_opts_from_ground(C.byref(g), C.byref(o)) == 0
    t = stub_run(tn, xyz, opts=o)
    tt = trees_run(tr, t["norm"], opts=trees_opts(tr, scale=scale, ground=0.0))
    d = dendro_opts(dn, scale=scale, ground=0.0)
    return g, t, tt, [dendro_run(dn, t["norm"], tt[0], s, d)[0] for s in range(tt[2].n_trees)]


def test_planted_scene_and_inventory_equal_the_chain_of_the_stubs(ctx, tn, tr, gn, dn):
    xyz, member, scale = big_scene()
    assert 1.1e5 < len(xyz) < 1.3e5
    g, t, tt, per_tree = stub_chain(tn, tr, gn, dn, xyz, scale)
    with Cloud(xyz) as c:
        got = terrain.inventory(c, ground.default_opts(inlier_tol=0.5 / scale), None, terrain.default_opts(scale=scale),
                                trees.default_opts(scale=scale), dendro.default_opts(scale=scale))
        again = device_run(c, opts=terrain.opts_from_ground(got[0], terrain.default_opts(scale=scale)))
    assert ground_bytes(got[0]) == ground_bytes(g) and same_run(again, t)
    assert got[1].tobytes() == t["is_ground"].tobytes() and got[2].tobytes() == t["hag"].tobytes() and result_bytes(got[3]) == result_bytes(t["res"])
    assert same_trees(got[4:7], tt) and got[6].n_trees == len(CENTRES) == len(got[7])
    for s in range(len(CENTRES)):
        assert dendro_bytes(got[7][s]) == dendro_bytes(per_tree[s]) and abs(per_tree[s].dbh - 0.3) < 0.02
    assert not t["is_ground"][member >= 0].all() and t["is_ground"][member < 0].mean() > 0.8


def test_host_mirror_selftest_terrain(ctx, tn, tr, gn, dn, tmp_path):
    """sfm_dendro_selftest --terrain on a PCD of the rotated scene, brought to metres, prints five trees and writes the chain's bytes."""
    exe = build.build_dendro_demo()
    xyz, member, scale = big_scene()
    xyz = (xyz.astype(np.float64) * scale).astype(np.float32)
    pcd, out = str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, np.full(len(xyz), 0x00406020, np.uint32))
    r = subprocess.run([exe, pcd, out, "--terrain=0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert "Trees=5" in lines and sum(ln.startswith("Tree ") for ln in lines) == 5, r.stdout[-2000:]
    g, t, tt, per_tree = stub_chain(tn, tr, gn, dn, xyz, 1.0)
    n = len(xyz)
    want = (np.int32(5).tobytes() + tt[1].tobytes() + b"".join(dendro_bytes(d) for d in per_tree) + tt[0].tobytes()
            + result_bytes(t["res"]) + t["is_ground"].tobytes() + t["hag"].tobytes())
    raw = open(out, "rb").read()
    assert len(raw) == len(want) and raw[-8 * n:] == want[-8 * n:] and raw == want
