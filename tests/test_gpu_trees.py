"""GPU: the individual-tree extraction (csrc/trees.hip) against the g++ build of the same header
(tests/stub/trees_capi.cpp), byte for byte: tree_of, every stem row and every field of the result.  The shapes are the smallest
at which the kernels can go wrong: 1 and 3 points, poles that need one and many batches of sweeps, columns of 257 and 1 025
voxels, touching crowns, the four-tree plot at 12 000 and 120 000 points, the rule cases, labels, NaN points, a rotated frame,
the flags, the refusals and the caps, a short stem table, the handle shared with the other cloud calls; then the plot
inventory against the chain of the three stubs, and the host mirror's self-test with --plot."""
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, dendro, ground, segment, trees
from sfm_danpipeline_amd.cloud import Cloud
from tests.test_dendro_cpu import dn, result_bytes as dendro_bytes, stub_opts as dendro_opts, stub_run as dendro_run  # noqa: F401
from tests.test_ground_cpu import TOL, gn, result_bytes as ground_bytes, stub_opts as ground_opts, stub_run as ground_run  # noqa: F401
from tests.test_gpu_segment import _write_pcd
from tests.test_gpu_segment import scene as colour_scene
from tests.test_trees_cpu import (ISLAND, NO_STEM, NONE_ABOVE, REFUSALS, SQUARE3, SQUARE5, TIE, TOO_MANY, TWO_TOUCHING, at, column,  # noqa: F401
                                  framed_opts, lattice_opts, plot, pole, result_bytes, same_run, show, stub_opts, stub_run, tr,
                                  transcription_cases)

pytestmark = pytest.mark.gpu


def assert_equal(tr, xyz, labels=None, label=0, opts=None, cloud=None, cap=trees.MAX_TREES):
    """One device call against the stub: the same bytes.  Returns the device's (tree_of, stems, result)."""
    if cloud is None:
        with Cloud(xyz) as c:
            return assert_equal(tr, xyz, labels, label, opts, c, cap)
    want = stub_run(tr, xyz, labels, label, opts, cap=cap)
    got = trees.trees(cloud, labels, label, opts, cap)
    assert same_run(got, want), (show(got), show(want), int((got[0] != want[0]).sum()))
    return got


def test_one_point_and_three_below(ctx, tr):
    tree_of, stems, res = assert_equal(tr, at((0, 0, 0)), opts=lattice_opts(tr))
    assert list(tree_of) == [0] and res.n_trees == 1 and res.n_voxels == 1 and stems[0]["points"] == 1
    res = assert_equal(tr, at((0, 0, 0), (1, 0, 0), (0, 1, 0)), opts=lattice_opts(tr, ground=3.0))[2]
    assert res.flags == NONE_ABOVE and res.n_selected == 3


@pytest.mark.parametrize("n,height", [(300, 3.0), (4000, 20.0)])
def test_poles(ctx, tr, n, height):
    """300 points: fewer voxel levels than a batch of 16 sweeps; the 20-long pole: more than several batches."""
    p = pole(n, height)
    with Cloud(p) as c:
        tree_of, stems, res = assert_equal(tr, p, opts=stub_opts(tr, ground=0.0, min_stem_pts=10), cloud=c)
        sweeps = trees.last_timing(c)["n_sweeps"]
    assert res.n_trees == 1 and res.n_labelled == int((p[:, 2].astype(np.float64) >= 0.3).sum()) and sweeps % 16 == 0 and sweeps >= 16
    if height == 20.0:
        assert abs(res.max_cost - 1234) <= 17


@pytest.mark.parametrize("nv", [257, 1025])
def test_columns_of_voxels(ctx, tr, nv):
    """One voxel past a workgroup of 256, and past four: a chain that long needs the sweeps to go on past many batches."""
    tree_of, _, res = assert_equal(tr, column(nv), opts=lattice_opts(tr))
    assert res.n_voxels == nv and res.max_cost == 10 * (nv - 1) and (tree_of == 0).all()


def test_two_trees_touching_at_3000_points(ctx, tr):
    xyz, _, _ = plot(31, TWO_TOUCHING, n_tree=1000, n_ground=1000)
    assert assert_equal(tr, xyz, opts=stub_opts(tr, ground=0.0, min_stem_pts=10, stem_cell=0.1, voxel=0.3))[2].n_trees == 2


@pytest.mark.parametrize("n_tree,n_ground,cell", [(2000, 4000, 0.1), (20000, 40000, 0.05)])
def test_four_tree_plot(ctx, tr, n_tree, n_ground, cell):
    xyz, _, _ = plot(20, SQUARE5, n_tree=n_tree, n_ground=n_ground)
    with Cloud(xyz) as c:
        a = assert_equal(tr, xyz, opts=stub_opts(tr, ground=0.0, stem_cell=cell), cloud=c)
        b = assert_equal(tr, xyz, opts=stub_opts(tr, ground=0.0, stem_cell=cell), cloud=c)       # two calls in a row: the same bytes
        assert same_run(a, b) and a[2].n_trees == 4 and a[2].flags == 0
        assert_equal(tr, xyz, opts=stub_opts(tr, ground=0.0, voxel=0.3, stem_cell=0.2), cloud=c)  # other grids on the same handle
        assert len(assert_equal(tr, xyz, opts=stub_opts(tr, ground=0.0, stem_cell=cell), cloud=c, cap=3)[1]) == 3  # a table shorter than T
        assert len(assert_equal(tr, xyz, opts=stub_opts(tr, ground=0.0, stem_cell=cell), cloud=c, cap=0)[1]) == 0


def test_rule_cases_on_the_device(ctx, tr):
    assert list(assert_equal(tr, TIE, opts=lattice_opts(tr))[0]) == [0, 1, 0, 0, 0, 1, 1]
    assert list(assert_equal(tr, ISLAND, opts=lattice_opts(tr))[0]) == [0, 0, -1]
    col = column(5)
    assert list(assert_equal(tr, col, opts=lattice_opts(tr, max_path=3.0))[0]) == [0, 0, 0, 0, -1]
    assert list(assert_equal(tr, col, opts=lattice_opts(tr, max_path=2.9))[0]) == [0, 0, 0, -1, -1]
    three = np.concatenate([at((0, 0, 0))] * 3 + [at((0, 0, 1))])
    for kw in (dict(min_cell_pts=3), dict(min_cell_pts=4), dict(min_stem_pts=3), dict(min_stem_pts=4)):
        assert_equal(tr, three, opts=lattice_opts(tr, **kw))
    wide = at((0, 0, 0), (1, 1, 0), (2, 0, 0))
    assert assert_equal(tr, wide, opts=lattice_opts(tr, max_stem_width=3.0))[2].n_trees == 1
    assert assert_equal(tr, wide, opts=lattice_opts(tr, max_stem_width=2.9))[2].flags == NO_STEM
    assert assert_equal(tr, wide[:, [1, 0, 2]], opts=lattice_opts(tr, max_stem_width=2.9))[2].flags == NO_STEM


def test_the_three_flags(ctx, tr):
    three = at((0, 0, 0), (3, 0, 0), (6, 0, 0), (6, 0, 1))
    tree_of, stems, res = assert_equal(tr, three, opts=lattice_opts(tr, max_trees=2))
    assert res.flags == TOO_MANY and list(tree_of) == [0, 1, -1, -1] and len(stems) == 2
    assert assert_equal(tr, three, opts=lattice_opts(tr, band_lo=2.0, band_hi=3.0))[2].flags == NO_STEM
    assert assert_equal(tr, three, opts=lattice_opts(tr, ground=5.0))[2].flags == NONE_ABOVE
    assert assert_equal(tr, three, np.zeros(4, np.int32), 1, lattice_opts(tr))[2].flags == NONE_ABOVE
    assert result_bytes(trees.default_opts(ground=0.0)) == result_bytes(stub_opts(tr, ground=0.0))


@pytest.mark.parametrize("name", ["rot_037", "labels", "nan"])
def test_labels_nan_points_and_a_rotated_frame(ctx, tr, gn, name):
    xyz, lab, label, o = transcription_cases(tr, gn)[name]
    assert assert_equal(tr, xyz, lab, label, o)[2].flags == 0


@pytest.mark.parametrize("kw", REFUSALS)
def test_refusals_on_the_device(ctx, tr, kw):
    base = dict(ground=0.0)
    base.update(kw)
    assert stub_run(tr, column(3), opts=stub_opts(tr, **base)) is None
    with pytest.raises(_lib.SfmHipError), Cloud(column(3)) as c:
        trees.trees(c, opts=trees.default_opts(**base))


def test_both_grid_caps_on_the_device(ctx, tr):
    for pts in (at((0, 0, 0), (4096, 4095, 0)), at((0, 0, 0), (1023, 1023, 2047))):
        assert stub_run(tr, pts, opts=lattice_opts(tr)) is None
        with pytest.raises(_lib.SfmHipError), Cloud(pts) as c:
            trees.trees(c, opts=lattice_opts(tr))
    assert assert_equal(tr, at((0, 0, 0), (1023, 1023, 2046)), opts=lattice_opts(tr))[2].n_voxels == 2    # keys up to 2^31 - 2^20


def test_handle_shared_with_the_other_cloud_calls(ctx, tr, gn, dn):
    """trees before and after ground_plane, dendrometry and segment_rgb on one handle: each gives what it gives alone."""
    xyz, rgb = colour_scene(8000, 3)
    o = stub_opts(tr, ground=0.9, ground_clear=0.0, band_lo=0.0, band_hi=0.5, min_stem_pts=5, min_cell_pts=1, stem_cell=0.1, voxel=0.2,
                  max_stem_width=10.0)                                   # the patch scene is one slab at z = 0.95 .. 1: one wide "stem"
    dopts = dendro.default_opts(up=(1, 0, 0), slice=0.02, scale=0.2, min_slice_pts=5)
    with Cloud(xyz) as c:
        first = assert_equal(tr, xyz, opts=o, cloud=c)                                           # before any other call
        assert first[2].n_trees == 1 and first[2].n_labelled > 7000
        g1 = ground.ground_plane(c, opts=ground.default_opts(min_inliers=50))
        labels, nc, _ = segment.segment_rgb(c, rgb, c.passthrough(2, 0.0, 14.0), segment.default_opts(min_cluster_size=100))
        d1 = dendro.measure(c, labels, 0, dopts)
        again = assert_equal(tr, xyz, opts=o, cloud=c)                                           # ... and after them
        assert same_run(first, again)
        assert_equal(tr, xyz, labels, 0, o, cloud=c)
        assert ground_bytes(ground.ground_plane(c, opts=ground.default_opts(min_inliers=50))) == ground_bytes(g1)
        assert dendro_bytes(dendro.measure(c, labels, 0, dopts)) == dendro_bytes(d1)
        labels2, nc2, _ = segment.segment_rgb(c, rgb, c.passthrough(2, 0.0, 14.0), segment.default_opts(min_cluster_size=100))
        assert nc2 == nc and np.array_equal(labels, labels2)


def rotated_plot():
    scale = 0.37
    xyz, member, _ = plot(20, SQUARE5, rot=12, scale=scale)
    return xyz, scale


def test_inventory_equals_the_chain_of_the_stubs(ctx, tr, gn, dn):
    xyz, scale = rotated_plot()
    o, g = framed_opts(tr, gn, xyz, scale)
    want = stub_run(tr, xyz, opts=o)
    d = dendro_opts(dn, scale=scale, up=tuple(g.up), north=tuple(g.north), ground=g.offset * scale)
    with Cloud(xyz) as c:
        got_g, tree_of, stems, res, per_tree = trees.inventory(c, ground.default_opts(inlier_tol=TOL / scale), None,
                                                               trees.default_opts(scale=scale), dendro.default_opts(scale=scale))
    assert ground_bytes(got_g) == ground_bytes(g) and same_run((tree_of, stems, res), want) and res.n_trees == 4 == len(per_tree)
    for s in range(4):
        assert dendro_bytes(per_tree[s]) == dendro_bytes(dendro_run(dn, xyz, want[0], s, d)[0]) and abs(per_tree[s].dbh - 0.3) < 0.01


def test_host_mirror_selftest_plot(ctx, tr, gn, tmp_path):
    """sfm_dendro_selftest --plot on a PCD of the rotated four-tree plot prints four trees and writes the stub's labels."""
    exe = build.build_dendro_demo()
    xyz, scale = rotated_plot()                      # (default scale 1 in the self-test: the plot's lengths are 1 / 0.37 of the defaults',
    xyz = (xyz.astype(np.float64) * scale).astype(np.float32)   # so the cloud is brought back to metres first)
    pcd, out = str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, np.full(len(xyz), 0x00406020, np.uint32))
    r = subprocess.run([exe, pcd, out, "--plot=%r" % TOL], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert "Trees=4" in lines and sum(ln.startswith("Tree ") for ln in lines) == 4, r.stdout[-2000:]
    for ln in lines:
        if ln.startswith("Tree "):
            assert " Altura DAP=1.3 DAP=" in ln and abs(float(ln.split(" DAP=")[2].split()[0]) - 0.3) < 0.01
    o, _ = framed_opts(tr, gn, xyz, 1.0)
    want = stub_run(tr, xyz, opts=o)
    raw = open(out, "rb").read()
    assert np.frombuffer(raw[:4], np.int32)[0] == 4 and raw[-4 * len(xyz):] == want[0].tobytes()
