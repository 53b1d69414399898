"""GPU: what the cloud family shares on the handle (csrc/cloud_grid.h): the stages' state slots and their lifetime, the grow-only
device arrays across calls of changing size (under SFMHIP_POISON, so a regrown block starts as NaN / -1), the one min / max
record under two handles that alternate, and sfmhip_cloud_minmax on a cloud with no finite point.  Every result is compared
with the same call on a fresh handle, byte for byte; the stage tests hold the stages to their stubs."""
import numpy as np
import pytest

from sfm_danpipeline_amd import dendro, ground, poisson, segment, trees
from sfm_danpipeline_amd.cloud import Cloud
from tests.test_cloud_filter_cpu import surface_cloud
from tests.test_dendro_cpu import result_bytes as dendro_bytes
from tests.test_ground_cpu import result_bytes as ground_bytes, scene as ground_scene
from tests.test_poisson_cpu import cg_cap, sphere_cloud
from tests.test_segment_cpu import passthrough_z, patch_scene
from tests.test_trees_cpu import SQUARE5, plot, same_run

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- one call of a stage, as bytes
def run_ground(c, cams=None):
    return ground_bytes(ground.ground_plane(c, opts=ground.default_opts(min_inliers=50), cam_centres=cams))


def run_trees(c, **kw):
    return trees.trees(c, opts=trees.default_opts(ground=0.0, min_stem_pts=10, **kw))


def run_dendro(c, labels=None, label=0):
    res, rows = dendro.measure_profile(c, labels, label)
    return dendro_bytes(res) + rows.tobytes(), res


def run_voxel_grid(c, leaf, rgb, nrm):
    out = c.voxel_grid(leaf, rgb=rgb, normals=nrm)
    return b"".join(out[k].tobytes() for k in ("xyz", "voxel_of", "rgb", "normals")), len(out["xyz"])


def run_sor(c):
    kept, md, thr = c.statistical_outlier(8, 1.0, return_distances=True)
    return kept.tobytes() + md.tobytes() + np.float64(thr).tobytes()


def run_poisson(c, nrm, depth):
    v, t, s = poisson.reconstruct(c, nrm, poisson.default_opts(depth=depth, cg_max_iter=cg_cap(depth)))
    return v.tobytes() + t.tobytes() + np.float64([s.iso_value, s.cg_relative_residual]).tobytes(), (s.n_samples, s.cg_iterations, s.grid)


def alone(xyz, f, *a, **kw):
    """f on a fresh handle over xyz."""
    with Cloud(xyz) as c:
        return f(c, *a, **kw)


# ---------------------------------------------------------------- scenes (3 000 to 8 000 points)
@pytest.fixture(scope="module")
def tree_plot():
    return plot(20, SQUARE5, n_tree=1000, n_ground=2000)[0]                      # 6 000 points, four trees on a ground disc


@pytest.fixture(scope="module")
def tree_on_ground():
    xyz, labels = ground_scene(31, 6000, 2000)[:2]                               # 8 000 points: labels 0 ground, 1 the tree
    return xyz, labels


def works(xyz):
    """A further handle over xyz does what a handle does."""
    with Cloud(xyz) as c:
        mn, mx, _ = segment.minmax(c)
        fin = np.isfinite(xyz).all(1)
        assert np.array_equal(mn, xyz[fin].min(0)) and np.array_equal(mx, xyz[fin].max(0))
        assert np.array_equal(c.passthrough("z", 0.0, 14.0), passthrough_z(xyz))


# ---------------------------------------------------------------- lifetime
def test_handles_without_a_stage_call_and_of_no_points(ctx, tree_plot):
    Cloud(tree_plot).close()
    works(tree_plot)
    with Cloud(tree_plot) as c:                                                  # a timing query before any stage call: zeros
        assert not any(segment.last_timing(c).values()) and not any(poisson.last_timing(c).values())
        assert not any(dendro.last_timing(c).values()) and not any(ground.last_timing(c).values())
        assert not any(trees.last_timing(c).values()) and not any(c.filter_last_timing())
    empty = np.zeros((0, 3), np.float32)
    Cloud(empty).close()
    with Cloud(empty) as c:                                                      # the stages on no points: nothing to do, no fault
        assert len(c.passthrough("z", 0.0, 14.0)) == 0
        assert ground.ground_plane(c).n_selected == 0 and dendro.measure(c).n_selected == 0
        assert trees.trees(c, opts=trees.default_opts(ground=0.0))[2].n_selected == 0
        assert len(c.voxel_grid(0.05)["xyz"]) == 0 and len(c.statistical_outlier(8)) == 0
        assert not any(ground.last_timing(c).values())
    works(tree_plot)


def test_all_seven_stages_once_then_destroy(ctx):
    xyz, rgb, _, _ = patch_scene(3000, 3, close=True)
    xyz[5::977, 0] = np.nan
    ind = passthrough_z(xyz)
    with Cloud(xyz) as c:
        nrm = c.normals(10)                                                      # cloud.hip: the k-NN grid
        assert len(c.radius_outlier(0.1, 2)) > 0                                 # ... and the radius grid with its chunk tables
        assert len(c.voxel_grid(0.05, rgb=rgb, normals=nrm[:, :3])["xyz"]) > 0   # cloud_filter.hip
        assert len(c.statistical_outlier(8)) > 0
        assert segment.segment_rgb(c, rgb, ind, segment.default_opts(min_cluster_size=100))[1] >= 1      # segment.hip
        flipped = nrm.copy()
        flipped[:, :3] *= -1.0
        assert poisson.reconstruct(c, flipped, poisson.default_opts(depth=5, cg_max_iter=cg_cap(5)))[2].n_samples > 0   # poisson.hip
        assert dendro.measure(c, opts=dendro.default_opts(up=(1, 0, 0), slice=0.02, scale=0.2, min_slice_pts=5)).n_selected > 0
        assert ground.ground_plane(c, opts=ground.default_opts(min_inliers=50)).n_selected > 0
        assert run_trees(c, ground_clear=0.0, band_lo=0.0, band_hi=0.5, min_cell_pts=1, stem_cell=0.1, voxel=0.2,
                         max_stem_width=10.0)[2].n_selected > 0
    works(xyz)


# ---------------------------------------------------------------- growth across calls on one handle
def test_ground_with_a_growing_list_of_camera_centres(ctx, monkeypatch, tree_on_ground):
    monkeypatch.setenv("SFMHIP_POISON", "1")
    xyz = tree_on_ground[0]
    cams = np.array([[0.0, 0.0, 5.0], [1.0, 1.0, 6.0], [-2.0, 1.0, -4.0], [3.0, -1.0, -5.0], [0.5, 0.5, -6.0]])
    with Cloud(xyz) as c:
        for k in (0, 2, 5, 1):                                                   # 5 centres: three of them below the ground
            use = cams[:k] if k else None
            assert run_ground(c, use) == alone(xyz, run_ground, use), k


def test_trees_with_growing_cell_and_voxel_tables(ctx, monkeypatch, tree_plot):
    monkeypatch.setenv("SFMHIP_POISON", "1")
    coarse, fine = dict(stem_cell=0.2, voxel=0.6), dict(stem_cell=0.05, voxel=0.15)   # 16 times the stem cells, more voxels
    with Cloud(tree_plot) as c:
        seen = []
        for kw in (coarse, fine, coarse):
            got, want = run_trees(c, **kw), alone(tree_plot, run_trees, **kw)
            assert same_run(got, want) and got[2].n_trees >= 1, kw                # (with a stem the neighbour table is built)
            seen.append(got[2].n_voxels)
        assert seen[1] > seen[0] == seen[2]


def test_voxel_grid_with_growing_run_tables_then_outlier_removal(ctx, monkeypatch):
    monkeypatch.setenv("SFMHIP_POISON", "1")
    xyz = surface_cloud(8000, 21)
    xyz[::401, 1] = np.nan
    rng = np.random.default_rng(6)
    rgb, nrm = rng.integers(0, 1 << 32, len(xyz), dtype=np.uint32), rng.normal(size=(len(xyz), 3)).astype(np.float32)
    with Cloud(xyz) as c:
        rows = []
        for leaf in (0.05, 0.02, 0.05):
            got, want = run_voxel_grid(c, leaf, rgb, nrm), alone(xyz, run_voxel_grid, leaf, rgb, nrm)
            assert got == want, leaf
            rows.append(got[1])
        assert rows[1] > rows[0] == rows[2]
        assert run_sor(c) == alone(xyz, run_sor)


def test_poisson_with_a_growing_block_pool(ctx, monkeypatch):
    monkeypatch.setenv("SFMHIP_POISON", "1")
    xyz, nrm = sphere_cloud(3000, 11)
    with Cloud(xyz) as c:
        for depth in (5, 6, 5):
            got, want = run_poisson(c, nrm, depth), alone(xyz, run_poisson, nrm, depth)
            assert got == want and got[1][0] == 3000 and got[1][2] == 1 << depth, depth


# ---------------------------------------------------------------- the shared min / max record
def test_two_handles_alternating(ctx, tree_on_ground, tree_plot):
    """ground on A, trees on B, dendrometry on A (two min / max calls inside it), ground on B: each equals the call alone."""
    xyz_a, labels = tree_on_ground
    with Cloud(xyz_a) as a, Cloud(tree_plot) as b:
        g_a = run_ground(a)
        t_b = run_trees(b)
        d_a, res = run_dendro(a, labels, 1)
        g_b = run_ground(b)
    assert res.crown_base_slice >= 0 and not res.flags & dendro.NO_CROWN          # the second min / max call, over the crown, ran
    assert g_a == alone(xyz_a, run_ground) and g_b == alone(tree_plot, run_ground)
    assert same_run(t_b, alone(tree_plot, run_trees)) and t_b[2].n_trees >= 1
    assert d_a == alone(xyz_a, run_dendro, labels, 1)[0]


# ---------------------------------------------------------------- sfmhip_cloud_minmax with no finite point
def test_minmax_with_no_finite_point(ctx):
    """pcl::getMinMax3D starts at FLT_MAX / -FLT_MAX and a cloud with no finite point keeps them; the height is segment.h's:
    each difference -FLT_MAX - FLT_MAX overflows to -inf in float, so the root of the sum of squares is +inf."""
    for xyz in (np.full((5, 3), np.nan, np.float32), np.zeros((0, 3), np.float32)):
        with Cloud(xyz) as c:
            mn, mx, h = segment.minmax(c)
        assert np.array_equal(bits(mn), bits(np.full(3, FLT_MAX))) and np.array_equal(bits(mx), bits(np.full(3, -FLT_MAX)))
        assert h == np.inf
    one = np.full((7, 3), np.nan, np.float32)
    one[4] = (0.25, -3.5, 1e-30)
    one[2, 1] = 9.0                                                              # (a point with one finite coordinate is not finite)
    with Cloud(one) as c:
        mn, mx, h = segment.minmax(c)
    assert np.array_equal(bits(mn), bits(one[4])) and np.array_equal(bits(mx), bits(one[4])) and h == 0.0
