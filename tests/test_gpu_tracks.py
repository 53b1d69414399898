"""GPU: multi-view tracks and their N-view triangulation (csrc/tracks.hip) against the g++ build of the same
header (tests/stub/tracks_capi.cpp), byte for byte: the statistics, trk_ptr, trk_view, trk_feat, node_track, X as u64 bits, err
as u32 bits, n_used and keep.  The shapes are the smallest at which the kernels can go wrong: 63 / 64 / 65 tracks, one track
through all 40 images beside length-2 ones (the length buckets), a 12-image chain (path compression), a star that conflicts
(many edges on one root), the refusals, one cfg2-sized graph, the lists of a real match plan read on the device, and two-view
tracks against sfmhip_triangulate bit for bit."""
import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, matcher, synth, tracks, triangulate
from tests.test_tracks_cpu import (K_RING, REFUSALS, STAT_FIELDS, chain, i32, reference_tracks, ring_scene, stub_build,  # noqa: F401
                                   stub_triangulate, tk, world_graph)

pytestmark = pytest.mark.gpu

DIST = (-0.12, 0.03, 1e-3, -2e-3, 1e-3)


def dev_build(ctx, n_feat, pairs, counts, q, t, **opts):
    h = tracks.build(ctx, n_feat, pairs, counts, q, t, **opts)
    return h, ({f: getattr(h.stats, f) for f in STAT_FIELDS}, *h.download())


def assert_build_equal(ctx, tk, n_feat, pairs, counts, q, t, min_len=2):
    """One device build against the stub: the same statistics and bytes.  Returns the device handle and the stub's output."""
    rc, *want = stub_build(tk, n_feat, pairs, counts, q, t, min_len=min_len)
    assert rc == 0
    h, got = dev_build(ctx, n_feat, pairs, counts, q, t, min_len=min_len)
    assert got[0] == want[0], (got[0], want[0])
    for name, a, b in zip(("trk_ptr", "trk_view", "trk_feat", "node_track"), got[1:], want[1:]):
        assert a.tobytes() == b.tobytes(), name
    return h, want


def same_bits(a, b):
    """Bit for bit, except that a NaN must meet a NaN in the same entry: the host's and the device's NaNs differ in sign (as in
    tests/test_gpu_triangulate.py); every entry that is not a NaN is compared bit for bit."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    na = np.isnan(a)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, np.isnan(b))
    assert np.array_equal(a.view(u)[~na], b.view(u)[~na])


def assert_triangulation_equal(tk, h, want, poses, has, K, dist, xy_ptr, xy, **kw):
    _, ptr, view, feat, _ = want
    X, err, used, keep = h.triangulate(poses, has, K, dist, xy_ptr, xy, **kw)
    Xs, errs, useds, keeps = stub_triangulate(tk, ptr, view, feat, poses, has, K, dist, xy_ptr, xy, **kw)
    same_bits(X, Xs), same_bits(err, errs)
    assert used.tolist() == useds.tolist() and keep.tolist() == keeps.tolist()
    return X, err, used, keep


def scene_for(n_feat, seed, dist=None, noise=0.5):
    """a ring scene in which feature f of every image is world point f (the widest image sets the number of points)"""
    n_images, n_pts = len(n_feat), int(max(n_feat))
    poses, dist, xy_ptr, xy, world = ring_scene(seed, n_images, n_pts, noise=noise, dist=dist)
    return poses, dist, xy_ptr, xy, world


def same_index_graph(seed, n_images, n_pts, p_seen=0.5, p_false=0.0):
    """world point j is feature j wherever it is seen: the tracks of this graph triangulate to the ring scene's points"""
    rng = np.random.default_rng(seed)
    seen = rng.random((n_images, n_pts)) < p_seen
    pairs, counts, q, t = [], [], [], []
    for a in range(n_images):
        for b in range(a + 1, n_images):
            both = np.flatnonzero(seen[a] & seen[b] & (rng.random(n_pts) < 0.8))
            tb = both.copy()
            false = rng.random(both.size) < p_false
            tb[false] = rng.integers(0, n_pts, int(false.sum()))
            pairs.append((a, b)), counts.append(both.size), q.append(both), t.append(tb)
    return np.full(n_images, n_pts, np.int32), i32(pairs), i32(counts), i32(np.concatenate(q)), i32(np.concatenate(t))


@pytest.mark.parametrize("seed,n_images,n_feat,n_world", [(1, 8, 120, 150), (3, 5, 400, 380)])
def test_build_equals_stub_and_scipy(ctx, tk, seed, n_images, n_feat, n_world):
    nf, pairs, counts, q, t, _ = world_graph(seed, n_images, n_feat, n_world)
    for min_len in (2, 3):
        h, want = assert_build_equal(ctx, tk, nf, pairs, counts, q, t, min_len=min_len)
        ref = reference_tracks(nf, pairs, counts, q, t, min_len)
        assert want[0] == ref[0] and want[1].tobytes() == ref[1].tobytes() and want[4].tobytes() == ref[4].tobytes()
        assert want[0]["conflicting"] > 0
        h.close()


@pytest.mark.parametrize("n_tracks", [1, 63, 64, 65])
def test_track_counts_at_wave_edges(ctx, tk, n_tracks):
    """n_tracks three-view tracks (one wave less a lane, a full wave, a wave and a lane) among features that stay alone"""
    nf = [n_tracks + 3] * 3
    f = np.arange(n_tracks)
    h, want = assert_build_equal(ctx, tk, nf, [(0, 1), (1, 2)], [n_tracks, n_tracks], np.concatenate([f, f + 1]), np.concatenate([f + 1, f + 2]))
    assert want[0]["n_tracks"] == n_tracks and want[0]["n_obs"] == 3 * n_tracks
    poses, dist, xy_ptr, xy, _ = scene_for(nf, 5, DIST)
    X, err, used, keep = assert_triangulation_equal(tk, h, want, poses, np.ones(3, np.uint8), K_RING, dist, xy_ptr, xy, max_err=1e9)
    assert (used == 3).all() and keep.all()          # (features f, f + 1, f + 2 are three world points: a large error, a finite point)
    h.close()


def test_bucket_mix_one_track_through_40_images(ctx, tk):
    """a track through all 40 images beside 200 length-2 tracks and 70 length-5 ones: the slab rows of the last wave are 80 long,
    those of the first 4"""
    n_images, n_pts = 40, 271
    pairs, counts, q, t = [], [], [], []
    for i in range(n_images - 1):                                   # point 0: a chain through every image
        pairs.append((i, i + 1)), counts.append(1), q.append([0]), t.append([0])
    two = np.arange(1, 201)
    for k, j in enumerate(two):                                     # points 1..200: one pair each, spread over the ring
        a = k % (n_images - 3)
        pairs.append((a, a + 3)), counts.append(1), q.append([j]), t.append([j])
    five = np.arange(201, 271)
    for i in range(10, 14):                                         # points 201..270: images 10..14
        pairs.append((i + 1, i)), counts.append(five.size), q.append(five), t.append(five)
    nf = [n_pts] * n_images
    h, want = assert_build_equal(ctx, tk, nf, pairs, counts, np.concatenate(q), np.concatenate(t))
    lens = np.diff(want[1])
    assert sorted(set(lens.tolist())) == [2, 5, 40] and lens[0] == 40 and want[0]["n_tracks"] == 271
    poses, dist, xy_ptr, xy, world = scene_for(nf, 9, DIST)
    X, err, used, keep = assert_triangulation_equal(tk, h, want, poses, np.ones(n_images, np.uint8), K_RING, dist, xy_ptr, xy)
    first = want[3][want[1][:-1]]                                   # (feature f of every image is world point f)
    assert keep.all() and np.abs(X - world[first]).max() < 0.05 and used[0] == 40
    has = np.zeros(n_images, np.uint8)
    has[[0, 3, 10, 11, 14, 39]] = 1                                  # masks that leave 0, 1, 2 and more used views
    X, err, used, keep = assert_triangulation_equal(tk, h, want, poses, has, K_RING, dist, xy_ptr, xy, min_views=3)
    assert set(used.tolist()) >= {0, 1, 2, 3, 6} and (keep == (used >= 3)).all() and np.isnan(X[used < 2]).all()
    a = h.triangulate(poses, has, K_RING, dist, xy_ptr, xy, min_views=3)  # repeat: the same bytes, NaNs included; slab reused
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, (X, err, used, keep)))
    h.close()


def test_chain_of_12_images_and_a_conflicting_star(ctx, tk):
    nf, pairs, counts, q, t = chain(12, n_feat=4, f=2)
    h, want = assert_build_equal(ctx, tk, nf, pairs[::-1], counts, q, t)      # hooked from the far end: the deepest parent chain
    assert want[0]["n_tracks"] == 1 and want[2].tolist() == list(range(12))
    h.close()
    # a star: feature 0 of image 0 matched to 300 features of image 1 (each also linked on to image 2) -- one root, many edges
    k = 300
    nf = [4, k, k]
    f = np.arange(k)
    h, want = assert_build_equal(ctx, tk, nf, [(0, 1), (1, 2), (2, 0)], [k, k, 1], np.concatenate([np.zeros(k, int), f, [5]]),
                                 np.concatenate([f, f, [3]]))
    assert want[0] == dict(nodes=4 + 2 * k, edges=2 * k + 1, components=1, conflicting=1, short_tracks=0, n_tracks=0, n_obs=0)
    assert (want[4] == -1).all()
    h.close()


def test_degenerate_inputs_and_refusals(ctx, tk):
    e = np.zeros(0, np.int32)
    for nf, pairs, counts in (([], e, e), ([4, 0, 5], e, e), ([4, 0, 5], [(0, 2), (2, 1)], [0, 0]), ([0, 0], [(0, 1)], [0])):
        h, want = assert_build_equal(ctx, tk, nf, pairs, counts, e, e)
        assert want[0]["n_tracks"] == 0
        n = len(nf)
        out = h.triangulate(np.zeros((n, 3, 4)), np.ones(n, np.uint8), K_RING, np.zeros(5), np.cumsum([0] + list(nf)), np.zeros((sum(nf), 2)))
        assert out[0].shape == (0, 3) and out[3].size == 0
        h.close()
    for _, nf, pairs, counts, q, t in REFUSALS:
        with pytest.raises(_lib.SfmHipError, match="status -3"):
            tracks.build(ctx, nf, pairs, counts, q, t)
    nf, pairs, counts, q, t = chain(3)
    h = tracks.build(ctx, nf, pairs, counts, q, t)
    with pytest.raises(_lib.SfmHipError, match="status -3"):                 # a posed view with fewer pixels than features
        h.triangulate(np.zeros((3, 3, 4)), [1, 1, 1], K_RING, np.zeros(5), [0, 3, 5, 8], np.zeros((8, 2)))
    h.close()


@pytest.fixture(scope="module")
def cfg2_graph():
    return world_graph(7, 50, 2000, 2000, p_seen=0.7, p_match=0.83, p_false=1e-4)[:5]


def test_cfg2_sized_graph(ctx, tk, cfg2_graph):
    """50 x 2000 features, all 1225 pairs, about 10^6 edges; twice, for the same bytes"""
    nf, pairs, counts, q, t = cfg2_graph
    assert 0.9e6 < q.size < 1.1e6
    h, want = assert_build_equal(ctx, tk, nf, pairs, counts, q, t)
    assert want[0]["n_tracks"] > 1000 and want[0]["conflicting"] > 10
    h2, got2 = dev_build(ctx, nf, pairs, counts, q, t)
    assert got2[0] == want[0] and all(a.tobytes() == b.tobytes() for a, b in zip(got2[1:], want[1:]))
    h.close(), h2.close()


def test_build_from_plan_equals_build_on_the_fetched_lists(ctx, tk):
    imgs = synth.sift_image_set(6, 300, 128, bank=450, seed=3)
    pairs = synth.all_pairs(6)
    s = matcher.ImageSet(imgs, ctx=ctx)
    s.prepare_async()
    pl = matcher.MatchPlan(s, pairs)
    pl.run_async(0.8)
    counts, q, t, _ = pl.fetch()
    assert counts.sum() > 500
    nf = [len(im) for im in imgs]
    for min_len in (2, 3):
        a = tracks.build_from_plan(pl, min_len=min_len)
        h, want = assert_build_equal(ctx, tk, nf, pairs, counts, q, t, min_len=min_len)
        assert {f: getattr(a.stats, f) for f in STAT_FIELDS} == want[0] and want[0]["n_tracks"] > 50
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.download(), want[1:]))
        a.close(), h.close()
    pl.close(), s.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 5000])
def test_r5_two_view_tracks_equal_sfmhip_triangulate(ctx, tk, m):
    va, vb = 1, 4
    poses, dist, xy_ptr, xy, _ = ring_scene(40 + m, 6, m, dist=DIST)
    if m > 10:
        xy[va * m + 7, 1] = np.nan
    f = np.arange(m)
    h, want = assert_build_equal(ctx, tk, [m] * 6, [(va, vb)], [m], f, f)
    assert want[0]["n_tracks"] == m
    X, err, used, keep = assert_triangulation_equal(tk, h, want, poses, np.ones(6, np.uint8), K_RING, dist, xy_ptr, xy, max_err=0.15)
    Xt, errt, keept = triangulate.triangulate_points(poses[va], poses[vb], K_RING, dist, xy[va * m:(va + 1) * m], xy[vb * m:(vb + 1) * m],
                                                     max_err=0.15, ctx=ctx)
    same_bits(X, Xt), same_bits(err, errt)
    assert keep.tolist() == keept.astype(bool).tolist() and (used == 2).all()
    if m > 10:
        assert np.isnan(X[7]).all() and keep[7] and np.isnan(err).sum() == 2 and np.isnan(X).sum() == 3
    h.close()


def test_noisy_graph_triangulates_and_front_only(ctx, tk):
    """tracks of a graph with false matches, on the ring scene: a kept track whose features are one world point gives that point"""
    nf, pairs, counts, q, t = same_index_graph(12, 9, 130, p_false=0.01)
    h, want = assert_build_equal(ctx, tk, nf, pairs, counts, q, t)
    assert want[0]["conflicting"] > 0 and want[0]["n_tracks"] > 60
    poses, dist, xy_ptr, xy, world = scene_for(nf, 13, DIST)
    X, err, used, keep = assert_triangulation_equal(tk, h, want, poses, np.ones(9, np.uint8), K_RING, dist, xy_ptr, xy)
    first = want[3][want[1][:-1]]
    pure = np.array([(want[3][a:b] == want[3][a]).all() for a, b in zip(want[1][:-1], want[1][1:])])
    assert pure.sum() > 60 and keep[pure].all() and np.abs(X - world[first])[pure].max() < 0.05
    h.close()
    hf = tracks.build(ctx, nf, pairs, counts, q, t, front_only=1)
    poses2 = poses.copy()
    poses2[2, :, :3], poses2[2, :, 3] = np.diag([-1.0, 1.0, -1.0]) @ poses[2, :, :3], np.diag([-1.0, 1.0, -1.0]) @ poses[2, :, 3]
    Xf, errf, usedf, keepf = hf.triangulate(poses2, np.ones(9, np.uint8), K_RING, dist, xy_ptr, xy, max_err=1e9)
    Xs, errs, useds, keeps = stub_triangulate(tk, *want[1:4], poses2, np.ones(9, np.uint8), K_RING, dist, xy_ptr, xy, max_err=1e9, front_only=1)
    same_bits(Xf, Xs)
    assert keepf.tolist() == keeps.tolist() and 0 < keepf.sum() < keepf.size
    hf.close()
