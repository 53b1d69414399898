"""Multi-view tracks (csrc/tracks.h) on the CPU, through a g++ build of the header the device code compiles
(tests/stub/tracks_capi.cpp): the components against scipy's connected_components with the conflicts by np.unique over
(label, image); T5's numbering and order asserted literally; the edge shapes (path, cycle, duplicates, a shuffled list,
min_len, empty inputs, every T1 refusal); R2 against numpy's SVD of the same matrix; R5 against the oracle's two-view
triangulation bit for bit; R1 / R4 under pose masks, min_views and front_only.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

from oracle import orc
from sfm_danpipeline_amd.tracks import TracksOpts, TracksStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "tracks_capi.cpp")
STAT_FIELDS = [f for f, _ in TracksStats._fields_]
K_RING = np.array([[1520.0, 0, 960.0], [0, 1520.0, 540.0], [0, 0, 1]])


@pytest.fixture(scope="module")
def tk(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tracks") / "libtrackscapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.trk_default_opts.argtypes = [vp]
    lib.trk_default_opts.restype = None
    lib.trk_sizes.argtypes = [vp, vp]
    lib.trk_build.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.trk_triangulate.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, ci, ci, vp, vp, vp, vp]
    lib.trk_triangulate.restype = None
    return lib


# ---------------------------------------------------------------- wrappers and generators (shared with tests/test_gpu_tracks.py)
def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def stub_build(tk, n_feat, pairs, counts, q, t, min_len=2, fill=None):
    """(rc, stats dict, trk_ptr, trk_view, trk_feat, node_track); after a refusal the arrays still hold `fill`"""
    n_feat, pairs, counts, q, t = i32(n_feat), i32(pairs).reshape(-1), i32(counts), i32(q), i32(t)
    nodes = int(np.clip(n_feat, 0, None).sum())
    ptr, view, feat, node = (np.full(n, -7 if fill is None else fill, np.int32) for n in (nodes // 2 + 2, nodes + 1, nodes + 1, nodes + 1))
    o, st = TracksOpts(min_len, 0), TracksStats()
    rc = tk.trk_build(n_feat.size, n_feat.ctypes.data, counts.size, pairs.ctypes.data, counts.ctypes.data, q.ctypes.data, t.ctypes.data,
                      C.byref(o), C.byref(st), ptr.ctypes.data, view.ctypes.data, feat.ctypes.data, node.ctypes.data)
    if rc != 0:
        return rc, None, ptr, view, feat, node
    return rc, {f: getattr(st, f) for f in STAT_FIELDS}, ptr[:st.n_tracks + 1].copy(), view[:st.n_obs].copy(), feat[:st.n_obs].copy(), node[:nodes].copy()


def stub_triangulate(tk, ptr, view, feat, poses, has_pose, K, dist, xy_ptr, xy, max_err=6.0, min_views=2, front_only=0):
    ptr, view, feat, xy_ptr = i32(ptr), i32(view), i32(feat), i32(xy_ptr)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1)
    has = np.ascontiguousarray(has_pose, np.uint8)
    K, dist = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(dist, np.float64).reshape(5)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    nt, no = ptr.size - 1, int(ptr[-1])
    X, err, used, keep = np.zeros((nt, 3)), np.zeros(no, np.float32), np.zeros(nt, np.int32), np.zeros(nt, np.uint8)
    tk.trk_triangulate(nt, ptr.ctypes.data, view.ctypes.data, feat.ctypes.data, poses.ctypes.data, has.ctypes.data, K.ctypes.data,
                       dist.ctypes.data, xy_ptr.ctypes.data, xy.ctypes.data, max_err, min_views, front_only, X.ctypes.data, err.ctypes.data,
                       used.ctypes.data, keep.ctypes.data)
    return X, err, used, keep.astype(bool)


def world_graph(seed, n_images, n_feat, n_world, p_seen=0.6, p_match=0.7, p_false=0.02):
    """Pair lists from world ids: world point w is seen in an image with p_seen, under a feature index of that image's own
    shuffle; every pair of images lists the points both see with p_match, and a listed match is false (its second index
    replaced by a random feature) with p_false.  Returns (n_feat [n_images], pairs, counts, q, t, feat_of [n_images, n_world])."""
    rng = np.random.default_rng(seed)
    nf = np.full(n_images, n_feat, np.int32)
    feat_of = np.full((n_images, n_world), -1, np.int32)
    for i in range(n_images):
        seen = np.flatnonzero(rng.random(n_world) < p_seen)[:n_feat]
        feat_of[i, seen] = rng.permutation(n_feat)[:seen.size]
    pairs, counts, q, t = [], [], [], []
    for a in range(n_images):
        for b in range(a + 1, n_images):
            both = np.flatnonzero((feat_of[a] >= 0) & (feat_of[b] >= 0))
            both = both[rng.random(both.size) < p_match]
            tb = feat_of[b, both].copy()
            false = rng.random(both.size) < p_false
            tb[false] = rng.integers(0, n_feat, int(false.sum()))
            pairs.append((a, b)), counts.append(both.size), q.append(feat_of[a, both]), t.append(tb)
    return nf, i32(pairs), i32(counts), i32(np.concatenate(q)), i32(np.concatenate(t)), feat_of


def reference_tracks(n_feat, pairs, counts, q, t, min_len=2):
    """T1-T5 by scipy and numpy alone: (stats dict, trk_ptr, trk_view, trk_feat, node_track, labels, image of every node)"""
    n_feat, pairs = np.asarray(n_feat, np.int64), np.asarray(pairs, np.int64).reshape(-1, 2)
    base = np.concatenate([[0], np.cumsum(n_feat)])
    n = int(base[-1])
    pa = np.repeat(pairs[:, 0], counts) if len(pairs) else np.zeros(0, np.int64)
    pb = np.repeat(pairs[:, 1], counts) if len(pairs) else np.zeros(0, np.int64)
    u, v = base[pa] + q, base[pb] + t
    g = sparse.coo_matrix((np.ones(u.size, np.int8), (u, v)), shape=(n, n))
    _, lab = csgraph.connected_components(g, directed=False)
    img = np.searchsorted(base, np.arange(n), side="right") - 1
    size = np.bincount(lab, minlength=lab.max() + 1 if n else 0)
    distinct = np.bincount(np.unique(np.stack([lab, img], 1), axis=0)[:, 0], minlength=size.size) if n else size
    conflicting = distinct < size
    need = max(2, min_len)
    kept = (~conflicting) & (size >= need)
    root = np.full(size.size, n, np.int64)
    np.minimum.at(root, lab, np.arange(n))
    order = np.argsort(root[kept])                       # tracks by ascending root
    kept_labels = np.flatnonzero(kept)[order]
    tno = np.full(size.size, -1, np.int64)
    tno[kept_labels] = np.arange(kept_labels.size)
    node_track = tno[lab] if n else np.zeros(0, np.int64)
    nodes = np.flatnonzero(node_track >= 0)
    nodes = nodes[np.argsort(node_track[nodes], kind="stable")]  # inside a track ascending node id = ascending (view, feature)
    ptr = np.concatenate([[0], np.cumsum(size[kept_labels])])
    stats = dict(nodes=n, edges=int(u.size), components=int((size >= 2).sum()), conflicting=int(conflicting.sum()),
                 short_tracks=int(((~conflicting) & (size >= 2) & (size < need)).sum()), n_tracks=int(kept.sum()), n_obs=int(ptr[-1]))
    return stats, i32(ptr), i32(img[nodes]), i32(nodes - base[img[nodes]]), i32(node_track), lab, img


def ring_scene(seed, n_views, n_pts, noise=0.5, radius=10.0, dist=None, K=K_RING):
    """n_views cameras on a circle of `radius` around the origin, looking inwards; n_pts points in the unit ball, each seen
    in every view as feature = its own index; pixels = cv::projectPoints' model + uniform noise of +-noise px.
    Returns (poses [n, 3, 4], dist, xy_ptr, xy [n * n_pts, 2], world)."""
    rng = np.random.default_rng(seed)
    dist = np.zeros(5) if dist is None else np.asarray(dist, np.float64)
    world = rng.normal(size=(n_pts, 3))
    world *= (rng.random(n_pts) ** (1 / 3) / np.linalg.norm(world, axis=1))[:, None]
    poses, xy = np.zeros((n_views, 3, 4)), np.zeros((n_views, n_pts, 2))
    for i in range(n_views):
        a = 2 * np.pi * i / n_views
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        Cc = np.array([-radius * s, 0.3 * np.sin(3 * a), -radius * c])
        poses[i, :, :3], poses[i, :, 3] = R, -R @ Cc
        xy[i] = project(poses[i], K, dist, world) + noise * (2 * rng.random((n_pts, 2)) - 1)
    return poses, dist, i32(np.arange(n_views + 1) * n_pts), xy.reshape(-1, 2), world


def project(P, K, dist, X):
    x = X @ P[:, :3].T + P[:, 3]
    x, y = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3
    xd = x * cd + p1 * 2 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + p2 * 2 * x * y
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], 1)


def full_tracks(n_views, n_pts):
    """the CSR in which point j is one track through every view, as feature j"""
    return i32(np.arange(n_pts + 1) * n_views), i32(np.tile(np.arange(n_views), n_pts)), i32(np.repeat(np.arange(n_pts), n_views))


def assert_tracks_equal(got, ref):
    st, ptr, view, feat, node = got
    rst, rptr, rview, rfeat, rnode = ref[:5]
    assert st == rst
    for a, b in ((ptr, rptr), (view, rview), (feat, rfeat), (node, rnode)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- T1-T5
def test_struct_sizes(tk):
    a, b = C.c_int(), C.c_int()
    tk.trk_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(TracksOpts), C.sizeof(TracksStats))
    o = TracksOpts(9, 9)
    tk.trk_default_opts(C.byref(o))
    assert (o.min_len, o.front_only) == (2, 0)


@pytest.mark.parametrize("seed,n_images,n_feat,n_world", [(1, 8, 120, 150), (2, 14, 60, 90), (3, 5, 400, 380)])
def test_components_against_scipy(tk, seed, n_images, n_feat, n_world):
    nf, pairs, counts, q, t, _ = world_graph(seed, n_images, n_feat, n_world)
    ref = reference_tracks(nf, pairs, counts, q, t)
    lab, img = ref[5], ref[6]
    # the input itself, on scipy's answer alone: conflicts, a length-2 and a long component, most components kept
    size = np.bincount(lab)
    distinct = np.bincount(np.unique(np.stack([lab, img], 1), axis=0)[:, 0], minlength=size.size)
    real = size >= 2
    assert (distinct < size).any() and ((size == 2) & (distinct == size)).any() and ((size >= 5) & (distinct == size)).any()
    assert ((distinct == size) & real).sum() > real.sum() / 2
    rc, *got = stub_build(tk, nf, pairs, counts, q, t)
    assert rc == 0
    assert_tracks_equal(got, ref)
    assert got[0]["components"] == got[0]["conflicting"] + got[0]["short_tracks"] + got[0]["n_tracks"]


def test_numbering_and_order_literally(tk):
    # images of 3, 2, 0, 3 features: nodes 0-2 | 3-4 | - | 5-7
    nf = [3, 2, 0, 3]
    pairs, counts = [(3, 0), (0, 1), (1, 3), (3, 1)], [2, 1, 1, 1]
    q = [2, 0, 2, 1, 1]      # (3,2)-(0,1)  (3,0)-(0,2) | (0,2)-(1,0) | (1,1)-(3,2)... see t
    t = [1, 2, 0, 2, 0]
    # edges: n7-n1, n5-n2, n2-n3, n4-n7, n6-n3
    rc, st, ptr, view, feat, node = stub_build(tk, nf, pairs, counts, q, t)
    assert rc == 0
    # components: {1, 4, 7} root 1; {2, 3, 5, 6} root 2 -- two nodes of image 3: conflicting; {0} alone
    assert st == dict(nodes=8, edges=5, components=2, conflicting=1, short_tracks=0, n_tracks=1, n_obs=3)
    assert ptr.tolist() == [0, 3] and view.tolist() == [0, 1, 3] and feat.tolist() == [1, 1, 2]
    assert node.tolist() == [-1, 0, -1, -1, 0, -1, -1, 0]
    # two tracks: numbered by their least node
    rc, st, ptr, view, feat, node = stub_build(tk, [2, 2, 2], [(1, 2), (0, 1)], [1, 1], [0, 1], [1, 1])
    assert rc == 0 and ptr.tolist() == [0, 2, 4] and view.tolist() == [0, 1, 1, 2] and feat.tolist() == [1, 1, 0, 1]
    assert node.tolist() == [-1, 0, 1, 0, -1, 1]


def chain(n_images, n_feat=3, f=1):
    return [n_feat] * n_images, [(i, i + 1) for i in range(n_images - 1)], [1] * (n_images - 1), [f] * (n_images - 1), [f] * (n_images - 1)


def test_edge_shapes(tk):
    rc, st, ptr, view, feat, node = stub_build(tk, *chain(10))            # a path through 10 images
    assert rc == 0 and st["n_tracks"] == 1 and view.tolist() == list(range(10)) and feat.tolist() == [1] * 10
    nf, pairs, counts, q, t = chain(5)                                     # a cycle: the path plus its closing edge
    rc, st2, *rest = stub_build(tk, nf, pairs + [(4, 0)], counts + [1], q + [1], t + [1])
    assert rc == 0 and st2["n_tracks"] == 1 and st2["n_obs"] == 5 and st2["edges"] == 5
    base = stub_build(tk, nf, pairs, counts, q, t)
    dup = stub_build(tk, nf, pairs + pairs, counts + counts, q + q, t + t)  # duplicate pairs and edges
    assert dup[0] == 0 and dup[1]["edges"] == 8 and all(a.tobytes() == b.tobytes() for a, b in zip(dup[2:], base[2:]))
    rc, st3, ptr3, *_ = stub_build(tk, nf, pairs, counts, q, t, min_len=6)
    assert rc == 0 and (st3["n_tracks"], st3["short_tracks"], st3["components"]) == (0, 1, 1) and ptr3.tolist() == [0]


def test_shuffled_edges_give_the_same_bytes(tk):
    nf, pairs, counts, q, t, _ = world_graph(5, 7, 90, 120)
    a = stub_build(tk, nf, pairs, counts, q, t)
    rng = np.random.default_rng(0)
    # one pair per edge, in random order, half of them stated the other way round
    pa, pb = np.repeat(pairs[:, 0], counts), np.repeat(pairs[:, 1], counts)
    order, flip = rng.permutation(q.size), rng.random(q.size) < 0.5
    p2 = np.where(flip[:, None], np.stack([pb, pa], 1), np.stack([pa, pb], 1))[order]
    q2, t2 = np.where(flip, t, q)[order], np.where(flip, q, t)[order]
    b = stub_build(tk, nf, p2, np.ones(q.size, np.int32), q2, t2)
    assert a[0] == b[0] == 0 and a[1] == b[1] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))


def test_min_len_three(tk):
    nf, pairs, counts, q, t, _ = world_graph(6, 6, 80, 100)
    for min_len in (0, 2, 3, 5):
        rc, *got = stub_build(tk, nf, pairs, counts, q, t, min_len=min_len)
        assert rc == 0
        assert_tracks_equal(got, reference_tracks(nf, pairs, counts, q, t, min_len))
    assert (np.diff(got[1]) >= 5).all()


def test_empty_inputs(tk):
    e = np.zeros(0, np.int32)
    for nf, pairs, counts in (([], e, e), ([4, 0, 5], e, e), ([4, 0, 5], [(0, 2), (2, 1)], [0, 0]), ([0, 0], [(0, 1)], [0])):
        rc, st, ptr, view, feat, node = stub_build(tk, nf, pairs, counts, e, e)
        assert rc == 0 and st["n_tracks"] == 0 and st["n_obs"] == 0 and ptr.tolist() == [0] and view.size == 0
        assert node.tolist() == [-1] * int(np.sum(nf))


REFUSALS = [("q at n_feat", [3, 3], [(0, 1)], [1], [3], [0]), ("t at n_feat", [3, 3], [(0, 1)], [1], [0], [3]),
            ("negative q", [3, 3], [(0, 1)], [1], [-1], [0]), ("negative t", [3, 3], [(0, 1)], [1], [0], [-1]),
            ("self pair", [3, 3], [(1, 1)], [1], [0], [1]), ("image past the end", [3, 3], [(0, 2)], [1], [0], [0]),
            ("negative image", [3, 3], [(-1, 1)], [1], [0], [0]), ("self pair without matches", [3, 3], [(0, 0)], [0], [], []),
            ("a feature of an empty image", [3, 0], [(0, 1)], [1], [0], [0]),
            ("the last match of the last pair", [3, 3, 3], [(0, 1), (1, 2)], [2, 2], [0, 1, 0, 1], [0, 1, 0, 3])]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_t1_refusals_leave_the_outputs_untouched(tk, case):
    _, nf, pairs, counts, q, t = case
    rc, st, *arrays = stub_build(tk, nf, pairs, counts, q, t, fill=-7)
    assert rc == 1 and st is None and all((a == -7).all() for a in arrays)


# ---------------------------------------------------------------- R1-R5
def svd_points(poses, K, xy, n_views, n_pts):
    """R2's matrix in numpy (no distortion) and numpy's SVD of it"""
    X = np.zeros((n_pts, 3))
    for j in range(n_pts):
        rows = []
        for v in range(n_views):
            u, w = xy[v * n_pts + j]
            x, y = (u - K[0, 2]) * (1.0 / K[0, 0]), (w - K[1, 2]) * (1.0 / K[1, 1])
            rows += [x * poses[v, 2] - poses[v, 0], y * poses[v, 2] - poses[v, 1]]
        vt = np.linalg.svd(np.array(rows))[2][-1]
        X[j] = vt[:3] / vt[3]
    return X


@pytest.mark.parametrize("m", [2, 3, 5, 10, 32])
def test_r2_against_numpy_svd(tk, m):
    """|X - X_svd| <= 1e-11 (|X| <= 1): a numpy restatement of the rule agreed with numpy's SVD to 2.6e-14 on 300 scenes per m; the
    stub's worst over these scenes is printed (DESIGN.md f-16 records it)"""
    worst = 0.0
    for seed in range(3):
        n_pts = 40
        poses, dist, xy_ptr, xy, _ = ring_scene(100 * m + seed, m, n_pts)
        X, err, used, keep = stub_triangulate(tk, *full_tracks(m, n_pts), poses, np.ones(m, np.uint8), K_RING, dist, xy_ptr, xy)
        assert (used == m).all() and keep.all() and (err >= 0).all() and err.max() < 3.0
        worst = max(worst, np.abs(X - svd_points(poses, K_RING, xy, m, n_pts)).max())
    print(f"R2 m={m}: worst |X - X_svd| = {worst:.3e}")
    assert worst <= 1e-11


def two_view_case(seed, n, dist, nan_at=None):
    poses, dist, xy_ptr, xy, _ = ring_scene(seed, 7, n, dist=dist)
    if nan_at is not None:
        xy[2 * n + nan_at, 0] = np.nan
    return poses, dist, xy_ptr, xy


@pytest.mark.parametrize("dist,nan_at", [(None, None), ((-0.12, 0.03, 1e-3, -2e-3, 1e-3), None), ((-0.12, 0.03, 1e-3, -2e-3, 1e-3), 5)],
                         ids=["plain", "distorted", "distorted+nan"])
def test_r5_two_view_tracks_equal_the_oracle_bit_for_bit(tk, dist, nan_at):
    n, va, vb = 70, 2, 5
    poses, dist, xy_ptr, xy = two_view_case(11, n, dist, nan_at)
    ptr, view, feat = i32(np.arange(n + 1) * 2), i32(np.tile([va, vb], n)), i32(np.repeat(np.arange(n), 2))
    X, err, used, keep = stub_triangulate(tk, ptr, view, feat, poses, np.ones(7, np.uint8), K_RING, dist, xy_ptr, xy, max_err=0.15)
    Xo, erro, keepo = orc.triangulate(poses[va], poses[vb], K_RING, dist, xy[va * n:(va + 1) * n], xy[vb * n:(vb + 1) * n], max_err=0.15)
    assert X.view(np.uint64).tolist() == Xo.view(np.uint64).tolist()
    assert err.view(np.uint32).tolist() == erro.reshape(-1).view(np.uint32).tolist()
    assert keep.tolist() == keepo.astype(bool).tolist() and 0 < keep.sum() < n
    if nan_at is not None:
        assert np.isnan(X[nan_at]).all() and keep[nan_at]     # a NaN error keeps its point, as sfmhip_triangulate does
    # the same two views out of a five-view track, the other three without a pose
    ptr5, view5, feat5 = i32(np.arange(n + 1) * 5), i32(np.tile([0, va, 3, vb, 6], n)), i32(np.repeat(np.arange(n), 5))
    has = np.zeros(7, np.uint8)
    has[[va, vb]] = 1
    X5, err5, used5, keep5 = stub_triangulate(tk, ptr5, view5, feat5, poses, has, K_RING, dist, xy_ptr, xy, max_err=0.15)
    assert X5.view(np.uint64).tolist() == Xo.view(np.uint64).tolist() and keep5.tolist() == keep.tolist() and (used5 == 2).all()
    e5 = err5.reshape(n, 5)
    assert (e5[:, [0, 2, 4]] == -1.0).all() and e5[:, [1, 3]].view(np.uint32).tolist() == erro.view(np.uint32).tolist()


def test_r1_r4_masks_min_views_and_front_only(tk):
    n, m = 20, 4
    poses, dist, xy_ptr, xy, _ = ring_scene(21, m, n, noise=0.2)
    tr = full_tracks(m, n)
    for has, n_used in (([0, 0, 0, 0], 0), ([0, 0, 1, 0], 1), ([1, 0, 0, 1], 2), ([1, 1, 1, 1], 4)):
        X, err, used, keep = stub_triangulate(tk, *tr, poses, np.array(has, np.uint8), K_RING, dist, xy_ptr, xy)
        assert (used == n_used).all()
        e = err.reshape(n, m)
        assert (e[:, np.array(has) == 0] == -1.0).all()
        if n_used < 2:
            assert np.isnan(X).all() and not keep.any() and (err == -1.0).all()
        else:
            assert np.isfinite(X).all() and keep.all() and (e[:, np.array(has) == 1] >= 0).all()
    # min_views: two used views are too few for 3; min_views below 2 asks for 2
    for min_views, has, expect in ((3, [1, 0, 0, 1], False), (3, [1, 1, 0, 1], True), (0, [1, 0, 0, 1], True), (-5, [0, 1, 0, 0], False)):
        keep = stub_triangulate(tk, *tr, poses, np.array(has, np.uint8), K_RING, dist, xy_ptr, xy, min_views=min_views)[3]
        assert keep.all() == expect and keep.any() == expect
    # max_err: an observation moved by 50 px drops its track only
    xy2 = xy.copy()
    xy2[3] += 50.0
    keep = stub_triangulate(tk, *tr, poses, np.ones(m, np.uint8), K_RING, dist, xy_ptr, xy2)[3]
    assert not keep[3] and keep.sum() == n - 1
    # front_only: a point behind the second camera (it looks away from it), exact pixels
    P = np.zeros((2, 3, 4))
    P[0, :, :3], P[1, :, :3], P[1, :, 3] = np.eye(3), np.diag([-1.0, 1.0, -1.0]), [0.5, 0, 0]
    world = np.array([[0.1, 0.2, 5.0], [-0.3, 0.1, 4.0]])
    pix = np.concatenate([project(P[0], K_RING, np.zeros(5), world), project(P[1], K_RING, np.zeros(5), world)])
    args = (*full_tracks(2, 2), P, np.ones(2, np.uint8), K_RING, np.zeros(5), [0, 2, 4], pix)
    X, err, used, keep = stub_triangulate(tk, *args)
    assert np.abs(X - world).max() < 1e-9 and keep.all() and err.max() < 1e-6
    assert not stub_triangulate(tk, *args, front_only=1)[3].any()
    P[1, :, :3], P[1, :, 3] = np.eye(3), [0.5, 0, 0]
    pix = np.concatenate([project(P[0], K_RING, np.zeros(5), world), project(P[1], K_RING, np.zeros(5), world)])
    assert stub_triangulate(tk, *full_tracks(2, 2), P, np.ones(2, np.uint8), K_RING, np.zeros(5), [0, 2, 4], pix, front_only=1)[3].all()
