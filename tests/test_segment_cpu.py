"""The colour region growing after map3D (csrc/segment.h: pcl::RegionGrowingRGB behind a PassThrough on z, reference
src/Segmentation.cpp:3-66) and Dendrometry's bounds (src/DendrometryE.cpp:3-29) on the CPU, through a g++ build of the
header the device code compiles (tests/stub/segment_capi.cpp): an independent, literal Python transcription of rules
2-10 of DESIGN.md f-8 (queue growth, plain loops, scipy's neighbours re-ranked in float32) against the stub on seeded
clouds, a planted scene of colour patches, the rule cases built by hand, the bounds against numpy, the XYZRGB PCD
reader, and one cloud under ASan / UBSan.  No GPU.  PARITY UNPINNED: PCL is not in the image."""
import ctypes as C
import heapq
import os
import struct
import subprocess
from collections import deque

import numpy as np
import pytest
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "segment_capi.cpp")
FLT_MAX = float(np.finfo(np.float32).max)
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("segment") / "libsegmentcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci, u32 = C.c_void_p, C.c_int, C.c_uint32
    lib.seg_reference_opts.argtypes = [vp, vp]
    lib.seg_reference_opts.restype = None
    lib.seg_colour_diff.argtypes = [u32, u32]
    lib.seg_channel.argtypes = [C.c_uint, C.c_uint]
    lib.seg_channel.restype = C.c_uint
    lib.seg_subset_knn.argtypes = [ci, vp, vp, ci, ci, vp, vp]
    lib.seg_grow.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp]
    lib.seg_segment_rgb.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.seg_regions.argtypes = [vp, vp, ci] + [vp] * 6 + [ci] + [vp] * 4
    lib.seg_regions.restype = None
    lib.seg_minmax.argtypes = [ci, vp, vp, vp, vp]
    lib.seg_minmax.restype = None
    lib.seg_load_pcd.argtypes = [C.c_char_p, vp, vp, ci, vp]
    lib.seg_ord_keys.argtypes = [ci, vp, vp, vp]
    lib.seg_ord_keys.restype = None
    return lib


# ---------------------------------------------------------------- numpy-facing wrappers (shared with tests/test_gpu_segment.py)
def ref_opts(**kw):
    """The reference's options as a dict (rule 1); keyword arguments override."""
    o = dict(region_neighbour_number=100, neighbour_number=30, min_cluster_size=600, max_cluster_size=INT_MAX,
             distance_threshold=10.0, point_color_threshold=6.0, region_color_threshold=5.0)
    o.update(kw)
    return o


def _opts(o):
    oi = np.array([o["region_neighbour_number"], o["neighbour_number"], o["min_cluster_size"], o["max_cluster_size"]], np.int32)
    of = np.array([o["distance_threshold"], o["point_color_threshold"], o["region_color_threshold"]], np.float32)
    return oi, of


def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def _i(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


def _u(a):
    return np.ascontiguousarray(np.asarray(a, np.uint32).reshape(-1))


def stub_subset_knn(sc, xyz, ind, k):
    xyz, ind = _f(xyz), _i(ind)
    idx, d2 = np.zeros((max(len(ind), 1), k), np.int32), np.zeros((max(len(ind), 1), k), np.float32)
    rc = sc.seg_subset_knn(len(xyz), xyz.ctypes.data, ind.ctypes.data, len(ind), k, idx.ctypes.data, d2.ctypes.data)
    assert rc == 0, rc
    return idx[:len(ind)], d2[:len(ind)]


def stub_grow(sc, xyz, rgb, ind, o):
    xyz, rgb, ind = _f(xyz), _u(rgb), _i(ind)
    oi, of = _opts(o)
    seg = np.zeros(max(len(xyz), 1), np.int32)
    ns = sc.seg_grow(len(xyz), xyz.ctypes.data, rgb.ctypes.data, ind.ctypes.data, len(ind), oi.ctypes.data, of.ctypes.data, seg.ctypes.data)
    assert ns >= 0, ns
    return seg[:len(xyz)], ns


def stub_segment(sc, xyz, rgb, ind, o):
    """(labels [n], cluster count, stats [n_idx, segments, regions, 0], region of every indexed point)."""
    xyz, rgb, ind = _f(xyz), _u(rgb), _i(ind)
    oi, of = _opts(o)
    labels, nc, stats = np.zeros(max(len(xyz), 1), np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)
    reg = np.zeros(max(len(ind), 1), np.int32)
    rc = sc.seg_segment_rgb(len(xyz), xyz.ctypes.data, rgb.ctypes.data, ind.ctypes.data, len(ind), oi.ctypes.data, of.ctypes.data,
                            labels.ctypes.data, nc.ctypes.data, stats.ctypes.data, reg.ctypes.data)
    if rc != 0:
        return rc
    return labels[:len(xyz)], int(nc[0]), stats, reg[:len(ind)]


def stub_regions(sc, o, count, colour, lists, point_seg):
    """Rules 8-10 on tables built by hand: lists[s] = [(segment, d2), ...] in stored order."""
    oi, of = _opts(o)
    S = len(count)
    off = np.zeros(S + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ns = _i([q for l in lists for q, _ in l] + [0])
    nd = np.array([d for l in lists for _, d in l] + [0], np.float32)
    count, colour, point_seg = _i(count), _u(np.asarray(colour).reshape(-1)), _i(point_seg)
    sr, pc, nr, nc = np.zeros(S, np.int32), np.zeros(len(point_seg), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    sc.seg_regions(oi.ctypes.data, of.ctypes.data, S, count.ctypes.data, colour.ctypes.data, off.ctypes.data, ns.ctypes.data,
                   nd.ctypes.data, point_seg.ctypes.data, len(point_seg), sr.ctypes.data, nr.ctypes.data, pc.ctypes.data, nc.ctypes.data)
    return sr, int(nr[0]), pc, int(nc[0])


def pack(r, g, b):
    return (np.asarray(r, np.uint32) << 16) | (np.asarray(g, np.uint32) << 8) | np.asarray(b, np.uint32)


def passthrough_z(xyz, lo=0.0, hi=14.0):
    xyz = _f(xyz)
    return np.nonzero(np.isfinite(xyz).all(1) & ~((xyz[:, 2] < np.float32(lo)) | (xyz[:, 2] > np.float32(hi))))[0].astype(np.int32)


PATCH_COLOURS = [(200, 40, 40), (40, 200, 40), (40, 40, 200), (200, 200, 40), (40, 200, 200), (200, 40, 200)]


def patch_scene(n, seed, salt=0.03, scale=1.0, close=False):
    """Six colour patches and a gradient patch (red 20..200 along x) on unit squares of a slightly wavy sheet at z ~ 1,
    colour noise of +-1 per channel, and `salt` of the points recoloured at random.  close: patches 1 and 2 get colours
    within the region threshold of patch 0's (the homogeneous merging joins them).  Returns xyz, rgb, patch id, salt mask."""
    rng = np.random.default_rng(seed)
    patch = rng.integers(0, 7, n)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x, y = (patch % 4) + u, (patch // 4) + v
    z = 1.0 + 0.05 * np.sin(3 * x) * np.cos(2 * y) + rng.normal(0, 1e-3, n)
    cols = list(PATCH_COLOURS)
    if close:
        cols[1], cols[2] = (202, 42, 41), (198, 38, 42)
    base = np.array(cols + [(0, 90, 160)])[patch]
    base[patch == 6, 0] = np.round(20 + 180 * u[patch == 6])
    rgb = base + rng.integers(-1, 2, (n, 3))
    is_salt = rng.uniform(size=n) < salt
    rgb[is_salt] = rng.integers(0, 256, (int(is_salt.sum()), 3))
    xyz = (np.c_[x, y, z] * [scale, scale, 1.0]).astype(np.float32)
    return xyz, pack(*rgb.T), patch, is_salt


# ---------------------------------------------------------------- the independent twin: rules 2-10, literally
def untie(xyz, ind, k, seed=0):
    """Moves, by a few parts in 1e5, the points that tie in some indexed point's candidate list, until no list has two
    equal float32 distances (a cloud of a few thousand float32 points has a handful of such pairs by chance; FLANN's
    order of them depends on its tree, so the comparisons keep clear of them)."""
    rng = np.random.default_rng(seed)
    xyz = _f(xyz).copy()
    for _ in range(20):
        cand, d2 = twin_knn(xyz, ind, k, check=False)
        rows, cols = np.nonzero(np.diff(d2, axis=1) <= 0)
        if len(rows) == 0:
            return xyz
        j = np.asarray(ind)[cand[rows, cols + 1]]
        xyz[j, :2] *= (1 + rng.uniform(1e-5, 3e-5, (len(j), 2))).astype(np.float32)
    raise AssertionError("could not make the cloud tie-free")


def twin_knn(xyz, ind, k, check=True):
    """Positions (in the index list) and float32 d2 of the min(k, n_idx) nearest indexed points in (d2, index) order,
    from scipy's double tree re-ranked with FLANN's float formula; asserts that no two candidates of a row tie (the
    8 candidates past the k-th included)."""
    pts = _f(xyz)[ind]
    m = len(pts)
    kk = min(k, m)
    q = min(kk + 8, m)
    _, cand = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=q)
    cand = cand.reshape(m, q)
    d = pts[:, None, :] - pts[cand]
    d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    order = np.lexsort((cand, d2), axis=1)
    cand, d2 = np.take_along_axis(cand, order, 1), np.take_along_axis(d2, order, 1)
    if not check:
        return cand, d2
    assert (np.diff(d2, axis=1) > 0).all(), "the cloud has tied neighbour distances"      # tie-free: asserted, not assumed
    return cand[:, :kk], d2[:, :kk]


def twin_segment(xyz, rgb, ind, o):
    """Returns (segment per list position, region per list position, clusters: lists of cloud indices, in order)."""
    rgb = _u(rgb)[ind]
    m = len(ind)
    nbr, d2 = twin_knn(xyz, ind, o["region_neighbour_number"])
    ch = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], 1).astype(np.int64)
    p2p = float(np.float32(o["point_color_threshold"]) * np.float32(o["point_color_threshold"]))
    r2r = float(np.float32(o["region_color_threshold"]) * np.float32(o["region_color_threshold"]))
    dist = float(np.float32(o["distance_threshold"]) * np.float32(o["distance_threshold"]))
    K = o["region_neighbour_number"]
    # rule 4: seeds in list order, a queue, the first neighbour_number entries, the difference to the current point
    lab, npts = [-1] * m, []
    for seed in range(m):
        if lab[seed] != -1:
            continue
        s = len(npts)
        lab[seed] = s
        cnt = 1
        q = deque([seed])
        while q:
            u = q.popleft()
            for e in range(min(o["neighbour_number"], nbr.shape[1])):
                w = int(nbr[u, e])
                if lab[w] != -1:
                    continue
                if float(((ch[u] - ch[w]) ** 2).sum()) > p2p:
                    continue
                lab[w] = s
                cnt += 1
                q.append(w)
        npts.append(cnt)
    S = len(npts)
    segs = [[] for _ in range(S)]                   # rule 5: ascending index
    for i in range(m):
        segs[lab[i]].append(i)
    # rule 6: segment neighbours through a max-heap of (d2, segment), stored in pop order
    snb, sd = [], []
    for s in range(S):
        best = {}
        for u in segs[s]:
            for e in range(nbr.shape[1]):
                b = lab[int(nbr[u, e])]
                if b != s and best.get(b, FLT_MAX) > float(d2[u, e]):
                    best[b] = float(d2[u, e])
        h = []
        for b in range(S):
            if b in best and best[b] < FLT_MAX:
                heapq.heappush(h, (-best[b], -b))
                if len(h) > K:
                    heapq.heappop(h)
        nb_, d_ = [], []
        while h:
            dd, bb = heapq.heappop(h)
            nb_.append(-bb)
            d_.append(-dd)
        snb.append(nb_)
        sd.append(d_)
    # rule 7
    col = [[int(np.float32(ch[segs[s], c].sum()) / np.float32(npts[s])) for c in range(3)] for s in range(S)]
    # rule 8: homogeneous merging
    slab, rpts, rnseg = [-1] * S, [], []
    for s in range(S):
        if slab[s] == -1:
            slab[s] = len(rpts)
            cur = len(rpts)
            rpts.append(npts[s])
            rnseg.append(1)
        else:
            cur = slab[s]
        e = 0
        while e < K and e < len(snb[s]):
            q = snb[s][e]
            if sd[s][e] > dist:
                e += 1
                continue
            if slab[q] == -1:
                if float(sum((a - b) ** 2 for a, b in zip(col[s], col[q]))) < r2r:
                    slab[q] = cur
                    rpts[cur] += npts[q]
                    rnseg[cur] += 1
            e += 1
    R = len(rpts)
    # rule 9: the regions' lists, then the small regions (eagerly, as PCL does it)
    final = [[] for _ in range(R)]
    for s in range(S):
        final[slab[s]].append(s)
    rnb = []
    for r in range(R):
        l = []
        for s in final[r]:
            for q, d in zip(snb[s], sd[s]):
                if d == FLT_MAX:
                    continue
                if slab[q] != r:
                    l.append((d, q))
        l.sort()
        rnb.append(l)
    for r in range(R):
        if rpts[r] < o["min_cluster_size"]:
            if not rnb[r]:
                continue
            if rnb[r][0][0] == FLT_MAX:
                continue
            to = slab[rnb[r][0][1]]
            for s in final[r]:
                final[to].append(s)
                slab[s] = to
            final[r] = []
            rpts[to] += rpts[r]
            rpts[r] = 0
            rnb[to] = [(FLT_MAX, 0) if slab[q] == to else (d, q) for d, q in rnb[to]]
            rnb[to] += [(d, q) for d, q in rnb[r] if slab[q] != to]
            rnb[r] = []
            rnb[to].sort()
    # rule 10: assembly in region order, points in list order; the swap-with-last compaction; the size limits
    clusters = [[] for _ in range(R)]
    for i in range(m):
        clusters[slab[lab[i]]].append(int(ind[i]))
    if clusters:
        i, j = 0, len(clusters) - 1
        while i < j:
            while clusters[i] and i < j:
                i += 1
            while not clusters[j] and i < j:
                j -= 1
            if i != j:
                clusters[i], clusters[j] = clusters[j], clusters[i]
        clusters = [c for c in clusters if c]
    clusters = [c for c in clusters if o["min_cluster_size"] <= len(c) <= o["max_cluster_size"]]
    return np.array(lab), np.array([slab[l] for l in lab]), clusters


def clusters_of(labels, nc):
    return [list(np.nonzero(labels == c)[0]) for c in range(nc)]


# ---------------------------------------------------------------- twin against stub
@pytest.mark.parametrize("seed,n,kw", [(1, 5000, dict(min_cluster_size=150)),
                                       (2, 4000, dict(min_cluster_size=300, close=True)),
                                       (3, 3000, dict(min_cluster_size=40, region_neighbour_number=20, neighbour_number=8)),
                                       (4, 6000, dict(min_cluster_size=600, max_cluster_size=1000, close=True)),
                                       (5, 3000, dict(min_cluster_size=100, point_color_threshold=1.5))])
def test_stub_equals_the_literal_twin(sc, seed, n, kw):
    kw = dict(kw)
    xyz, rgb, _, _ = patch_scene(n, seed, salt=0.05, close=kw.pop("close", False))
    xyz[::41, 2] = 20.0                                       # points the PassThrough drops
    xyz[7] = [np.nan, 0, 1]
    ind = passthrough_z(xyz)
    assert 0 < len(ind) < n
    o = ref_opts(**kw)
    xyz = untie(xyz, ind, o["region_neighbour_number"])
    t_seg, t_reg, t_clusters = twin_segment(xyz, rgb, ind, o)
    k = o["region_neighbour_number"]
    idx, d2 = stub_subset_knn(sc, xyz, ind, k)
    t_nbr, t_d2 = twin_knn(xyz, ind, k)
    assert np.array_equal(idx, ind[t_nbr]) and np.array_equal(d2.view(np.uint32), t_d2.view(np.uint32))
    seg, ns = stub_grow(sc, xyz, rgb, ind, o)
    assert ns == t_seg.max() + 1 and np.array_equal(seg[ind], t_seg)
    assert (np.delete(seg, ind) == -1).all()
    labels, nc, stats, reg = stub_segment(sc, xyz, rgb, ind, o)
    assert np.array_equal(reg, t_reg)
    assert clusters_of(labels, nc) == t_clusters                                    # the lists and their order
    assert list(stats[:2]) == [len(ind), ns] and nc >= 2
    assert ns > nc + 50                                                              # (salt: many small segments were merged away)
    if o["point_color_threshold"] < 6:                                               # fragments of one patch: rule 8 joins them
        assert stats[2] < 0.8 * ns


def test_planted_scene(sc):
    n = 30_000
    xyz, rgb, patch, is_salt = patch_scene(n, 11)
    ind = passthrough_z(xyz)
    assert len(ind) == n and np.bincount(patch).min() > 3000                        # every patch well over 600 points
    o = ref_opts()
    labels, nc, stats, _ = stub_segment(sc, xyz, rgb, ind, o)
    assert nc == 7 and (labels >= 0).all()
    sizes = np.bincount(labels)
    assert sizes.min() >= 600
    vote = [np.bincount(patch[labels == c], minlength=7).argmax() for c in range(nc)]
    assert sorted(vote) == list(range(7))                                            # one cluster per planted patch
    clean = ~is_salt
    assert np.array_equal(np.array(vote)[labels[clean]], patch[clean])              # exactly the patches
    assert stats[1] > 7 + 0.8 * is_salt.sum()                                        # the salt points grew segments of their own
    # rule 9: a salt point ends in the region of its nearest entry
    idx, _ = stub_subset_knn(sc, xyz, ind, 2)
    lone = np.nonzero(is_salt & ~is_salt[idx[:, 1]])[0]
    assert len(lone) > 0.9 * is_salt.sum()
    assert np.array_equal(labels[lone], labels[idx[lone, 1]])


# ---------------------------------------------------------------- rule cases built by hand
def _line(xs, cols, order=None):
    xyz = np.c_[np.asarray(xs, np.float32), np.zeros(len(xs)), np.ones(len(xs))].astype(np.float32)
    rgb = pack(*np.asarray(cols).T)
    if order is not None:
        xyz, rgb = xyz[order], rgb[order]
    return xyz, rgb


def test_neighbour_ranked_beyond_30_does_not_join(sc):
    A, B = (10, 10, 10), (200, 10, 10)
    xs = [0.0] + [1.0 + 0.37 * j for j in range(35)] + [40.0]
    xyz, rgb = _line(xs, [A] + [B] * 35 + [A])
    ind = np.arange(len(xs), dtype=np.int32)
    idx, _ = stub_subset_knn(sc, xyz, ind, 37)
    assert list(idx[0]).index(36) == 36                                              # rank 37 of 100 searched, beyond the first 30
    seg, ns = stub_grow(sc, xyz, rgb, ind, ref_opts())
    assert ns == 3 and seg[0] == 0 and seg[36] == 2 and (seg[1:36] == 1).all()
    seg, ns = stub_grow(sc, xyz, rgb, ind, ref_opts(neighbour_number=40))           # (within the entries looked at: it joins)
    assert ns == 2 and seg[36] == seg[0] == 0


def test_directed_pair_depends_on_index_order(sc):
    xs, cols = [0.0, 1.0, 1.5], [(50, 50, 50)] * 3                                    # u, v, w: u -> v, v -> w, w -> v with 2 entries
    o = ref_opts(neighbour_number=2, region_neighbour_number=2)
    xyz, rgb = _line(xs, cols)
    ind = np.arange(3, dtype=np.int32)
    idx, _ = stub_subset_knn(sc, xyz, ind, 2)
    assert idx.tolist() == [[0, 1], [1, 2], [2, 1]]                                  # v is in u's list, u is not in v's
    seg, ns = stub_grow(sc, xyz, rgb, ind, o)
    assert ns == 1 and list(seg) == [0, 0, 0]                                        # u first: u -> v -> w
    xyz, rgb = _line(xs, cols, order=[1, 2, 0])                                      # v, w, u: v's flood never reaches u
    seg, ns = stub_grow(sc, xyz, rgb, ind, o)
    assert ns == 2 and list(seg) == [0, 0, 1]


def test_colour_thresholds_are_inclusive_and_strict(sc):
    assert sc.seg_colour_diff(0x000000, 0x060000) == 36 and sc.seg_colour_diff(0x102030, 0x0F2232) == 9
    assert sc.seg_channel(10, 4) == 2 and sc.seg_channel(255 * 3, 3) == 255
    ind = np.arange(2, dtype=np.int32)
    for c, want in (((6, 0, 0), 1), ((6, 1, 0), 2), ((4, 4, 2), 1), ((4, 4, 3), 2)):  # 36 joins, 37 and 41 do not
        xyz, rgb = _line([0.0, 1.0], [(0, 0, 0), c])
        assert stub_grow(sc, xyz, rgb, ind, ref_opts())[1] == want
    # region colour: a difference of exactly 25 does not merge, 16 does; d2 == 100 is near enough, the next float is not
    o = ref_opts(min_cluster_size=1)
    above = float(np.nextafter(np.float32(100), np.float32(200)))
    for colour, d2, regions in (([(10, 10, 10), (15, 10, 10)], 1.0, 2), ([(10, 10, 10), (14, 10, 10)], 1.0, 1),
                                ([(10, 10, 10), (13, 14, 10)], 1.0, 2), ([(10, 10, 10), (14, 10, 10)], 100.0, 1),
                                ([(10, 10, 10), (14, 10, 10)], above, 2)):
        sr, nr, pc, nc = stub_regions(sc, o, [3, 2], colour, [[(1, d2)], [(0, d2)]], [0, 0, 0, 1, 1])
        assert nr == regions and nc == regions and list(pc) == ([0, 0, 0, 0, 0] if regions == 1 else [0, 0, 0, 1, 1])


def test_small_regions_and_compaction_by_hand(sc):
    # four segments of distinct colours in a row 0 - 1 - 2 - 3, sizes 5, 2, 6, 1; min 4: region 1 moves into its nearest
    # (segment 2, d2 1 against 4), region 3 into region 2; the emptied regions 1 and 3 are compacted away in place
    col = [(0, 0, 0), (100, 0, 0), (0, 100, 0), (0, 0, 100)]
    lists = [[(1, 4.0)], [(0, 4.0), (2, 1.0)], [(1, 1.0), (3, 9.0)], [(2, 9.0)]]
    pts = [0] * 5 + [1] * 2 + [2] * 6 + [3]
    sr, nr, pc, nc = stub_regions(sc, ref_opts(min_cluster_size=4), [5, 2, 6, 1], col, lists, pts)
    assert nr == 4 and list(sr) == [0, 2, 2, 2] and nc == 2
    assert list(pc) == [0] * 5 + [1] * 9
    # an emptied FIRST region takes the last one's place: the cluster order changes (rule 10)
    sr, nr, pc, nc = stub_regions(sc, ref_opts(min_cluster_size=4), [2, 6, 5], col[:3], [[(1, 1.0)], [(0, 1.0), (2, 4.0)], [(1, 4.0)]],
                                  [0] * 2 + [1] * 6 + [2] * 5)
    assert list(sr) == [1, 1, 2] and nc == 2 and list(pc) == [1] * 8 + [0] * 5
    # a region with no list stays and is erased by the size limit; so is one above the maximum
    sr, nr, pc, nc = stub_regions(sc, ref_opts(min_cluster_size=4, max_cluster_size=5), [2, 6, 5], col[:3], [[], [(2, 4.0)], [(1, 4.0)]],
                                  [0] * 2 + [1] * 6 + [2] * 5)
    assert nc == 1 and list(pc) == [-1] * 8 + [0] * 5


def test_points_outside_the_limits_and_short_lists(sc):
    xyz, rgb, _, _ = patch_scene(60, 5, salt=0.0)
    xyz[::6, 2] = [14.5, -0.25, 20, 15, np.nan, 30, -1, 16, 14.001, np.inf]
    xyz[1, 2], xyz[2, 2] = 14.0, 0.0                                                  # the limits are inclusive
    ind = passthrough_z(xyz)
    assert len(ind) == 50 and {1, 2} <= set(ind)                                      # n_idx < 100
    xyz = untie(xyz, ind, 100)
    idx, d2 = stub_subset_knn(sc, xyz, ind, 100)
    assert (idx[:, :50] >= 0).all() and (idx[:, 50:] == -1).all() and np.isinf(d2[:, 50:]).all()
    assert not np.isin(idx, np.arange(0, 60, 6)).any() and np.array_equal(idx[:, 0], ind)
    o = ref_opts(min_cluster_size=5)
    labels, nc, stats, _ = stub_segment(sc, xyz, rgb, ind, o)
    assert (labels[::6] == -1).all() and stats[0] == 50
    t_seg, t_reg, t_clusters = twin_segment(xyz, rgb, ind, o)
    assert clusters_of(labels, nc) == t_clusters and nc >= 1


def test_empty_or_malformed_index_list_is_an_error(sc):
    xyz, rgb, _, _ = patch_scene(20, 6)
    assert stub_segment(sc, xyz, rgb, np.zeros(0, np.int32), ref_opts()) == -3
    assert stub_segment(sc, xyz, rgb, [3, 2], ref_opts()) == -3
    assert stub_segment(sc, xyz, rgb, [1, 20], ref_opts()) == -3
    assert stub_segment(sc, xyz, rgb, [1, 2], ref_opts(region_neighbour_number=129)) == -3


# ---------------------------------------------------------------- bounds
def stub_minmax(sc, xyz):
    xyz = _f(xyz)
    mn, mx, h = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(1, np.float64)
    sc.seg_minmax(len(xyz), xyz.ctypes.data, mn.ctypes.data, mx.ctypes.data, h.ctypes.data)
    return mn, mx, float(h[0])


def test_bounds_against_numpy(sc):
    rng = np.random.default_rng(8)
    xyz = (rng.normal(size=(5000, 3)) * [3, 1, 7]).astype(np.float32)
    xyz[17] = [np.nan, 100, 100]                                                      # skipped whole: 100 is not the maximum
    xyz[18] = [0, -np.inf, 0]
    fin = np.isfinite(xyz).all(1)
    mn, mx, h = stub_minmax(sc, xyz)
    assert np.array_equal(mn, xyz[fin].min(0)) and np.array_equal(mx, xyz[fin].max(0))
    d = (mx - mn).astype(np.float32).astype(np.float64)
    assert h == np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    mn, mx, _ = stub_minmax(sc, np.zeros((0, 3), np.float32))
    assert (mn == np.float32(FLT_MAX)).all() and (mx == -np.float32(FLT_MAX)).all()


def ord_key_cases():
    """Bit patterns for the ordered keys: the zeros, the denormals' ends, the normals' ends, the infinities, quiet and
    signalling NaNs of both signs, and a million random patterns."""
    special = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF,
               0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF]
    rnd = np.random.default_rng(11).integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([np.array(special, np.uint32), rnd])


def check_ord_keys(fn):
    """The one ord_key / ord_val of csrc/cloud.h, through a stub's entry `fn`, against the rule segment.h and poisson.h
    each used to spell out: the sign bit set on a non-negative float, every bit flipped on a negative one."""
    u = ord_key_cases()
    key, back = np.zeros(len(u), np.uint32), np.zeros(len(u), np.uint32)
    fn(len(u), u.ctypes.data, key.ctypes.data, back.ctypes.data)
    neg = (u & np.uint32(0x80000000)) != 0
    assert np.array_equal(key, np.where(neg, ~u, u | np.uint32(0x80000000)))
    assert np.array_equal(back, u)                                                    # ord_val inverts it, NaN payloads included
    f = u.view(np.float32)
    num = ~np.isnan(f)
    o = np.argsort(key[num], kind="stable")
    assert (np.diff(f[num][o].astype(np.float64)) >= 0).all()                         # ascending keys: ascending floats, -inf .. +inf
    assert key[1] < key[0]                                                            # -0 below +0: the one pair of equal floats


def test_ord_keys_match_the_rule_both_headers_spelled(sc):
    check_ord_keys(sc.seg_ord_keys)


# ---------------------------------------------------------------- the XYZRGB PCD reader (pcllite.h)
def load_pcd_rgb(sc, path, cap=1 << 16):
    xyz, rgb, info = np.zeros((cap, 3), np.float32), np.zeros(cap, np.uint32), np.zeros(3, np.int32)
    n = sc.seg_load_pcd(str(path).encode(), xyz.ctypes.data, rgb.ctypes.data, cap, info.ctypes.data)
    return (None, None, info) if n < 0 else (xyz[:n].copy(), rgb[:n].copy(), info)


def _pcd_head(n, fields, sizes, types, data):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (fields, sizes, types, " ".join("1" * len(fields.split())), n, n, data)).encode()


def test_pcd_reader_ascii_and_binary(sc, tmp_path):
    rng = np.random.default_rng(9)
    n = 400
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    rgb = pack(*rng.integers(0, 256, (3, n)))
    rgb[:4] = [0, 0x00FFFFFF, 0x00800000, 0x007FFFFF]                                # zero, the largest, both sides of the subnormals
    as_float = rgb.view(np.float32)
    # ascii with 8 significant digits, the way convertPLYtoPCD writes it (the colour's bits as a float)
    body = "".join("%.8g %.8g %.8g %.8g\n" % (p[0], p[1], p[2], c) for p, c in zip(xyz, as_float))
    (tmp_path / "a.pcd").write_bytes(_pcd_head(n, "x y z rgb", "4 4 4 4", "F F F F", "ascii") + body.encode())
    got, col, info = load_pcd_rgb(sc, tmp_path / "a.pcd")
    p8 = np.array([np.float32("%.8g" % v) for v in xyz.ravel()], np.float32).reshape(xyz.shape)
    assert np.array_equal(got, p8) and np.array_equal(col, rgb) and list(info) == [n, 1, 1]
    rec = np.zeros(n, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")]))
    rec["x"], rec["y"], rec["z"], rec["rgb"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rgb
    for types in ("F F F F", "F F F U"):
        (tmp_path / "b.pcd").write_bytes(_pcd_head(n, "x y z rgb", "4 4 4 4", types, "binary") + rec.tobytes())
        got, col, info = load_pcd_rgb(sc, tmp_path / "b.pcd")
        assert np.array_equal(got, xyz) and np.array_equal(col, rgb) and list(info) == [n, 1, 1]
    body = "".join("%.8g %.8g %.8g %d\n" % (p[0], p[1], p[2], c) for p, c in zip(xyz, rgb))
    (tmp_path / "u.pcd").write_bytes(_pcd_head(n, "x y z rgba", "4 4 4 4", "F F F U", "ascii") + body.encode())
    assert np.array_equal(load_pcd_rgb(sc, tmp_path / "u.pcd")[1], rgb)
    # no colour field: colour 0; a nan coordinate: not dense; a truncated file: refused
    (tmp_path / "n.pcd").write_bytes(_pcd_head(2, "x y z", "4 4 4", "F F F", "ascii") + b"nan 1 2\n0.5 -1.25 3\n")
    got, col, info = load_pcd_rgb(sc, tmp_path / "n.pcd")
    assert np.isnan(got[0, 0]) and list(col) == [0, 0] and list(info) == [2, 1, 0]
    (tmp_path / "t.pcd").write_bytes(_pcd_head(n, "x y z rgb", "4 4 4 4", "F F F F", "binary") + rec.tobytes()[:-1])
    assert load_pcd_rgb(sc, tmp_path / "t.pcd")[0] is None


# ---------------------------------------------------------------- sanitizers
def test_segmentation_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "segment_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DSEGMENT_MAIN", "-o", exe, STUB])
    xyz, rgb, _, _ = patch_scene(6000, 2, salt=0.05, close=True)
    xyz[3] = [np.nan, 0, 0]
    xyz[::29, 2] = 15.0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(xyz)))
        f.write(xyz.astype("<f4").tobytes())
        f.write(rgb.astype("<u4").tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("segment rc 0 ")
