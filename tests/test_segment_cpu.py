"""The colour region growing after map3D (csrc/segment.h: pcl::RegionGrowingRGB behind a PassThrough on z, reference
src/Segmentation.cpp:3-66) and Dendrometry's bounds (src/DendrometryE.cpp:3-29) on the CPU, through a g++ build of the
header the device code compiles (tests/stub/segment_capi.cpp): an independent, literal Python transcription of rules
2-10 of DESIGN.md f-8 (queue growth, plain loops, scipy's neighbours re-ranked in float32) against the stub on seeded
clouds, a planted scene of colour patches, the rule cases built by hand, the small scenes of tests/segment_scenes.py
(the stub against the twin, or against numpy's brute force where distances tie, and the property each scene is named
for), the bounds against numpy, the XYZRGB PCD reader, and one cloud under ASan / UBSan.  No GPU.  PARITY UNPINNED: PCL is not in the image."""
import ctypes as C
import heapq
import os
import struct
import subprocess
from collections import deque

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import segment_scenes as scenes
from tests.segment_scenes import PATCH_COLOURS, _line, pack, patch_scene  # noqa: F401  (tests/test_gpu_segment.py takes them from here)

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


def passthrough_z(xyz, lo=0.0, hi=14.0):
    xyz = _f(xyz)
    return np.nonzero(np.isfinite(xyz).all(1) & ~((xyz[:, 2] < np.float32(lo)) | (xyz[:, 2] > np.float32(hi))))[0].astype(np.int32)


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


def brute_knn(xyz, ind, k):
    """Positions and float32 d2 of the min(k, finite rows) nearest indexed points by brute force: all pairwise d2 in float32,
    np.lexsort((position, d2)).  For clouds whose d2 are exact in float32 (the lattice scenes: ties are the rule there, and the
    order of a list is (d2, index) by definition); rows of non-finite points, and the columns past the list, are -1 / inf."""
    pts = _f(xyz)[ind]
    m = len(pts)
    fin = np.isfinite(pts).all(1)
    with np.errstate(invalid="ignore"):
        d = pts[:, None, :] - pts[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    d2[:, ~fin] = np.inf
    pos = np.broadcast_to(np.arange(m), (m, m))
    order = np.lexsort((pos, d2), axis=1)
    kk = min(k, int(fin.sum()))
    nbr, nd2 = np.full((m, k), -1, np.int64), np.full((m, k), np.inf, np.float32)
    nbr[:, :kk], nd2[:, :kk] = order[:, :kk], np.take_along_axis(d2, order[:, :kk], 1)
    nbr[~fin], nd2[~fin] = -1, np.inf
    return nbr, nd2


def twin_segment(xyz, rgb, ind, o, knn=None):
    """Returns (segment per list position, region per list position, clusters: lists of cloud indices, in order).  knn: the
    (positions, d2) lists to grow over, for a tied cloud the twin's own search refuses (brute_knn's, all rows finite)."""
    rgb = _u(rgb)[ind]
    m = len(ind)
    nbr, d2 = knn if knn is not None else twin_knn(xyz, ind, o["region_neighbour_number"])
    if knn is not None:
        nbr, d2 = nbr[:, :min(o["region_neighbour_number"], m)], d2[:, :min(o["region_neighbour_number"], m)]
        assert (nbr >= 0).all()
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


# ---------------------------------------------------------------- rule cases built by hand (the scenes: tests/segment_scenes.py)
def test_neighbour_ranked_beyond_30_does_not_join(sc):
    xyz, rgb, ind, kw = scenes.beyond_30()
    idx, _ = stub_subset_knn(sc, xyz, ind, 37)
    assert list(idx[0]).index(36) == 36                                              # rank 37 of 100 searched, beyond the first 30
    seg, ns = stub_grow(sc, xyz, rgb, ind, ref_opts(**kw))
    assert ns == 3 and seg[0] == 0 and seg[36] == 2 and (seg[1:36] == 1).all()
    xyz, rgb, ind, kw = scenes.beyond_30(neighbour_number=40)
    seg, ns = stub_grow(sc, xyz, rgb, ind, ref_opts(**kw))                           # (within the entries looked at: it joins)
    assert kw == dict(neighbour_number=40) and ns == 2 and seg[36] == seg[0] == 0


def test_directed_pair_depends_on_index_order(sc):
    xyz, rgb, ind, kw = scenes.directed_pair(True)                                   # u, v, w: u -> v, v -> w, w -> v with 2 entries
    o = ref_opts(**kw)
    assert kw == dict(neighbour_number=2, region_neighbour_number=2)
    idx, _ = stub_subset_knn(sc, xyz, ind, 2)
    assert idx.tolist() == [[0, 1], [1, 2], [2, 1]]                                  # v is in u's list, u is not in v's
    seg, ns = stub_grow(sc, xyz, rgb, ind, o)
    assert ns == 1 and list(seg) == [0, 0, 0]                                        # u first: u -> v -> w
    xyz, rgb, ind, kw = scenes.directed_pair(False)                                  # v, w, u: v's flood never reaches u
    seg, ns = stub_grow(sc, xyz, rgb, ind, o)
    assert ns == 2 and list(seg) == [0, 0, 1]


def test_colour_thresholds_are_inclusive_and_strict(sc):
    assert sc.seg_colour_diff(0x000000, 0x060000) == 36 and sc.seg_colour_diff(0x102030, 0x0F2232) == 9
    assert sc.seg_channel(10, 4) == 2 and sc.seg_channel(255 * 3, 3) == 255
    assert scenes.POINT_THRESHOLD_PAIRS == (((6, 0, 0), 1), ((6, 1, 0), 2), ((4, 4, 2), 1), ((4, 4, 3), 2))
    for c, want in scenes.POINT_THRESHOLD_PAIRS:                                     # 36 joins, 37 and 41 do not
        xyz, rgb, ind, kw = scenes.threshold_pair(c)
        assert stub_grow(sc, xyz, rgb, ind, ref_opts(**kw))[1] == want and kw == {}
    # region colour: a difference of exactly 25 does not merge, 16 does; d2 == 100 is near enough, the next float is not
    o = ref_opts(min_cluster_size=1)
    cases = scenes.region_threshold_cases()
    assert [(sc.seg_colour_diff(int(pack(*a)), int(pack(*b))), regions) for (a, b), _, regions in cases] == \
        [(25, 2), (16, 1), (25, 2), (16, 1), (16, 2)]
    assert [d2 for _, d2, _ in cases][:4] == [1.0, 1.0, 1.0, 100.0] and np.float32(cases[4][1]) == np.nextafter(np.float32(100), np.float32(200))
    for colour, d2, regions in cases:
        sr, nr, pc, nc = stub_regions(sc, o, [3, 2], colour, [[(1, d2)], [(0, d2)]], [0, 0, 0, 1, 1])
        assert nr == regions and nc == regions and list(pc) == ([0, 0, 0, 0, 0] if regions == 1 else [0, 0, 0, 1, 1])


def test_small_regions_and_compaction_by_hand(sc):
    # four segments of distinct colours in a row 0 - 1 - 2 - 3, sizes 5, 2, 6, 1; min 4: region 1 moves into its nearest
    # (segment 2, d2 1 against 4), region 3 into region 2; the emptied regions 1 and 3 are compacted away in place
    t = scenes.compaction_tables()
    kw, count, col, lists, pts, _ = t[0]
    assert (kw, count, lists) == (dict(min_cluster_size=4), [5, 2, 6, 1], [[(1, 4.0)], [(0, 4.0), (2, 1.0)], [(1, 1.0), (3, 9.0)], [(2, 9.0)]])
    sr, nr, pc, nc = stub_regions(sc, ref_opts(**kw), count, col, lists, pts)
    assert nr == 4 and list(sr) == [0, 2, 2, 2] and nc == 2
    assert list(pc) == [0] * 5 + [1] * 9
    # an emptied FIRST region takes the last one's place: the cluster order changes (rule 10)
    kw, count, col, lists, pts, _ = t[1]
    assert (kw, count, lists) == (dict(min_cluster_size=4), [2, 6, 5], [[(1, 1.0)], [(0, 1.0), (2, 4.0)], [(1, 4.0)]])
    sr, nr, pc, nc = stub_regions(sc, ref_opts(**kw), count, col, lists, pts)
    assert list(sr) == [1, 1, 2] and nc == 2 and list(pc) == [1] * 8 + [0] * 5
    # a region with no list stays and is erased by the size limit; so is one above the maximum
    kw, count, col, lists, pts, _ = t[2]
    assert (kw, count, lists) == (dict(min_cluster_size=4, max_cluster_size=5), [2, 6, 5], [[], [(2, 4.0)], [(1, 4.0)]])
    sr, nr, pc, nc = stub_regions(sc, ref_opts(**kw), count, col, lists, pts)
    assert nc == 1 and list(pc) == [-1] * 8 + [0] * 5
    for kw, count, col, lists, pts, (want_sr, want_nc, want_pc) in t:                # (what the scenes module hands the device tests)
        sr, nr, pc, nc = stub_regions(sc, ref_opts(**kw), count, col, lists, pts)
        assert (want_sr is None or list(sr) == want_sr) and nc == want_nc and list(pc) == want_pc
        assert [tuple(c) for c in col] == scenes.COMPACTION_COLOURS[:len(count)] and pts == [s for s, n in enumerate(count) for _ in range(n)]


def check_expectation(want, grow, whole):
    """A rule scene's expectation (segment_scenes.rule_scenes) against (segment [n], count) and (labels [n], clusters, regions)."""
    if "segments" in want:
        assert grow[1] == want["segments"][0] and list(grow[0]) == want["segments"][1]
    if "clusters" in want:
        assert whole[1] == want["clusters"][0] and list(whole[0]) == want["clusters"][1]
    if "regions" in want:
        assert whole[2] == want["regions"]


@pytest.mark.parametrize("name,scene,want", scenes.rule_scenes(), ids=[r[0] for r in scenes.rule_scenes()])
def test_rule_scenes_as_points(sc, name, scene, want):
    xyz, rgb, ind, kw = scene
    o = ref_opts(**kw)
    labels, nc, stats, _ = stub_segment(sc, xyz, rgb, ind, o)
    check_expectation(want, stub_grow(sc, xyz, rgb, ind, o), (labels, nc, stats[2]))


# ---------------------------------------------------------------- the small scenes: the stub against the twins, and what each is named for
def finite_rows_knn(xyz, ind, k, knn=twin_knn):
    """The reference lists of a list with non-finite rows: `knn` over the finite rows, as cloud indices; -1 / inf elsewhere."""
    ind = np.asarray(ind)
    fin = np.isfinite(_f(xyz)[ind]).all(1)
    idx, d2 = np.full((len(ind), k), -1, np.int32), np.full((len(ind), k), np.inf, np.float32)
    if fin.any():
        nbr, nd2 = knn(xyz, ind[fin], k)
        idx[fin, :nbr.shape[1]], d2[fin, :nbr.shape[1]] = np.where(nbr >= 0, ind[fin][np.maximum(nbr, 0)], -1), nd2
    return idx, d2


def ubits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_knn(got, xyz, ind, k, knn=twin_knn):
    idx, d2 = finite_rows_knn(xyz, ind, k, knn)
    assert np.array_equal(got[0], idx) and np.array_equal(ubits(got[1]), ubits(d2))


def reference_segmentation(xyz, rgb, ind, o, tied=False):
    """(segment [n], segments, labels [n], clusters, final region of every list position) from the literal twin; tied: over
    brute_knn's lists."""
    knn = brute_knn(xyz, ind, o["region_neighbour_number"]) if tied else None
    t_seg, t_reg, t_clusters = twin_segment(xyz, rgb, ind, o, knn=knn)
    n = len(_f(xyz))
    seg, labels = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    seg[ind] = t_seg
    for c, members in enumerate(t_clusters):
        labels[members] = c
    return seg, int(t_seg.max()) + 1, labels, len(t_clusters), t_reg


def check_stub_against_twin(sc, xyz, rgb, ind, o, tied=False):
    k = o["region_neighbour_number"]
    check_knn(stub_subset_knn(sc, xyz, ind, k), xyz, ind, k, brute_knn if tied else twin_knn)
    ref = reference_segmentation(xyz, rgb, ind, o, tied)
    seg, ns = stub_grow(sc, xyz, rgb, ind, o)
    assert ns == ref[1] and np.array_equal(seg, ref[0])
    labels, nc, stats, reg = stub_segment(sc, xyz, rgb, ind, o)
    assert nc == ref[3] and np.array_equal(labels, ref[2]) and list(stats[:2]) == [len(ind), ns] and np.array_equal(reg, ref[4])
    return ref + (int(stats[2]),)                                                    # (and the regions rule 8 opened, from the stub)


K_SWEEP = (1, 2, 3, 4, 5, 63, 64, 65, 99, 100, 101, 127, 128)
K_GROW = (2, 3, 5, 65, 127)


def sweep_lengths(k, n=300):
    return sorted({m for m in (1, 2, k - 1, k, k + 1, n) if 1 <= m <= n})


@pytest.mark.parametrize("k", K_SWEEP)
def test_scene_untied_sheet(sc, k):
    xyz, rgb, ind, kw = scenes.untied_sheet(300)
    for m in sweep_lengths(k):
        check_knn(stub_subset_knn(sc, xyz, ind[:m], k), xyz, ind[:m], k)             # (the twin asserts that no row ties)
    if k in K_GROW:
        ref = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**dict(kw, region_neighbour_number=k, neighbour_number=min(30, k))))
        assert ref[1] > 7


@pytest.mark.parametrize("k", [3, 27, 64, 101])
def test_scene_lattice(sc, k):
    xyz, rgb, ind, kw = scenes.lattice(6, 6, 3)
    idx, d2 = stub_subset_knn(sc, xyz, ind, k)
    check_knn((idx, d2), xyz, ind, k, brute_knn)
    assert set(np.unique(d2)) <= set(np.arange(0, 60, dtype=np.float32))             # small integers: exact in any order
    ties = np.diff(d2, axis=1) == 0
    assert ties.any(1).all() and ties.mean() > 0.3                                   # every list has ties, many of them
    assert (np.diff(idx, axis=1)[ties] > 0).all()                                    # and tied entries ascend by index


@pytest.mark.parametrize("k", [5, 100, 127])
def test_scene_far_clusters(sc, k):
    xyz, rgb, ind, kw, member = scenes.far_clusters(k)
    assert kw["region_neighbour_number"] == k and len(ind) >= k
    nbr, _ = twin_knn(xyz, ind, k)
    assert ((member[nbr[:, k - 1]] != member) | (member < 0)).all()                  # the k-th neighbour: in another cluster
    assert (member[nbr[:, 1]] == member)[member >= 0].all()                          # the nearest: in its own
    sizes = np.bincount(member[member >= 0])
    assert len(sizes) == 3 and (sizes < k).all() and (member < 0).sum() == 2
    for sub in (ind, ind[::3]):
        check_knn(stub_subset_knn(sc, xyz, sub, k), xyz, sub, k)
    check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**kw))


@pytest.mark.parametrize("k", [3, 100])
def test_scene_line(sc, k):
    xyz, rgb, ind, kw = scenes.line(5000)
    assert len(ind) == 5000 and (xyz[:, 1] == 0).all() and (xyz[:, 2] == 1).all() and (np.diff(xyz[:, 0]) > 0).all()
    assert np.diff(xyz[:, 0]).max() > 2 * np.diff(xyz[:, 0]).min()                   # unequal spacings
    for sub in (ind, ind[::3]):
        check_knn(stub_subset_knn(sc, xyz, sub, k), xyz, sub, k)
    if k == 100:
        ref = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**kw))
        assert ref[1] == 10


def with_holes(xyz, ind):
    """The scene with a few indexed rows made non-finite: every 7th gets a NaN, an inf or a -inf in one coordinate."""
    xyz = xyz.copy()
    rows = np.asarray(ind)[3::7]
    for j, r in enumerate(rows):
        xyz[r, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    return xyz, rows


def test_scene_holes_stub_against_twin(sc):
    for (xyz, _, ind, *_), k in ((scenes.far_clusters(100), 100), (scenes.line(5000), 3)):
        holed, rows = with_holes(xyz, ind)
        idx, d2 = stub_subset_knn(sc, holed, ind, k)
        check_knn((idx, d2), holed, ind, k)
        assert len(rows) > 3 and not np.isin(idx, rows).any() and (idx[np.isin(ind, rows)] == -1).all()


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("nn", [2, 3])
def test_scene_snake(sc, order, nn):
    m = 4097
    xyz, rgb, ind, kw = scenes.snake(m, order)
    o = ref_opts(**dict(kw, neighbour_number=nn))
    ref = check_stub_against_twin(sc, xyz, rgb, ind, o)
    assert ref[1] == 1 and (ref[0] == 0).all() and ref[3] == 1                       # one segment of m points
    # what the chain is made of: consecutive points within the point threshold, points two apart outside it
    chain = np.argsort(xyz[:, 0])
    ch = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], 1).astype(np.int64)[chain]
    assert (((ch[1:] - ch[:-1]) ** 2).sum(1) <= 36).all() and (((ch[2:] - ch[:-2]) ** 2).sum(1) > 36).all()
    nbr, _ = twin_knn(xyz, ind, 2)
    assert np.array_equal(nbr[chain[:-1], 1], chain[1:])                             # every point's nearest: the next of the chain
    assert chain[0] == 0 and {"ascending": chain[-1] == m - 1, "descending": chain[-1] == 1 and (np.diff(chain[1:]) == -1).all(),
                              "shuffled": (np.diff(chain) < 0).mean() > 0.4}[order]
    if nn == 2 and order == "ascending":      # the same chain indexed from its tail (m - 1, .., 1, 0): no seed reaches past its neighbour
        assert stub_grow(sc, xyz[::-1], rgb[::-1], ind, o)[1] == m - 1


@pytest.mark.parametrize("S", scenes.BLOB_SIZES)
def test_scene_blobs(sc, S):
    xyz, rgb, ind, kw, which = scenes.blobs(S)
    ref = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**kw))
    assert ref[1] == S and ref[3] == S and ref[5] == S                               # exactly S segments, clusters, regions
    first = [int(np.nonzero(which == b)[0][0]) for b in range(S)]
    assert np.array_equal(ref[0], np.argsort(np.argsort(first))[which])              # numbered by their smallest index
    if S > 1:
        nbr, _ = twin_knn(xyz, ind, kw["region_neighbour_number"])
        assert (which[nbr] != which[:, None]).any(1).all()                           # every point's list reaches another blob


def segment_neighbours(xyz, ind, k, seg, a):
    """Segment a's neighbour segments as (d2, segment), ascending: the minimum over its points' entries (rule 6, uncapped)."""
    nbr, d2 = brute_knn(xyz, ind, k)
    best = {}
    for u in np.nonzero(seg == a)[0]:
        for v, d in zip(nbr[u], d2[u]):
            if v >= 0 and seg[v] != a:
                best[int(seg[v])] = min(best.get(int(seg[v]), np.inf), float(d))
    return sorted((d, b) for b, d in best.items())


@pytest.mark.parametrize("keep", [1, 4, 5])
def test_scene_hub(sc, keep):
    n_sat = 12
    xyz, rgb, ind, kw, n_hub = scenes.hub(n_sat, keep)
    o = ref_opts(**kw)
    assert o["region_neighbour_number"] == keep and n_sat > keep
    ref = check_stub_against_twin(sc, xyz, rgb, ind, o, tied=True)
    if keep == 1:               # one neighbour searched: the point itself.  No list crosses a segment, so no segment has a neighbour
        assert ref[1] == len(ind) and ref[5] == len(ind) and segment_neighbours(xyz, ind, keep, ref[0], 0) == []
        return
    assert ref[1] == 1 + n_sat and (ref[0][:n_hub] == 0).all() and list(ref[0][n_hub:]) == list(range(1, n_sat + 1))
    nb = segment_neighbours(xyz, ind, keep, ref[0], 0)
    assert len(nb) == n_sat > keep                                                   # more neighbour segments than the cap keeps
    assert sorted(d for d, _ in nb) == [1 / 16] * 2 + [1 / 4] * 4 + [9 / 16] * 6
    assert nb[keep - 1][0] == nb[keep][0]                                            # the cap cuts between two tied satellites
    kept = [b for _, b in nb[:keep]]
    assert nb[keep][1] > nb[keep - 1][1] and kept != sorted(kept) and kept != list(range(1, keep + 1))
    # rule 8 merges what the hub's list keeps, and nothing else: the clusters show the cap and its tie-break
    assert ref[5] == 1 + n_sat - keep
    assert sorted(np.nonzero(ref[2] == ref[2][0])[0][n_hub:] - n_hub + 1) == sorted(kept)


def test_scene_thirds(sc):
    xyz, rgb, ind, kw, run = scenes.thirds()
    ref = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**kw))
    assert np.array_equal(ref[0], run) and ref[1] == 5 and list(np.bincount(run)) == [3, 7, 5, 5, 5]
    ch = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], 1).astype(np.int64)
    for s, c in ((0, 0), (1, 1)):
        total, n = int(ch[run == s, c].sum()), int((run == s).sum())
        assert total % n != 0 and sc.seg_channel(total, n) == total // n == int(round(total / n)) - 1   # truncated, not rounded
    lab = ref[2]
    A, B, D, E, F = (lab[run == j] for j in range(5))
    assert ref[5] == 4 and ref[3] == 4
    assert (A == A[0]).all() and (F == A[0]).all() and (D != A[0]).all() and (E != B[0]).all()           # rounded means: A + D, B + E


@pytest.mark.parametrize("m", [257, 1025])
def test_scene_every_point_its_own_segment(sc, m):
    xyz, rgb, ind, kw = scenes.untied_sheet(m, seed=m)
    ref = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**dict(kw, neighbour_number=1)))
    assert ref[1] == m and np.array_equal(ref[0], np.arange(m))


def test_scene_clamped_neighbour_number_and_zero_threshold(sc):
    xyz, rgb, ind, kw = scenes.untied_sheet(300)
    a = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**dict(kw, neighbour_number=200, region_neighbour_number=100)))
    b = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**dict(kw, neighbour_number=100, region_neighbour_number=100)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])                 # 200 entries of a list of 100: all of them
    z = check_stub_against_twin(sc, xyz, rgb, ind, ref_opts(**dict(kw, point_color_threshold=0.0)))
    seg = z[0]
    assert z[1] > a[1] and all(len(set(rgb[seg == s])) == 1 for s in range(z[1]))    # only equal colours join


def test_all_non_finite_and_single_rows(sc):
    xyz, rgb, ind, kw = scenes.untied_sheet(300)
    o = ref_opts(**kw)
    none = xyz.copy()
    none[ind[:40], 0] = np.nan
    labels, nc, stats, _ = stub_segment(sc, none, rgb, ind[:40], o)
    assert (labels == -1).all() and nc == 0 and list(stats) == [0, 0, 0, 0]
    seg, ns = stub_grow(sc, none, rgb, ind[:40], o)
    assert (seg == -1).all() and ns == 0
    idx, d2 = stub_subset_knn(sc, none, ind[:40], 5)
    assert (idx == -1).all() and np.isinf(d2).all()
    one = none.copy()
    one[17] = xyz[17]
    labels, nc, stats, _ = stub_segment(sc, one, rgb, ind[:40], ref_opts(min_cluster_size=1))
    assert nc == 1 and list(np.nonzero(labels == 0)[0]) == [17] and list(stats[:3]) == [1, 1, 1]
    seg, ns = stub_grow(sc, one, rgb, ind[:40], o)
    assert ns == 1 and list(np.nonzero(seg == 0)[0]) == [17] and (np.delete(seg, 17) == -1).all()
    check_knn(stub_subset_knn(sc, one, ind[:40], 3), one, ind[:40], 3)
    labels, nc, stats, _ = stub_segment(sc, xyz[:1], rgb[:1], ind[:1], ref_opts(min_cluster_size=1))    # a cloud of one point
    assert list(labels) == [0] and nc == 1 and list(stats[:3]) == [1, 1, 1]


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
