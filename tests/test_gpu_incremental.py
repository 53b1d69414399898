"""GPU: find2D3DMatches association and mergeNewPoints through the C ABI, bit-exact against the
oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sfm_danpipeline_amd import incremental, synth, triangulate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 256            # csrc/incremental.hip: cloud points, matches and new points per workgroup
R01 = np.float32(0.01)


@pytest.mark.parametrize("n_cloud,n_matches,seed,done,new", [(1, 1, 1, 0, 1), (300, 120, 2, 2, 5), (300, 120, 3, 5, 2),
                                                             (5000, 390, 4, 1, 7), (100000, 400, 5, 6, 0)])
def test_find_2d3d_vs_oracle(ctx, orc, n_cloud, n_matches, seed, done, new):
    cloud, matches = synth.random_tracks_and_matches(n_cloud, 8, n_matches, seed=seed, done_view=done)
    ptr, views, feats = synth.tracks_to_csr(cloud)
    mq, mt = [m[0] for m in matches], [m[1] for m in matches]
    oc, of = incremental.find_2d3d(ptr, views, feats, done, new, mq, mt, ctx=ctx)
    rc, rf = orc.find_2d3d(ptr, views, feats, done, new, mq, mt)
    assert np.array_equal(oc, rc) and np.array_equal(of, rf)          # bit-exact, cloud order


def test_find_2d3d_edges(ctx, orc):
    cloud = [{0: 7, 1: 3}, {1: 3}, {0: 9}, {1: 4, 2: 8}]
    ptr, views, feats = synth.tracks_to_csr(cloud)
    oc, of = incremental.find_2d3d(ptr, views, feats, 1, 0, [5, 6, 2], [3, 3, 4], ctx=ctx)
    assert list(oc) == [0, 1, 3] and list(of) == [5, 5, 2]            # first match on a repeated trainIdx wins
    oc, of = incremental.find_2d3d(ptr, views, feats, 1, 0, [], [], ctx=ctx)
    assert len(oc) == 0
    oc, of = incremental.find_2d3d([0], [], [], 1, 0, [1], [2], ctx=ctx)
    assert len(oc) == 0
    oc, of = incremental.find_2d3d(ptr, views, feats, 5, 0, [5, 6, 2], [3, 3, 4], ctx=ctx)   # nobody saw view 5
    assert len(oc) == 0


def test_find_2d3d_matches_builds_the_reference_vectors(ctx, orc):
    sc = synth.two_view_scene(50, seed=3)
    cloud = [dict(pt=tuple(np.array([i, 2 * i, 3 * i], float)), idxImage={0: i, 1: 49 - i}, pt2D={}) for i in range(50)]
    q = np.arange(0, 50, 2)
    t = 49 - q
    p3, p2 = incremental.find_2d3d_matches(cloud, 1, 0, q, t, sc["xy2"], ctx=ctx)
    assert np.array_equal(p3[:, 0], q.astype(float)) and np.array_equal(p2, sc["xy2"][t])


@pytest.mark.parametrize("n_cloud,n_new,seed", [(0, 5, 1), (1, 1, 2), (255, 257, 3), (4000, 3000, 4), (50000, 2000, 5)])
def test_merge_vs_oracle(ctx, orc, n_cloud, n_new, seed):
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-1, 1, (n_cloud, 3))
    k = min(n_cloud, n_new // 3)
    near = cloud[rng.choice(n_cloud, k, replace=False)] + rng.normal(0, 0.004, (k, 3)) if k else np.zeros((0, 3))
    dup = rng.uniform(2, 3, (max(n_new // 6, 1), 3))
    new = np.concatenate([near, dup, dup + rng.normal(0, 0.004, dup.shape), rng.uniform(-1, 1, (max(n_new - 2 * len(dup) - k, 0), 3))])
    rng.shuffle(new)
    acc, n = incremental.merge_accept(cloud, new, ctx=ctx)
    racc, rn = orc.merge_new_points(cloud, new)
    assert np.array_equal(acc, racc) and n == rn
    assert 0 < n < len(new) or len(new) <= 1


def test_merge_chain_and_threshold(ctx, orc):
    chain = np.stack([np.arange(40) * 0.006 + 3.0, np.zeros(40), np.zeros(40)], 1)
    acc, n = incremental.merge_accept(np.zeros((1, 3)), chain, ctx=ctx)
    assert np.array_equal(acc, orc.merge_new_points(np.zeros((1, 3)), chain)[0])
    assert list(acc) == [True, False] * 20                           # 40-deep in-order dependency
    r = np.float64(np.float32(0.01))
    pts = np.array([[r, 0, 0], [0, np.nextafter(r, 0), 0], [0, 0, 0.01]])
    acc, _ = incremental.merge_accept(np.zeros((1, 3)), pts, ctx=ctx)
    assert list(acc) == [True, False, True]                           # < (double)(float)0.01, like cv::norm(..) < 0.01f
    acc, n = incremental.merge_accept(np.zeros((3, 3)), np.zeros((0, 3)), ctx=ctx)
    assert n == 0


def test_merge_new_points_appends_in_order(ctx):
    cloud = [dict(pt=(0.0, 0.0, 0.0), idxImage={0: 1, 1: 2}, pt2D={})]
    new = [dict(pt=(0.0, 0.0, 0.005), idxImage={0: 3, 2: 4}, pt2D={}), dict(pt=(1.0, 0.0, 0.0), idxImage={1: 5, 2: 6}, pt2D={}),
           dict(pt=(1.0, 0.0, 0.002), idxImage={1: 7, 2: 8}, pt2D={})]
    assert incremental.merge_new_points(cloud, new, ctx=ctx) == 1
    assert len(cloud) == 2 and cloud[1]["idxImage"] == {1: 5, 2: 6}   # tracks are never merged (src/Sfm.cpp:1225)


# ---------------------------------------------------------------------------------------------------------------------
# The shapes the kernels of csrc/incremental.hip can break at.  Every comparison is np.array_equal against the oracle
# (plus a hand-written expectation where one exists); every case first asserts, on the oracle's answer alone, that it
# exercises what it is for.


def random_csr(n_cloud, seed, n_views=8, n_feat=400, see=()):
    """Tracks as CSR without a Python loop per point: a random non-empty subset of n_views views per point (from random
    bits; np.nonzero walks row-major, so the views of a point ascend), random features below n_feat.  `see` lists
    (point, view, feature) triples that the tracks must hold."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(1, 1 << n_views, n_cloud)
    for p, v, _ in see:
        bits[p] |= 1 << v
    seen = ((bits[:, None] >> np.arange(n_views)) & 1).astype(bool)
    _, views = np.nonzero(seen)
    ptr = np.zeros(n_cloud + 1, np.int32)
    ptr[1:] = np.cumsum(seen.sum(1))
    feats = rng.integers(0, n_feat, len(views)).astype(np.int32)
    for p, v, f in see:
        feats[ptr[p] + int(seen[p, :v].sum())] = f
    return ptr, views.astype(np.int32), feats


def random_matches(n_matches, seed, n_feat=400):
    """queryIdx unique and ascending like getMatching, trainIdx with repeats (synth.random_tracks_and_matches' rule)."""
    rng = np.random.default_rng(seed)
    q = np.sort(rng.permutation(n_feat)[:n_matches]).astype(np.int32)
    t = rng.integers(0, n_feat // 2, n_matches).astype(np.int32)
    return q, t


def _find_both(ctx, orc, ptr, views, feats, done, new, mq, mt, check=None):
    rc, rf = orc.find_2d3d(ptr, views, feats, done, new, mq, mt)
    if check is not None:
        check(rc, rf)                                   # non-vacuity, on the oracle's answer alone
    oc, of = incremental.find_2d3d(ptr, views, feats, done, new, mq, mt, ctx=ctx)
    assert np.array_equal(oc, rc) and np.array_equal(of, rf)
    return oc, of


@pytest.mark.parametrize("done,new", [(2, 5), (5, 2)])
@pytest.mark.parametrize("n_cloud", [262144, 262145, 524801])
def test_find_2d3d_scan_carries_across_trips(ctx, orc, n_cloud, done, new):
    """scan_kernel's loop (incremental.hip, `for (base = 0; base < n; base += 1024)`): 1024, 1025 and 2051 block counts
    are one, two and three trips, so the LDS `carry`, the third __syncthreads() and the re-use of `wsum` run.  A wrong
    carry shifts every output of block 1024 onwards; a missing barrier shows as a torn offset."""
    mq, mt = random_matches(390, seed=7)
    key = mq if done < new else mt
    nblk = (n_cloud + BLK - 1) // BLK
    edge = sorted({1023 * BLK, min(1024 * BLK, n_cloud - 1), n_cloud - 1})  # a survivor on each side of every trip's edge
    ptr, views, feats = random_csr(n_cloud, seed=n_cloud % 1000 + done, see=[(p, done, int(key[0])) for p in edge])

    def check(rc, rf):
        blocks = set((rc // BLK).tolist())
        assert 1023 in blocks and nblk - 1 in blocks and (nblk <= 1024 or 1024 in blocks)
        assert rc[-1] == n_cloud - 1 and 0 < len(rc) < n_cloud
        trips = (nblk + 1023) // 1024
        assert trips == {262144: 1, 262145: 2, 524801: 3}[n_cloud]
        for t in range(trips):                                              # every trip carries a non-zero total out
            assert np.any((rc // BLK) // 1024 == t)

    _find_both(ctx, orc, ptr, views, feats, done, new, mq, mt, check)


@pytest.mark.parametrize("n_cloud", [63, 64, 65, 255, 256, 257, 513])
def test_find_2d3d_survivor_patterns(ctx, orc, n_cloud):
    """assoc_kernel's ballot + popcount per wave and compact_pairs_kernel's `b & ((1ull << lane) - 1)` at lane 63, the
    four wave sums and the block offset: all points survive, none, only the first, only the last, every second one.
    Point p sees the done view with feature p; the match list holds the chosen features."""
    ptr = np.arange(n_cloud + 1, dtype=np.int32)
    views = np.zeros(n_cloud, np.int32)
    feats = np.arange(n_cloud, dtype=np.int32)
    patterns = dict(all=np.arange(n_cloud), none=np.zeros(0, int), first=np.array([0]), last=np.array([n_cloud - 1]),
                    second=np.arange(0, n_cloud, 2), odd=np.arange(1, n_cloud, 2))
    for name, chosen in patterns.items():
        # 'none' still runs every kernel: its matches key features that no point has
        key = chosen if len(chosen) else np.array([n_cloud + 5, n_cloud + 6])
        other = 1000 + key
        for done, new, mq, mt in ((0, 1, key, other), (0, 0, other, key)):   # queryIdx keyed, then trainIdx keyed
            def check(rc, rf):
                assert np.array_equal(rc, chosen) and np.array_equal(rf, 1000 + chosen), name
            _find_both(ctx, orc, ptr, views, feats, done, new, mq[::-1].copy(), mt[::-1].copy(), check)


@pytest.mark.parametrize("n_match", [1, 255, 256, 257, 5000])
def test_find_2d3d_lowest_match_index_wins_across_blocks(ctx, orc, n_match):
    """first_match_kernel's atomicMin (incremental.hip): feature F repeats on the key side once in every block of 256
    matches (index 200 in block 0, index 3 of every later block), feature G from the last lane of block 1 onwards.  The
    table must hold the LOWEST match index whatever order the workgroups run in; every other key is unique."""
    F, G = 5, 6
    key = (10 + np.arange(n_match)).astype(np.int32)
    other = (100000 + np.arange(n_match)).astype(np.int32)
    pos_f = [min(200, n_match - 1)] + [b * BLK + 3 for b in range(1, (n_match + BLK - 1) // BLK) if b * BLK + 3 < n_match]
    pos_g = [b * BLK + (BLK - 1 if b == 1 else 9) for b in range(1, (n_match + BLK - 1) // BLK) if b * BLK + BLK - 1 < n_match]
    key[pos_f] = F
    key[pos_g] = G
    taken = set(pos_f) | set(pos_g)
    uniq = [j for j in (0, 1, 254, 255, 256, 257, n_match - 2, n_match - 1) if 0 <= j < n_match and j not in taken]
    track_feats = [F, G, 9, 10 + n_match] + [10 + j for j in sorted(set(uniq))]      # 9 and 10 + n_match: no match keys them
    cloud = [{1: f} for f in track_feats]
    ptr, views, feats = synth.tracks_to_csr(cloud)
    exp_c, exp_f = [0], [100000 + pos_f[0]]
    if pos_g:
        exp_c, exp_f = exp_c + [1], exp_f + [100000 + pos_g[0]]
    for k, j in enumerate(sorted(set(uniq))):
        exp_c, exp_f = exp_c + [4 + k], exp_f + [100000 + j]
    assert len(pos_f) == (n_match + BLK - 1) // BLK or n_match % BLK <= 3       # F sits in every (full enough) block
    for done, new, mq, mt in ((1, 2, key, other), (1, 0, other, key)):

        def check(rc, rf):
            assert list(rc) == exp_c and list(rf) == exp_f

        _find_both(ctx, orc, ptr, views, feats, done, new, mq, mt, check)


def test_find_2d3d_large_table_and_features_outside_it(ctx, orc):
    """A key of 2 000 000 makes `tbl_n` 2 000 001 (the host loop over key_h, the 8 MB memset of `first`).  Track features
    equal to tbl_n, above it and negative must fail assoc_kernel's `f >= 0 && f < tbl_n` instead of indexing the table."""
    key, other = [3, 2000000, 3, 8], [11, 12, 13, 14]
    tbl_n = max(key) + 1
    track_feats = [2000000, tbl_n, tbl_n + 1, 2**31 - 1, -1, -7, -2**31, 3, 1999999, 0, 8]
    ptr, views, feats = synth.tracks_to_csr([{4: f} for f in track_feats])
    for done, new, mq, mt in ((4, 6, key, other), (4, 1, other, key)):

        def check(rc, rf):
            assert list(rc) == [0, 7, 10] and list(rf) == [12, 11, 14]

        _find_both(ctx, orc, ptr, views, feats, done, new, mq, mt, check)


@pytest.mark.parametrize("done,new", [(0, 4), (3, 4), (7, 9), (7, 4), (3, 0), (0, 0), (3, 3), (7, 7)])
def test_find_2d3d_track_shapes(ctx, orc, done, new):
    """assoc_kernel's walk `for (e = trk_ptr[p]; e < trk_ptr[p + 1]; ++e)`: rows with no entry at all (first, between,
    last), rows of eight entries with the done view first, in the middle and last, and done_view == new_view (not
    'left', so trainIdx is the key: `left = done_view < new_view`)."""
    cloud = [{}, {v: 10 + v for v in range(8)}, {}, {v: 20 + v for v in range(8)}, {}, {}]
    ptr, views, feats = synth.tracks_to_csr(cloud)
    fwd = [(a + v, 100 + a + v) for a in (10, 20) for v in range(8)]
    matches = fwd + [(t, q) for q, t in fwd]            # either side as key gives the same answer
    mq, mt = [m[0] for m in matches], [m[1] for m in matches]

    def check(rc, rf):
        assert list(rc) == [1, 3] and list(rf) == [110 + done, 120 + done]

    _find_both(ctx, orc, ptr, views, feats, done, new, mq, mt, check)


def test_find_2d3d_passes_over_a_negative_other_side(ctx, orc):
    """first_match_kernel's `other[m] >= 0`: the reference's scan only stops at a match whose other side is >= 0
    (src/Sfm.cpp:1062-1082), so the table holds the first USABLE match on a key.  Before the kernel took the other side
    it answered [1], [9] on the first example: the -1 won the atomicMin and the point was dropped."""
    ptr, views, feats = synth.tracks_to_csr([{1: 3}, {1: 4}])

    def check(rc, rf):
        assert list(rc) == [0, 1] and list(rf) == [7, 9]

    oc, of = _find_both(ctx, orc, ptr, views, feats, 1, 0, [-1, 7, 9], [3, 3, 4], check)
    assert list(oc) == [0, 1] and list(of) == [7, 9]
    # unusable matches before, between and after the usable one, in one block and spread over three, on both sides
    n = 700
    key = (1000 + np.arange(n)).astype(np.int32)
    other = np.arange(n, dtype=np.int32)
    key[[1, 300, 520, 600, 690]] = 6
    other[[1, 300, 520, 600, 690]] = [-1, -2, 77, -3, 88]
    key[[2, 3, 4, 5, 6]] = 3
    other[[2, 3, 4, 5, 6]] = [-5, -1, 8, -2, 6]
    key[[7, 699]] = 4
    other[[7, 699]] = [-9, -2**31]                       # a key with no usable match at all
    key[[8, 9]] = 5
    other[[8, 9]] = [0, -3]                              # 0 is usable
    ptr, views, feats = synth.tracks_to_csr([{1: 3}, {1: 4}, {1: 5}, {1: 6}, {1: 3}, {1: 1010}])

    def check2(rc, rf):
        assert list(rc) == [0, 2, 3, 4, 5] and list(rf) == [8, 0, 77, 8, 10]

    _find_both(ctx, orc, ptr, views, feats, 1, 2, key, other, check2)      # done < new: queryIdx is the key
    _find_both(ctx, orc, ptr, views, feats, 1, 0, other, key, check2)      # done > new: trainIdx is the key


# ---------------------------------------------------------------- merge
FAR = np.full((1, 3), 1000.0)


def _merge_both(ctx, orc, cloud, new, r=R01, check=None):
    r = float(np.float32(r))
    racc, rn = orc.merge_new_points(cloud, new, min_dist=r)
    assert rn == racc.sum()
    if check is not None:
        check(racc)
    acc, n = incremental.merge_accept(cloud, new, min_dist=r, ctx=ctx)
    assert np.array_equal(acc, racc) and n == rn
    return acc


def _lattice(n, off):
    j = np.arange(n)
    return np.stack([j % 16, (j // 16) % 16, j // 256], 1).astype(np.float64) + off


@pytest.mark.parametrize("n_cloud", [255, 256, 257, 1023, 1024, 1025, 2049])
def test_merge_tile_edges(ctx, orc, n_cloud):
    """near_cloud_kernel's staging (256 cloud points per LDS tile, `m = min(BLK, hi - base)`), its slices of 1024
    (`blockIdx.y`), the sticky `found` and the clamp of the last block's idle rows to row 0 (`ii = i < n_new ? i : 0`,
    row 0 is a probe here): the only near cloud point sits at index 0, 255, 256, 1023, 1024 or n_cloud - 1."""
    cloud = _lattice(n_cloud, 0.0)
    cands = sorted({c for c in (0, 255, 256, 1023, 1024, n_cloud - 1) if c < n_cloud})
    probes = [0, 255, 256, 514]
    steps = np.array([[0.004, 0, 0], [0, -0.004, 0], [0, 0, 0.004], [-0.003, 0.003, 0]])       # all within r / 2 = 0.005
    for rnd in range((len(cands) + 3) // 4):
        new = _lattice(515, 0.5)                          # nothing within 0.86 of any cloud point or of another new point
        near_of = [cands[(4 * rnd + k) % len(cands)] for k in range(4)]
        for k, (i, c) in enumerate(zip(probes, near_of)):
            new[i] = cloud[c] + steps[k]
        d = np.linalg.norm(new[:, None, :] - cloud[None, :, :], axis=2)
        assert np.array_equal(np.nonzero((d < 0.01).any(1))[0], probes) and np.all((d[probes] < 0.005).sum(1) == 1)
        assert [int(np.argmin(d[i])) for i in probes] == near_of
        expect = np.ones(515, bool)
        expect[probes] = False

        def check(racc):
            assert np.array_equal(racc, expect)            # exactly the probes are rejected

        _merge_both(ctx, orc, cloud, new, check=check)


def test_merge_chain_across_blocks(ctx, orc):
    """resolve_kernel's relaxation across workgroups: a chain of 700 points 0.006 apart crosses two block edges, and each
    point's decision waits for `state[j]` of its predecessor, which another workgroup writes in the same or an earlier
    sweep.  Accept alternates; then two independent chains interleaved in index order (neighbours two apart, chains
    crossing five block edges)."""
    k = np.arange(700)
    a = np.stack([3.0 + 0.006 * k, np.zeros(700), np.zeros(700)], 1)

    def check(racc):
        assert np.array_equal(racc, k % 2 == 0) and racc.sum() == 350

    _merge_both(ctx, orc, FAR, a, check=check)
    b = np.stack([np.zeros(700), 50.0 + 0.006 * k[::-1], np.zeros(700)], 1)      # the second chain runs downwards
    both = np.empty((1400, 3))
    both[0::2], both[1::2] = a, b

    def check2(racc):
        assert np.array_equal(racc[0::2], k % 2 == 0) and np.array_equal(racc[1::2], k % 2 == 0)

    _merge_both(ctx, orc, FAR, both, check=check2)


def test_merge_pile_of_duplicates(ctx, orc):
    """resolve_kernel when every thread waits on point 0 (`wait = true` in all four workgroups in the first sweep):
    1000 copies of one point, only the first is appended; none once the cloud holds that point (init_state_kernel)."""
    pt = np.array([[0.3, -1.7, 2.9]])
    pile = np.repeat(pt, 1000, 0)

    def check(racc):
        assert racc[0] and racc.sum() == 1

    _merge_both(ctx, orc, FAR, pile, check=check)

    def check0(racc):
        assert racc.sum() == 0

    _merge_both(ctx, orc, np.concatenate([FAR, pt]), pile, check=check0)


def _mix():
    rng = np.random.default_rng(9)
    base = rng.uniform(-1, 1, (40, 3))
    new = np.concatenate([base, base[:10], base[:5] + 0.001, [[np.nan, 0, 0], [0, np.nan, 1], [np.nan] * 3]])
    nan_rows = np.arange(55, 58)
    return base[20:30] + 0.002, new, nan_rows


@pytest.mark.parametrize("r", [0.0, -1.0, np.nan, np.inf], ids=["0", "-1", "nan", "inf"])
def test_merge_min_dist_outside_the_positive_reals(ctx, orc, r):
    """The host's threshold search (incremental.hip, `if (!(r > 0)) thr = -1.0` and the two nextafter loops): nothing is
    closer than 0, -1 or NaN, so everything is appended; everything finite is closer than +inf (thr = DBL_MAX), so only
    the rows with a NaN coordinate are."""
    cloud, new, nan_rows = _mix()

    def check(racc):
        if np.isinf(r):
            assert np.array_equal(np.nonzero(racc)[0], nan_rows)
        else:
            assert racc.all()

    _merge_both(ctx, orc, cloud, new, r=np.float32(r), check=check)


@pytest.mark.parametrize("r", [0.01, 0.003, 0.1, 1.0, 1e-20, 1e19], ids=str)
def test_merge_threshold_to_the_ulp(ctx, orc, r):
    """`sqrt(s) < r` restated as `s <= thr` (incremental.hip, the host search for thr): the six axis points at distance d
    from the origin, d the seven doubles from three below (double)(float)r to three above.  sqrt(d * d) == d in IEEE
    double, so a point is appended iff d >= r; the axis points are r * sqrt(2) apart and never block one another."""
    r32 = np.float32(r)
    rd = np.float64(r32)
    ds = [rd]
    for _ in range(3):
        ds = [np.nextafter(ds[0], 0.0)] + ds + [np.nextafter(ds[-1], np.inf)]
    assert len(set(ds)) == 7 and ds[3] == rd
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    for d in ds:

        def check(racc):
            assert racc.all() if d >= rd else not racc.any()

        _merge_both(ctx, orc, np.zeros((1, 3)), axes * d, r=r32, check=check)


def test_merge_non_finite_coordinates(ctx, orc):
    """dist2 with NaN / inf / overflowing coordinates in both clouds, at the tile and block edges of near_cloud_kernel and
    resolve_kernel: `s <= thr` is false for a NaN or infinite s exactly where `sqrt(s) < r` is."""
    rng = np.random.default_rng(21)
    cloud = rng.uniform(-1, 1, (1025, 3))
    bad = [np.nan, np.inf, -np.inf, 1e200, -1e200]
    for k, j in enumerate([0, 255, 256, 1023, 1024]):
        cloud[j, k % 3] = bad[k]
    new = rng.uniform(2, 3, (515, 3))
    new[[10, 250, 260, 500]] = cloud[[1, 254, 257, 1022]] + 0.003     # near one existing point each
    for k, i in enumerate([0, 255, 256, 514]):
        new[i] = new[(i + 7) % 515]                        # a copy of a later / earlier row ...
        new[i, (k + 1) % 3] = bad[k]                       # ... with one coordinate non-finite
    new[100] = [np.inf, np.inf, 0]
    new[101] = [np.inf, np.inf, 0]                         # inf - inf = NaN: not near its twin
    new[300:310] = new[290:300] + 0.001                    # in-call duplicates next to the block edge

    def check(racc):
        assert racc[[0, 255, 256, 514, 100, 101]].all()
        assert not racc[300:310].any()
        assert not racc[[10, 250, 260, 500]].any()

    _merge_both(ctx, orc, cloud, new, check=check)


# ---------------------------------------------------------------- all three entry points
def mid_cases():
    """One mid-sized input of each entry point (shared with the poisoned child process)."""
    ptr, views, feats = random_csr(5000, seed=31)
    mq, mt = random_matches(390, seed=32)
    rng = np.random.default_rng(33)
    cloud = rng.uniform(-1, 1, (3000, 3))
    new = np.concatenate([cloud[:700] + rng.normal(0, 0.004, (700, 3)), rng.uniform(-1, 1, (1300, 3))])
    new[1500:1600] = new[1400:1500] + 0.002
    sc = synth.two_view_scene(1500, seed=34)
    return (ptr, views, feats, 2, 5, mq, mt), (cloud, new), (sc["P1"], sc["P2"], sc["K"], np.array([-0.05, 0.01, 1e-4, -2e-4, 0.001]), sc["xy1"], sc["xy2"])


def run_mid_cases(ctx=None):
    f, m, t = mid_cases()
    oc, of = incremental.find_2d3d(*f, ctx=ctx)
    acc, n = incremental.merge_accept(*m, ctx=ctx)
    X, err, keep = triangulate.triangulate_points(*t, ctx=ctx)
    return dict(oc=oc, of=of, acc=acc, n=np.int64(n), X=X.view(np.uint64), err=err.view(np.uint32), keep=keep)


def _same_outputs(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_entry_points_repeat_and_interleave(ctx, orc):
    """sfmhip_find_2d3d, sfmhip_merge_new_points and sfmhip_triangulate allocate per call on one context and stream: two
    calls in a row give the same bytes, and so do calls interleaved with the other two entry points (run_mid_cases runs
    them one after the other; the second pass runs them in the opposite order)."""
    f, m, t = mid_cases()
    rc, rf = orc.find_2d3d(*f)
    racc, rn = orc.merge_new_points(*m)
    assert 0 < len(rc) < 5000 and 0 < rn < 2000               # a mid-sized case with both outcomes
    first = run_mid_cases(ctx)
    assert np.array_equal(first["oc"], rc) and np.array_equal(first["of"], rf) and np.array_equal(first["acc"], racc)
    _same_outputs(first, run_mid_cases(ctx))
    X, err, keep = triangulate.triangulate_points(*t, ctx=ctx)
    X2, err2, keep2 = triangulate.triangulate_points(*t, ctx=ctx)
    acc, n = incremental.merge_accept(*m, ctx=ctx)
    oc, of = incremental.find_2d3d(*f, ctx=ctx)
    oc2, of2 = incremental.find_2d3d(*f, ctx=ctx)
    acc2, n2 = incremental.merge_accept(*m, ctx=ctx)
    for got in (dict(oc=oc, of=of, acc=acc, n=np.int64(n), X=X.view(np.uint64), err=err.view(np.uint32), keep=keep),
                dict(oc=oc2, of=of2, acc=acc2, n=np.int64(n2), X=X2.view(np.uint64), err=err2.view(np.uint32), keep=keep2)):
        _same_outputs(first, got)


_POISON = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_incremental as T
np.savez(sys.argv[2], **T.run_mid_cases())
"""


def test_entry_points_on_poisoned_allocations(ctx, tmp_path):
    """SFMHIP_POISON=1 (csrc/common.h: fresh device memory holds 0xFF bytes) in a process of its own: `first` is memset,
    `near` is memset, `val`, `block_cnt`, `state` and triangulate's slab must be written before they are read (the tail
    of a last block included).  Every output equals the unpoisoned run's."""
    ref = run_mid_cases(ctx)
    script, out = tmp_path / "poison.py", tmp_path / "poison.npz"
    script.write_text(_POISON)
    subprocess.run([sys.executable, str(script), ROOT, str(out)], check=True, timeout=300, env=dict(os.environ, SFMHIP_POISON="1"))
    got = np.load(out)
    _same_outputs(ref, {k: got[k] for k in got.files})
