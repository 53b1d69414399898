"""GPU: every kernel instantiation of the matcher against the oracle, bit for bit -- not only the 128-wide one.

csrc/match.hip picks its kernel from the descriptor width (pick_ks):

    L2       dim <= 32      knn_kernel<1,0,2,256>        two query tiles per wave, 256-row stages
    L2       33 .. 64       knn_kernel<2,0,2,256>
    L2       65 .. 128      knn_kernel<4,0,2,256>        (tests/test_gpu_match.py lives here)
    L2       129 .. 256     knn_kernel<8,0,1,128>        ONE query tile per wave, 128-row stages, BATCH 2, LPR 8
    L2       > 256          knn_exact_kernel, force_all  no MFMA
    Hamming  <= 32 bytes    knn_keyed_kernel<8,128>      nbits = 8 * dim, zero-padded bit columns
    Hamming  > 32 bytes     knn_exact_kernel, force_all

Every comparison is _assert_pair's: both k-NN indices, the distance bits and the ratio-filtered lists equal
orc.match_knn2's.  No tolerances.

Route x case, as (nq, nt, dim or bytes, dtype); "both" is u8 and integer-valued f32:

    route          more than one stage and work item      ties                              merge range                       epoch / key-chunk boundary
    KS=1           (226,225) (33,482) (64,738) x 17|32    (300,700,32) two values + ovf,    unreachable; the range of h at    (130,8193,32,u8) (98,16500,32,u8)
                   both                                   4 cluster seeds at 32, both       (300,700,32) both
    KS=2           the same x 61|64 both                  the same at 61, both              unreachable; (300,700,64) both    (130,8193,61,u8) (98,16500,61,u8)
    KS=4           the same x 65 both (lower edge)        tests/test_gpu_match.py           tests/test_gpu_match.py           tests/test_gpu_match.py
    KS=8           (98,97) (33,226) (64,354) x            (300,700,250|256) two values +    (300,700,129|200|250|256) S=3,    (130,8193,256,u8) (98,16500,256,u8)
                   129|250|256 both                       ovf, 4 cluster seeds, both        (100,700,256) S=8, 4 x            (130,8193,250,f32) (98,16500,250,f32)
                                                                                            (300,700,256) S=1, both           and both lengths on the 0/255 rows at 256 u8
    L2 > 256       (5,300) (300,5) x 257|300 both,        (300,700,300) two values, both    no flag on this route             no epochs on this route
                   (200,300,300,f32) random, ragged 300
    Hamming keyed  (256,128) (257,129) (64,385) x         0x00/0xFF rows with copies        --                                (130,8193,16) (98,16500,16): chunks of 1024
                   1|8|16|31|32 bytes
    Hamming exact  (5,300) (300,5) x 33|61|64 bytes,      --                                --                                --
                   ragged 61                              (300,700,61) 0x00/0xFF twinned

f32 rows off the MFMA route: (200,200) x 61|250 with one image + 0.25, the values 300, -1, 256 at 61, and random
non-integer (200,300) at 61|250|300.  Ragged plans [130, 513, 2, 0, 1] x all 20 pairs: 32 u8, 256 f32, 300 u8, Hamming 16
and 61 bytes.

What the tests were held against (the breaks were built apart and are not in the tree): emitting from the h_p == 1 lanes at
NU == 1 changes no bit -- both half-waves hold the same merged result -- and nothing can catch it; staging the C inputs of
even 128-row stages only fails test_edges_l2_ks8 from two stages on and 38 more KS=8 cases; nbits = 256 in the Hamming
prepare fails every test_edges_hamming_keyed below 32 bytes; dropping the tail loop of exact_dist<KIND_F32_L2> fails
test_random_non_integer_rows and every f32 case of the exact route at dim % 8 != 0."""
import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, matcher, synth
from tests.test_gpu_match import _assert_pair, _plan

pytestmark = pytest.mark.gpu

U8, F32 = np.uint8, np.float32
DTYPES = [pytest.param(U8, id="u8"), pytest.param(F32, id="f32")]


def _onorm(orc, norm):
    return orc.NORM_HAMMING if norm == _lib.HAMMING else orc.NORM_L2


def _knn(orc, q, t, norm=_lib.L2):
    r = orc.match_knn2(q, t, norm=_onorm(orc, norm), want_knn=True, threads=8)
    return r[3], r[4]


def _check_pair(ctx, orc, q, t, norm=_lib.L2):
    s, pl = _plan(ctx, [q, t], [[0, 1]], norm)
    _assert_pair(orc, pl, 0, q, t, norm)
    return pl


def _tied(orc, q, t, norm=_lib.L2):
    """share of the queries whose best two distances are equal, from the oracle's lists alone"""
    ki, kd = _knn(orc, q, t, norm)
    return float(np.mean((ki[:, 1] >= 0) & (kd[:, 0] == kd[:, 1])))


# ---------------------------------------------------------------- a. stage, work-item and tiny edges
# Positions are n + 31 (L2: the odd class is padded to a tile) or n (Hamming).  A work item holds 256 query positions
# (NU = 2, keyed kernel) or 128 (KS = 8); a stage 256 train positions (KS = 1, 2, 4) or 128 (KS = 8, keyed kernel).
# The sizes sit on and one past those edges: 1, 2 and 3 stages, 1 and 2 work items.
NU2_SHAPES = [(1, 1), (1, 2), (2, 1), (225, 226), (226, 225), (33, 482), (64, 738)]
KS8_SHAPES = [(1, 1), (1, 2), (2, 1), (97, 98), (98, 97), (33, 226), (64, 354)]
KEYED_SHAPES = [(1, 1), (1, 2), (256, 128), (257, 129), (64, 385)]
EXACT_SHAPES = [(1, 1), (1, 2), (5, 300), (300, 5)]


def _edge_case(ctx, orc, q, t, norm):
    pl = _check_pair(ctx, orc, q, t, norm)
    ki, kd = pl.fetch_knn(0)
    if len(t) == 1:                                        # one neighbour, no match
        assert np.all(ki[:, 0] == 0) and np.all(ki[:, 1] == -1) and pl.counts()[0] == 0
    else:                                                  # from two train rows on the list is complete
        assert np.all(ki >= 0) and np.all(ki[:, 0] != ki[:, 1])


def _sift_rows(nq, nt, dim, cast, seed):
    n = max(nq, nt)
    imgs = synth.sift_image_set(2, n, dim, bank=n + 200, seed=seed)
    return imgs[0][:nq].astype(cast), imgs[1][:nt].astype(cast)


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("nq,nt", NU2_SHAPES)
@pytest.mark.parametrize("dim", [17, 32, 61, 64, 65])
def test_edges_l2_two_query_tiles_per_wave(ctx, orc, dim, nq, nt, cast):
    q, t = _sift_rows(nq, nt, dim, cast, seed=dim * 1000 + nq * 7 + nt)
    _edge_case(ctx, orc, q, t, _lib.L2)


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("nq,nt", KS8_SHAPES)
@pytest.mark.parametrize("dim", [129, 250, 256])
def test_edges_l2_ks8(ctx, orc, dim, nq, nt, cast):
    q, t = _sift_rows(nq, nt, dim, cast, seed=dim * 1000 + nq * 7 + nt)
    _edge_case(ctx, orc, q, t, _lib.L2)


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("nq,nt", EXACT_SHAPES)
@pytest.mark.parametrize("dim", [257, 300])
def test_edges_l2_without_mfma(ctx, orc, dim, nq, nt, cast):
    q, t = _sift_rows(nq, nt, dim, cast, seed=dim * 1000 + nq * 7 + nt)
    _edge_case(ctx, orc, q, t, _lib.L2)


def _orb_rows(nq, nt, nbytes, seed):
    n = max(nq, nt)
    imgs = synth.orb_image_set(2, n, nbytes=nbytes, bank=n + 200, seed=seed)
    return imgs[0][:nq].copy(), imgs[1][:nt].copy()


@pytest.mark.parametrize("nq,nt", KEYED_SHAPES)
@pytest.mark.parametrize("nbytes", [1, 8, 16, 31, 32])
def test_edges_hamming_keyed(ctx, orc, nbytes, nq, nt):
    q, t = _orb_rows(nq, nt, nbytes, seed=nbytes * 1000 + nq * 7 + nt)
    _edge_case(ctx, orc, q, t, _lib.HAMMING)


@pytest.mark.parametrize("nq,nt", EXACT_SHAPES)
@pytest.mark.parametrize("nbytes", [33, 61, 64])
def test_edges_hamming_without_mfma(ctx, orc, nbytes, nq, nt):
    q, t = _orb_rows(nq, nt, nbytes, seed=nbytes * 1000 + nq * 7 + nt)
    _edge_case(ctx, orc, q, t, _lib.HAMMING)


# ---------------------------------------------------------------- b. ties
TIE_DIMS = [32, 61, 250, 256]


def _positions(t):
    """Where the prepare pass puts the rows of an L2 image: the rows with an odd element sum first, padded to a 32-row
    tile, then the even ones, original order inside each class"""
    odd = (t.astype(np.int64).sum(1) & 1).astype(bool)
    pos = np.empty(len(t), np.int64)
    pos[odd] = np.arange(odd.sum())
    pos[~odd] = (odd.sum() + 31) // 32 * 32 + np.arange((~odd).sum())
    return pos, odd


def _overflow_queries(q, t):
    """Per epoch of 8192 train positions, how many queries MUST take the many-equal-slots overflow of knn_kernel's resolve
    (ovf: the query is redone exactly), worked out from the rows alone.  A lane (query, half h) sees the train positions
    whose bit 2 is h, one accumulator slot per position mod 32, and resolves the rows of two slots; when the query's largest
    h of the epoch is held by three slots of one lane, all three reach its threshold.  Equal h is equal (squared distance
    + odd class).

    This and _positions mirror csrc/match.hip -- the parity order of the prepare pass, the rows 8g + 4h + j of a lane's
    accumulator slots, `ns > 2` in phase A of the resolve, EPOCH_TILES -- and prove only that the recipe reaches the case;
    no comparison uses them.  A change of that layout has to change them with it, or they assert another kernel's condition."""
    pos, odd = _positions(t)
    qf, tf = q.astype(np.float64), t.astype(np.float64)    # (integers below 2^53: exact)
    d = (qf * qf).sum(1)[:, None] + (tf * tf).sum(1)[None, :] - 2.0 * (qf @ tf.T) + odd[None, :]
    out = []
    for ep in range(int(pos.max()) // 8192 + 1):
        here = pos // 8192 == ep
        best = d[:, here].min(1)                           # (the query's best of the epoch: no other lane's tile tops it)
        n = np.zeros(len(q), bool)
        for h in (0, 1):
            lane = here & ((pos >> 2 & 1) == h)
            slot = pos[lane] & 31
            for i in range(len(q)):
                n[i] |= len(np.unique(slot[d[i, lane] == best[i]])) >= 3
        out.append(int(n.sum()))
    return out


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("dim", TIE_DIMS)
def test_heavy_ties_two_values(ctx, orc, dim, cast):
    """test_heavy_ties_across_tiles_and_chunks' one-level case at the other widths: rows of 0 and 60 only, every train row
    twinned half an image later.  Some queries overflow the two resolved slots at every width (KS = 1 and KS = 8 differ
    in BATCH, LPR and STEPS, not in the tagged keys)."""
    rng = np.random.default_rng(1)
    q = (rng.integers(0, 2, (300, dim)) * 60).astype(cast)
    t = (rng.integers(0, 2, (700, dim)) * 60).astype(cast)
    t[350:] = t[:350]
    assert _tied(orc, q, t) >= 0.10
    assert _overflow_queries(q, t)[0] > 0
    _check_pair(ctx, orc, q, t)


@pytest.mark.parametrize("cast", DTYPES)
def test_heavy_ties_l2_without_mfma(ctx, orc, cast):
    """the same rows at dim 300: knn_exact_kernel's insertion and wave merge by (distance, lower train index)"""
    rng = np.random.default_rng(1)
    q = (rng.integers(0, 2, (300, 300)) * 60).astype(cast)
    t = (rng.integers(0, 2, (700, 300)) * 60).astype(cast)
    t[350:] = t[:350]
    assert _tied(orc, q, t) >= 0.10
    _check_pair(ctx, orc, q, t)


def test_heavy_ties_hamming_without_mfma(ctx, orc):
    """61 bytes of 0x00 / 0xFF, every train row twinned: the exact route's ties under Hamming"""
    rng = np.random.default_rng(1)
    q = rng.integers(0, 2, (300, 61)).astype(U8) * 255
    t = rng.integers(0, 2, (700, 61)).astype(U8) * 255
    t[350:] = t[:350]
    assert _tied(orc, q, t, _lib.HAMMING) >= 0.10
    _check_pair(ctx, orc, q, t, _lib.HAMMING)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("dim", TIE_DIMS)
def test_ties_at_the_second_best_value(ctx, orc, dim, seed):
    """test_ties_at_the_second_best_value_inside_a_lane's recipe at the other widths: cluster centres, small steps, exact
    copies one row, one tile and several tiles away, before and behind the best row."""
    rng = np.random.default_rng(1000 + seed)
    nt = int(rng.integers(96, 900))
    nq = int(rng.integers(40, 260))
    centres = rng.integers(0, 256, (max(nt // 6, 4), dim))
    t = centres[rng.integers(0, len(centres), nt)].copy()
    for _ in range(3):
        d_ = rng.integers(0, dim, nt)
        t[np.arange(nt), d_] = np.clip(t[np.arange(nt), d_] + rng.integers(-2, 3, nt), 0, 255)
    for off in (1, 2, 31, 32, 33, 64, 97, 160):
        src = rng.integers(0, nt, nt // 10)
        dst = np.clip(src + rng.choice([-off, off], len(src)), 0, nt - 1)
        t[dst] = t[src]
    q = t[rng.integers(0, nt, nq)].copy()
    dq = rng.integers(0, dim, nq)
    q[np.arange(nq), dq] = np.clip(q[np.arange(nq), dq] + rng.integers(-1, 2, nq), 0, 255)
    for cast in (F32, U8):
        assert _tied(orc, q.astype(cast), t.astype(cast)) >= 0.10
        _check_pair(ctx, orc, q.astype(cast), t.astype(cast))


# ---------------------------------------------------------------- c. extremes and the merge range
def _extreme_rows(nq, nt, dim, cast, seed=77):
    """mostly-0 queries against mostly-255 train rows: h = q.t - ceil(|t|^2 / 2) near its minimum (-6 226 048 at dim 256
    for an all-0 query and an all-255 row, 74 % of the HPAD budget), squared distances far in the sqrtf merge range.  The
    all-0 rows go into q only and the all-255 rows into t only: the extreme h without a near match."""
    rng = np.random.default_rng(seed)
    q = ((rng.random((nq, dim)) < 0.1) * 255).astype(cast)
    t = ((rng.random((nt, dim)) < 0.9) * 255).astype(cast)
    q[0] = q[nq // 2] = 0
    t[0] = t[nt * 10 // 21] = t[nt - 1] = 255
    return q, t


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("dim", [129, 200, 250, 256])
def test_extremes_in_the_merge_range_ks8(ctx, orc, dim, cast):
    q, t = _extreme_rows(300, 700, dim, cast)
    assert not q[0].any() and not q[150].any() and t[0].min() == t[333].min() == t[699].min() == 255
    ki, kd = _knn(orc, q, t)
    assert np.all(kd[:, 1] >= 2048.0)                      # every query flagged: 300 listed, knn_fixup_kernel with S = 3
    _check_pair(ctx, orc, q, t)


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("dim", [32, 64])
def test_extremes_below_the_merge_range(ctx, orc, dim, cast):
    """64 * 255^2 < 2^22: the flag cannot fire at KS <= 2; what is tested is the range of h"""
    q, t = _extreme_rows(300, 700, dim, cast)
    ki, kd = _knn(orc, q, t)
    assert np.all(kd[:, 1] < 2048.0)
    _check_pair(ctx, orc, q, t)


@pytest.mark.parametrize("cast", DTYPES)
@pytest.mark.parametrize("n_pairs,nq", [(1, 100), (4, 300)])
def test_fixup_workgroup_split_at_256(ctx, orc, n_pairs, nq, cast):
    """knn_fixup_kernel shares a flagged query among S = clamp(FIX_GRID / nfix, 1, 8) workgroups, FIX_GRID = 1024:
    100 flagged queries take S = 8, 4 pairs x 300 = 1200 take S = 1 (300 in one pair, S = 3, is the test above)."""
    qs = [_extreme_rows(nq, 700, 256, cast, seed=77 + i)[0] for i in range(n_pairs)]
    t = _extreme_rows(nq, 700, 256, cast)[1]
    imgs = qs + [t]
    pairs = [[i, n_pairs] for i in range(n_pairs)]
    s, pl = _plan(ctx, imgs, pairs)
    for p in range(n_pairs):
        assert np.all(_knn(orc, qs[p], t)[1][:, 1] >= 2048.0)
        _assert_pair(orc, pl, p, qs[p], t, _lib.L2)


# ---------------------------------------------------------------- d. epochs
EPOCH_SHAPES = [(130, 8193), (98, 16500)]


def _plant_across_epochs(q, t, seed):
    """test_train_images_longer_than_an_epoch with dup=True: copies of early rows behind the epoch boundary, half of the
    queries exact hits (some of rows that have copies)"""
    rng = np.random.default_rng(seed)
    nq, nt = len(q), len(t)
    src = rng.integers(0, 8000, 400)
    t[8192 + rng.integers(0, nt - 8192, 400)] = t[src]
    q[: nq // 2] = t[rng.integers(0, nt, nq // 2)]


def _epochs_of(ki, t):
    """the epoch (8192 train positions) of each listed neighbour"""
    return _positions(t)[0][ki] // 8192


@pytest.mark.parametrize("nq,nt", EPOCH_SHAPES)
@pytest.mark.parametrize("dim,cast", [(32, U8), (61, U8), (256, U8), (250, F32)])
def test_epochs_at_other_widths(ctx, orc, dim, cast, nq, nt):
    imgs = synth.sift_image_set(2, nt, dim, bank=nt + 500, seed=nq + nt + dim)
    q, t = imgs[0][:nq].copy(), imgs[1][:nt].copy()
    _plant_across_epochs(q, t, nt)
    pos, odd = _positions(t)
    first, last = int(np.nonzero(~odd)[0][0]), int(np.argmax(pos))
    q[0] = t[last] = t[first]                              # a tie across the first and the last epoch (same class: positions stay)
    q, t = q.astype(cast), t.astype(cast)
    ki, kd = _knn(orc, q, t)
    ep = _epochs_of(ki, t)
    assert ep[0, 0] < ep[0, 1] == pos.max() // 8192 and kd[0, 0] == kd[0, 1] == 0
    _check_pair(ctx, orc, q, t)


@pytest.mark.parametrize("nq,nt", EPOCH_SHAPES)
def test_epochs_in_the_merge_range_at_256(ctx, orc, nq, nt):
    """the 0/255 rows over two and three epochs.  The first half of the queries has both neighbours in the sqrtf merge
    range; the second half are exact hits, some with a copy in a later epoch; the last query's row stands eight times in
    a row in the first epoch -- four equal slots in each half: it overflows there and is carried, flagged, through the
    epochs behind."""
    q, t = _extreme_rows(nq, nt, 256, U8)
    rng = np.random.default_rng(nt)
    t[8192 + rng.integers(0, nt - 8192, 400)] = t[rng.integers(1, 8000, 400)]
    t[8191] = t[8192] = 255
    t[100:108] = t[100]
    q[nq // 2 + 1:] = t[rng.integers(1, nt, nq - nq // 2 - 1)]
    q[nq - 1] = t[100]
    assert not q[0].any() and not q[nq // 2].any() and t[0].min() == 255
    ki, kd = _knn(orc, q, t)
    assert np.all(kd[:nq // 2 + 1, 1] >= 2048.0) and np.any(kd[:, 1] < 2048.0)
    ovf = _overflow_queries(q, t)
    assert len(ovf) >= 2 and any(n > 0 for n in ovf[:-1])  # (in the first epoch, or the second when row 100 is an even one)
    _check_pair(ctx, orc, q, t)


@pytest.mark.parametrize("nq,nt", EPOCH_SHAPES)
def test_hamming_16_bytes_across_the_key_chunks(ctx, orc, nq, nt):
    """test_hamming_ties_across_the_key_chunks' recipe at nbits = 128 and beyond 8192 rows"""
    rng = np.random.default_rng(nt)
    orb = rng.integers(0, 2, (nt, 16)).astype(U8) * 255
    for off in (1, 32, 1023, 1024, 1025, 2048):
        src = rng.integers(0, nt - off, nt // 8)
        orb[src + off] = orb[src]
    qb = orb[rng.integers(0, nt, nq)].copy()
    flip = rng.integers(0, 16, nq)
    qb[np.arange(nq), flip] ^= rng.choice(np.array([0, 1, 3, 255], U8), nq)
    assert _tied(orc, qb, orb, _lib.HAMMING) >= 0.10
    _check_pair(ctx, orc, qb, orb, _lib.HAMMING)


# ---------------------------------------------------------------- e. f32 rows that leave the MFMA route
@pytest.mark.parametrize("dim", [61, 250])
def test_non_integer_image_poisons_only_its_pairs(ctx, orc, dim):
    """dim % 8 = 5 and 2: the tail of exact_dist's eight interleaved sums; the clean pair stays on the MFMA route"""
    imgs = synth.sift_image_set(3, 200, dim, bank=300, seed=5)
    mixed = [imgs[0] + 0.25, imgs[1], imgs[2]]
    pairs = [(0, 1), (1, 2), (2, 0)]
    s, pl = _plan(ctx, mixed, pairs)
    for p, (a, b) in enumerate(pairs):
        _assert_pair(orc, pl, p, mixed[a], mixed[b], _lib.L2)


@pytest.mark.parametrize("value", [300.0, -1.0, 256.0])
def test_integer_rows_outside_the_range_at_61(ctx, orc, value):
    imgs = synth.sift_image_set(3, 200, 61, bank=300, seed=6)
    bad = imgs[1].copy()
    bad[17, 5] = value
    bad[150, :] = value
    mixed = [imgs[0], bad, imgs[2]]
    pairs = [(0, 1), (1, 2), (2, 0), (1, 0)]
    s, pl = _plan(ctx, mixed, pairs)
    for p, (a, b) in enumerate(pairs):
        _assert_pair(orc, pl, p, mixed[a], mixed[b], _lib.L2)


@pytest.mark.parametrize("dim", [61, 250, 300])
def test_random_non_integer_rows(ctx, orc, dim):
    """every sum rounds: the bits agree only if the summation order is the oracle's l2_f32, tail included"""
    rng = np.random.default_rng(dim)
    q = (rng.random((200, dim)) * 255).astype(F32)
    t = (rng.random((300, dim)) * 255).astype(F32)
    _check_pair(ctx, orc, q, t)


# ---------------------------------------------------------------- f. plans over ragged sets
RAGGED = [130, 513, 2, 0, 1]
RAGGED_PAIRS = np.array([[a, b] for a in range(5) for b in range(5) if a != b], np.int32)


def _ragged_set(norm, width, cast):
    if norm == _lib.HAMMING:
        imgs = synth.orb_image_set(5, 513, nbytes=width, bank=700, seed=31 + width)
    else:
        imgs = [a.astype(cast) for a in synth.sift_image_set(5, 513, width, bank=700, seed=31 + width)]
    return [np.ascontiguousarray(a[:n]) for a, n in zip(imgs, RAGGED)]


@pytest.mark.parametrize("norm,width,cast", [
    pytest.param(_lib.L2, 32, U8, id="l2-32-u8"), pytest.param(_lib.L2, 256, F32, id="l2-256-f32"),
    pytest.param(_lib.L2, 300, U8, id="l2-300-u8"), pytest.param(_lib.HAMMING, 16, U8, id="hamming-16"),
    pytest.param(_lib.HAMMING, 61, U8, id="hamming-61")])
def test_ragged_plan_retarget_and_drop_in(ctx, orc, norm, width, cast):
    imgs = _ragged_set(norm, width, cast)
    pairs = RAGGED_PAIRS
    s, pl = _plan(ctx, imgs, pairs, norm)
    cnt, oq, ot, od = pl.fetch()
    ocnt, ocs = orc.match_many_checksum(imgs, pairs, norm=_onorm(orc, norm), threads=8)
    assert np.array_equal(cnt, ocnt)
    assert np.array_equal(orc.pair_checksums(cnt, oq, ot, od), ocs)
    assert cnt[0] > 20                                     # (the 130 x 513 pair shares bank rows)
    for p, (a, b) in enumerate(pairs):
        if RAGGED[b] < 2:
            assert cnt[p] == 0                             # an empty or one-row train image matches nothing
    for a, b in ((0, 1), (1, 0), (1, 2)):
        p = int(np.nonzero((pairs[:, 0] == a) & (pairs[:, 1] == b))[0][0])
        _assert_pair(orc, pl, p, imgs[a], imgs[b], norm)
    # a one-pair plan pointed at every pair in turn
    off = np.concatenate([[0], np.cumsum(cnt)])
    one = matcher.MatchPlan(s, pairs[:1])
    for p in np.random.default_rng(0).permutation(len(pairs)):
        one.set_pairs(pairs[p:p + 1])
        one.run_async(0.8)
        c1, q1, t1, d1 = one.fetch()
        assert c1[0] == cnt[p]
        assert np.array_equal(q1, oq[off[p]:off[p + 1]]) and np.array_equal(t1, ot[off[p]:off[p + 1]])
        assert np.array_equal(d1.view(np.uint32), od[off[p]:off[p + 1]].view(np.uint32))
    # the getMatching drop-in (sfmhip_match_knn2)
    mq, mt, md = matcher.get_matching(imgs[0], imgs[1], norm=norm, ctx=ctx)
    r = orc.match_knn2(imgs[0], imgs[1], norm=_onorm(orc, norm))
    assert np.array_equal(mq, r[0]) and np.array_equal(mt, r[1])
    assert np.array_equal(md.view(np.uint32), r[2].view(np.uint32))


# ---------------------------------------------------------------- g. the order in which set and plan go away
def test_closing_the_set_before_its_plan(ctx):
    """A failing comparison leaves set and plan in the traceback's reference cycle, and the collector finalises a cycle in
    any order: sfmhip_matchplan_destroy must not read the set (it did, for the device number, and a failing test took the
    interpreter down with it).  The plan's own buffers are all it frees."""
    q, t = _sift_rows(40, 50, 32, U8, seed=3)
    s, pl = _plan(ctx, [q, t], [[0, 1]])
    want = [a.copy() for a in pl.fetch()]
    s.close()
    pl.close()
    s2, pl2 = _plan(ctx, [q, t], [[0, 1]])                 # the device is as usable as before
    assert all(np.array_equal(a, b) for a, b in zip(pl2.fetch(), want))
