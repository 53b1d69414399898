"""GPU: two-view verification of match lists (csrc/verify.hip) against the composition of parts that are already
pinned -- the lists as fetched, a host gather of the pixels, scoring.score_essential with masks (E from pose.essential_pose,
which runs the same RANSAC), and the CPU stub of V4 / V5 (tests/stub/verify_capi.cpp) -- byte for byte: counts, packed q / t,
inliers, iterations, kept, and E as u64 bits.  The shapes are the edges of the wave, the 256-thread block and the list slot
(0, 4, 5, 6, 63, 64, 65, 255, 256, 257, 513 matches, the longest pair filling its slot), a pair without outliers, a pair of
noise, the same pair twice, an image without features, slack in xy_ptr, every pair alone against its batch, the lists of a
real match plan read on the device, the refusals and the empty sets, and the options off their defaults with fx != fy."""
import ctypes as C

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, matcher, pose, scoring, synth, tracks, verify
from tests import score_scenes as Z
from tests.test_tracks_cpu import K_RING, i32, ring_scene, tk  # noqa: F401
from tests.test_verify_cpu import gather, stub_compact_E, stub_compact_mask, vf  # noqa: F401

pytestmark = pytest.mark.gpu

K = Z.K
COUNTS = (0, 4, 5, 6, 63, 64, 65, 255, 256, 257, 513)


def two_view_lists(scenes, seed=0, slack=False, empty_at=None):
    """Pair p of `scenes` (left pixels, right pixels) becomes two images of its own, 2p and 2p + 1 (one more before `empty_at`:
    an image without features), whose features are the pair's pixels in a shuffled order, and a list that names them match by
    match.  slack: one to three NaN pixels after every image, which xy_ptr skips.  Returns dict(n_feat, pairs, counts, q, t,
    xy_ptr, xy)."""
    rng, pad_rng = np.random.default_rng(seed), np.random.default_rng(seed + 1)   # (the lists do not depend on the layout)
    n_feat, rows, xy_ptr, pairs, counts, q, t = [], [], [0], [], [], [], []

    def add_image(pix):
        n_feat.append(len(pix))
        rows.append(np.asarray(pix, np.float64).reshape(-1, 2))
        pad = int(pad_rng.integers(1, 4)) if slack else 0
        rows.append(np.full((pad, 2), np.nan))
        xy_ptr.append(xy_ptr[-1] + len(pix) + pad)
        return len(n_feat) - 1

    for a, b in scenes:
        ids, idx = [], []
        for pix in (a, b):
            if empty_at is not None and len(n_feat) == empty_at:
                add_image(np.zeros((0, 2)))
            perm = rng.permutation(len(pix))
            img = np.empty((len(pix), 2))
            img[perm] = pix                                          # match i's pixel is feature perm[i]
            ids.append(add_image(img)), idx.append(perm)
        pairs.append(ids), counts.append(len(a)), q.append(idx[0]), t.append(idx[1])
    return dict(n_feat=i32(n_feat), pairs=i32(pairs).reshape(-1, 2), counts=i32(counts), q=i32(np.concatenate(q)), t=i32(np.concatenate(t)),
                xy_ptr=i32(xy_ptr), xy=np.concatenate(rows))


def reference(ctx, vf, L, K, prob=0.999, threshold=1.0, min_inliers=15):
    """the composition: host gather -> score_essential with masks (+ essential_pose's E) -> the stub's V4 / V5"""
    pts = gather(L["pairs"], L["counts"], L["q"], L["t"], L["xy_ptr"], L["xy"])
    inl, masks, its = scoring.score_essential(pts, K, prob, threshold, want_mask=True, ctx=ctx)
    flags = scoring.last_flags(ctx)
    E = np.zeros((len(pts), 3, 3))                                    # (zero where there is no model, as d_bestE starts)
    ran = np.flatnonzero(L["counts"] >= 5)
    if ran.size:
        E[ran] = pose.essential_pose([pts[p] for p in ran], K, prob, threshold, ctx=ctx)["E"]
    has = np.where(inl > 0, np.where(L["counts"] == 5, 2, 1), 0).astype(np.uint8)
    mask = np.concatenate(masks) if len(pts) else np.zeros(0, np.uint8)
    ref = stub_compact_mask(vf, L["counts"], L["q"], L["t"], mask, has, inl, min_inliers)
    # the stub's own V1 / V3 from E gives the same lists as the device's mask
    from_E = stub_compact_E(vf, L["pairs"], L["counts"], L["q"], L["t"], L["xy_ptr"], L["xy"], K, E, has, inl, threshold, min_inliers)
    assert all(from_E[k].tobytes() == ref[k].tobytes() for k in ("counts", "q", "t", "kept")) and from_E["stats"] == ref["stats"]
    ref.update(inliers=inl.copy(), iterations=its.copy(), E=E, flags=flags, has=has)
    return ref


def assert_same(h, ref):
    got = h.download()
    assert {f: getattr(h.stats, f) for f, _ in verify.VerifyStats._fields_} == ref["stats"]
    for k in ("counts", "q", "t", "inliers", "iterations"):
        assert got[k].dtype == np.int32 and got[k].tobytes() == i32(ref[k]).tobytes(), k
    assert got["kept"].tolist() == ref["kept"].tolist()
    assert got["E"].reshape(-1).view(np.uint64).tolist() == np.ascontiguousarray(ref["E"]).reshape(-1).view(np.uint64).tolist()
    # V5: the output count of a kept pair is the RANSAC's own count; every other pair keeps nothing
    assert got["counts"][got["kept"]].tolist() == got["inliers"][got["kept"]].tolist() and not got["counts"][~got["kept"]].any()
    return got


def check_lists(ctx, vf, L, K=K, **opts):
    ref = reference(ctx, vf, L, K, **opts)
    h = verify.verify_lists(ctx, L["n_feat"], L["pairs"], L["counts"], L["q"], L["t"], L["xy_ptr"], L["xy"], K, **opts)
    assert scoring.last_flags(ctx) == ref["flags"]
    got = assert_same(h, ref)
    h.close()
    return got, ref


def count_scenes():
    """one pair per count of COUNTS: the first matches of a 600-match scene with a fifth of outliers (the five-match pair from a
    scene without any, so that its one sample gives a model)"""
    return [(a[:c], b[:c]) for c, (a, b) in ((c, Z.scene(600, 900 + c, outliers=0.0 if c == 5 else 0.2)) for c in COUNTS)]


# ---------------------------------------------------------------- the shapes
@pytest.mark.parametrize("min_inliers", [15, 0])
def test_match_counts_at_the_wave_block_and_slot_edges(ctx, vf, min_inliers):
    L = two_view_lists(count_scenes(), seed=1)
    assert L["counts"].tolist() == list(COUNTS)                       # host lists: the slot is the longest pair's count, 513
    got, ref = check_lists(ctx, vf, L, min_inliers=min_inliers)
    assert not got["kept"][:2].any() and (got["inliers"][:2] == 0).all() and (got["iterations"][:2] == 0).all()  # 0 and 4 matches: no RANSAC
    assert ref["has"][2] == 2 and got["inliers"][2] == 5 and got["kept"][2] == (min_inliers <= 5)
    assert got["kept"][4:].all() and (got["counts"][4:] < L["counts"][4:]).all()     # the outliers are gone, not the pair
    if min_inliers == 0:
        assert got["counts"][2] == 5


def test_special_pairs_layouts_and_batch_independence(ctx, vf):
    rng = np.random.default_rng(5)
    clean = Z.scene(300, 31, outliers=0.0, noise=0.0)               # exact pixels: every match is an inlier of the true E
    noise = (rng.uniform(0, 600, (100, 2)), rng.uniform(0, 500, (100, 2)))
    scenes = [clean, noise, Z.scene(257, 44, outliers=0.4), Z.scene(400, 41, outliers=0.45), Z.scene(64, 45, outliers=0.1)]
    plain = two_view_lists(scenes, seed=2)
    got, ref = check_lists(ctx, vf, plain)
    assert got["kept"].tolist() == [True, False, True, True, True]
    assert got["counts"][0] == 300 and got["counts"][1] == 0 and got["inliers"][1] < 15
    # an image without features in the middle and slack in xy_ptr: the same lists, other image numbers and pixel offsets
    moved = two_view_lists(scenes, seed=2, slack=True, empty_at=3)
    assert moved["n_feat"][3] == 0 and np.isnan(moved["xy"]).any() and moved["q"].tolist() == plain["q"].tolist()
    got2, _ = check_lists(ctx, vf, moved)
    assert all(got2[k].tobytes() == got[k].tobytes() for k in ("counts", "q", "t", "inliers", "iterations", "E"))
    # the same pair twice in one batch, and the batch reversed
    twice = dict(plain, pairs=np.concatenate([plain["pairs"], plain["pairs"][2:3]]), counts=np.concatenate([plain["counts"], plain["counts"][2:3]]))
    o = int(plain["counts"][:2].sum())
    twice["q"], twice["t"] = (np.concatenate([plain[k], plain[k][o:o + 257]]) for k in ("q", "t"))
    got3, _ = check_lists(ctx, vf, twice)
    o3 = int(got3["counts"][:2].sum())
    assert got3["counts"][5] == got3["counts"][2] and got3["q"][-got3["counts"][5]:].tolist() == got3["q"][o3:o3 + got3["counts"][2]].tolist()
    assert got3["E"][5].tobytes() == got3["E"][2].tobytes() and got3["iterations"][5] == got3["iterations"][2]
    # every pair alone gives what it gives inside the batch
    off, ooff = np.concatenate([[0], np.cumsum(plain["counts"])]), np.concatenate([[0], np.cumsum(got["counts"])])
    for p in range(len(scenes)):
        one = dict(plain, pairs=plain["pairs"][p:p + 1], counts=plain["counts"][p:p + 1], q=plain["q"][off[p]:off[p + 1]], t=plain["t"][off[p]:off[p + 1]])
        h = verify.verify_lists(ctx, one["n_feat"], one["pairs"], one["counts"], one["q"], one["t"], one["xy_ptr"], one["xy"], K)
        d = h.download()
        h.close()
        assert (d["counts"][0], d["inliers"][0], d["iterations"][0], d["kept"][0]) == (got["counts"][p], got["inliers"][p], got["iterations"][p], got["kept"][p])
        assert d["q"].tolist() == got["q"][ooff[p]:ooff[p + 1]].tolist() and d["t"].tolist() == got["t"][ooff[p]:ooff[p + 1]].tolist()
        assert d["E"][0].tobytes() == got["E"][p].tobytes()


# ---------------------------------------------------------------- a real plan
def plan_scene(n_images=6, n_feat=300, bank=450, seed=3, displaced=0.1):
    """synth.sift_image_set's descriptors with pixels: a feature shows the world point of its bank row (found again as the
    nearest row of the regenerated bank) in a ring of cameras; a seeded tenth of the features is displaced by 20 to 60 px."""
    imgs = synth.sift_image_set(n_images, n_feat, 128, bank=bank, seed=seed)
    W = np.random.default_rng(seed).integers(0, 256, size=(bank, 128), dtype=np.int16).astype(np.float32)
    _, _, _, ring_xy, _ = ring_scene(seed, n_images, bank, noise=0.3)
    ring_xy = ring_xy.reshape(n_images, bank, 2)
    rng = np.random.default_rng(seed + 50)
    xy = np.zeros((n_images, n_feat, 2))
    for i, d in enumerate(imgs):
        row = np.argmin((d * d).sum(1)[:, None] - 2 * d @ W.T + (W * W).sum(1)[None, :], axis=1)
        assert np.unique(row).size == n_feat
        xy[i] = ring_xy[i, row]
        bad = rng.random(n_feat) < displaced
        xy[i, bad] += rng.uniform(20, 60, (int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
    return imgs, i32(np.arange(n_images + 1) * n_feat), xy.reshape(-1, 2)


def test_verify_plan_equals_verify_lists_equals_the_composition(ctx, vf):
    imgs, xy_ptr, xy = plan_scene()
    pairs = synth.all_pairs(6)
    s = matcher.ImageSet(imgs, ctx=ctx)
    s.prepare_async()
    pl = matcher.MatchPlan(s, pairs)
    pl.run_async(0.8)
    counts, q, t, _ = pl.fetch()
    assert counts.sum() > 500
    nf = i32([len(im) for im in imgs])
    L = dict(n_feat=nf, pairs=pairs, counts=counts, q=q, t=t, xy_ptr=xy_ptr, xy=xy)
    ref = reference(ctx, vf, L, K_RING)
    a = verify.verify_plan(pl, xy_ptr, xy, K_RING)
    assert scoring.last_flags(ctx) == ref["flags"]
    got = assert_same(a, ref)
    b = verify.verify_lists(ctx, nf, pairs, counts, q, t, xy_ptr, xy, K_RING)
    assert_same(b, ref)
    assert got["kept"].all() and 0 < a.stats.matches_out < a.stats.matches_in    # the displaced pixels are gone
    tm = a.last_timing()
    assert tm["total"] > 0 and abs(tm["gather"] + tm["ransac"] + tm["compact"] - tm["total"]) <= 1e-9 + 1e-6 * tm["total"]
    # the tracks of the verified set, read on the device, are the tracks of its downloaded lists
    for h in (a, b):
        for min_len in (2, 3):
            x = tracks.build_from_verified(h, min_len=min_len)
            y = tracks.build(ctx, nf, pairs, got["counts"], got["q"], got["t"], min_len=min_len)
            assert all(getattr(x.stats, f) == getattr(y.stats, f) for f, _ in tracks.TracksStats._fields_) and x.stats.n_tracks > 50
            assert all(u.tobytes() == v.tobytes() for u, v in zip(x.download(), y.download()))
            x.close(), y.close()
    raw = tracks.build_from_plan(pl)
    ver = tracks.build_from_verified(a)
    print(f"MEASURE verify plan: matches {a.stats.matches_in} -> {a.stats.matches_out}; conflicting {raw.stats.conflicting} -> "
          f"{ver.stats.conflicting}, tracks {raw.stats.n_tracks} -> {ver.stats.n_tracks}")
    raw.close(), ver.close()
    # the plan's own lists are as they were
    c2, q2, t2, _ = pl.fetch()
    assert c2.tobytes() == counts.tobytes() and q2.tobytes() == q.tobytes() and t2.tobytes() == t.tobytes()
    a.close(), b.close(), pl.close(), s.close()


# ---------------------------------------------------------------- V6 and the options
def raw_verify_lists(ctx, L, K=K, prob=0.999):
    """the C entry itself: (status, *out afterwards) with *out preset to a marker; an entry of L, or K, may be None"""
    A = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in L.items()}   # (the arrays outlive the call)
    A["K"] = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
    p = lambda k: None if A[k] is None else A[k].ctypes.data
    o, h = verify.default_opts(prob=prob), C.c_void_p(0x5a5a)
    rc = _lib.lib().sfmhip_verify_lists(ctx.h, len(A["n_feat"]), p("n_feat"), len(A["counts"]), p("pairs"), p("counts"), p("q"), p("t"),
                                        p("xy_ptr"), p("xy"), p("K"), C.byref(o), C.byref(h))
    return rc, h.value


def small_lists():
    return two_view_lists([Z.scene(40, 71), Z.scene(30, 72)], seed=3)


def _set(key, index, value):
    return lambda L: L[key].__setitem__(index, value)


# (name, a change to the lists, keyword arguments of the call)
REFUSALS = [("q at n_feat", _set("q", 7, 40), {}), ("negative t", _set("t", 45, -1), {}), ("the last match of the last pair", _set("t", 69, 30), {}),
            ("self pair", _set("pairs", (1, 1), 2), {}), ("image past the end", _set("pairs", (0, 1), 4), {}),
            ("negative image", _set("pairs", (0, 0), -1), {}), ("negative count", _set("counts", 1, -1), {}),
            ("decreasing xy_ptr", _set("xy_ptr", 2, 39), {}), ("negative xy_ptr", _set("xy_ptr", 0, -1), {}),
            ("an image with fewer pixels than features", _set("xy_ptr", slice(3, None), [109, 139]), {}),
            ("prob 0", None, dict(prob=0.0)), ("prob 1", None, dict(prob=1.0)), ("no K", None, dict(K=None)),
            ("no xy_ptr", lambda L: L.update(xy_ptr=None), {}), ("no xy with a match", lambda L: L.update(xy=None), {})]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_v6_refusals_leave_out_unwritten(ctx, case):
    L = {k: v.copy() for k, v in small_lists().items()}
    assert L["counts"].tolist() == [40, 30] and L["xy_ptr"].tolist() == [0, 40, 80, 110, 140]
    if case[1]:
        case[1](L)
    rc, out = raw_verify_lists(ctx, L, **case[2])
    assert rc == -3 and out == 0x5a5a


def test_refusals_of_a_plan_and_the_unharmed_call(ctx):
    L = small_lists()
    rc, out = raw_verify_lists(ctx, L)                                 # the lists themselves are fine
    assert rc == 0 and out not in (0, 0x5a5a)
    _lib.lib().sfmhip_verified_destroy(C.c_void_p(out))
    imgs = synth.sift_image_set(3, 60, 128, bank=80, seed=5)
    s = matcher.ImageSet(imgs, ctx=ctx)
    s.prepare_async()
    pl = matcher.MatchPlan(s, synth.all_pairs(3))
    pl.run_async(0.8)
    xy_ptr, xy = i32([0, 60, 120, 180]), np.random.default_rng(1).uniform(0, 600, (180, 2))
    with pytest.raises(_lib.SfmHipError):
        verify.verify_plan(pl, i32([0, 60, 119, 180]), xy, K)         # image 1 has 60 features and 59 pixels
    with pytest.raises(_lib.SfmHipError):
        verify.verify_plan(pl, xy_ptr, xy, K, prob=1.5)
    with pytest.raises(_lib.SfmHipError):
        verify.verify_plan(pl, xy_ptr, xy, None)
    h = verify.verify_plan(pl, xy_ptr, xy, K)                         # random pixels: matches, but no pair with 15 inliers
    assert h.stats.pairs == 3 and h.stats.matches_in > 0 and h.stats.matches_out == 0 and h.stats.pairs_kept == 0
    h.close(), pl.close(), s.close()


def test_empty_sets(ctx, vf):
    e = np.zeros(0, np.int32)
    L = small_lists()
    few = lambda a: np.concatenate([a[:4], a[40:43]])
    for pairs, counts, q, t in ((e, e, e, e), (L["pairs"], [0, 0], e, e), (L["pairs"], [4, 3], few(L["q"]), few(L["t"]))):
        M = dict(L, pairs=i32(pairs).reshape(-1, 2), counts=i32(counts), q=i32(q), t=i32(t))
        got, _ = check_lists(ctx, vf, M)
        assert not got["kept"].any() and not got["counts"].any() and got["q"].size == 0 and not got["E"].any()
        assert not got["inliers"].any() and not got["iterations"].any()
        h = verify.verify_lists(ctx, M["n_feat"], M["pairs"], M["counts"], M["q"], M["t"], M["xy_ptr"], M["xy"], K)
        tr = tracks.build_from_verified(h)
        assert tr.stats.n_tracks == 0 and tr.stats.edges == 0 and tr.stats.nodes == 140
        tr.close(), h.close()
    # no match anywhere: xy may be missing
    h = verify.verify_lists(ctx, L["n_feat"], L["pairs"], [0, 0], e, e, L["xy_ptr"], None, K)
    assert h.stats.matches_out == 0 and h.stats.pairs == 2
    h.close()
    h = verify.verify_lists(ctx, e, e, e, e, e, [0], None, K)          # no image at all
    assert h.stats.pairs == 0 and h.download()["counts"].size == 0
    h.close()


def test_min_inliers_and_options_off_their_defaults(ctx, vf):
    L = two_view_lists([Z.scene(120, 81, outliers=0.3), Z.scene(200, 82, outliers=0.5), Z.scene(20, 83, outliers=0.0)], seed=4)
    got0, _ = check_lists(ctx, vf, L, min_inliers=0)
    assert got0["kept"].all()
    top = int(got0["inliers"].max())
    got1, _ = check_lists(ctx, vf, L, min_inliers=top)                # the threshold itself is kept
    assert got1["kept"].tolist() == (got0["inliers"] == top).tolist()
    got2, _ = check_lists(ctx, vf, L, min_inliers=top + 1)            # above every count
    assert not got2["kept"].any() and got2["inliers"].tolist() == got0["inliers"].tolist() and got2["E"].tobytes() == got0["E"].tobytes()
    # fx != fy, prob and threshold off their defaults: the figures of tests/score_scenes.py's tables
    for Kc, (prob, thr), (inl, its) in ((Z.K_TALL, *Z.OPTIONS_TALL[5]), (Z.K_WIDE, *Z.OPTIONS_WIDE[2]), (Z.K_TALL, *Z.OPTIONS_TALL[3])):
        M = two_view_lists([Z.options_scene(Kc), Z.scene(65, 84, K=Kc)], seed=6, slack=True)
        got, _ = check_lists(ctx, vf, M, K=Kc, prob=prob, threshold=thr)
        assert (got["inliers"][0], got["iterations"][0]) == (inl, its) and got["counts"][0] == inl
