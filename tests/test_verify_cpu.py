"""Two-view verification of match lists (csrc/verify.h) on the CPU, through a g++ build of the header the device
code compiles (tests/stub/verify_capi.cpp): V4 / V5 against a numpy restatement on hand-made lists (order kept, count == inliers
for kept pairs, min_inliers at and one above the inlier count, the three `has` codes), V1 / V3 from a pair's E against the same
mask, the struct sizes, the V6 refusals that need no device -- and the point of the feature with the oracle alone: a match
graph with false edges, filtered by the oracle's RANSAC masks, loses fewer components to conflicts and keeps more tracks.  No
GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from sfm_danpipeline_amd.verify import VerifyOpts, VerifyStats
from tests.test_tracks_cpu import K_RING, i32, ring_scene, stub_build, tk, world_graph  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "verify_capi.cpp")
STAT_FIELDS = [f for f, _ in VerifyStats._fields_]


@pytest.fixture(scope="module")
def vf(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("verify") / "libverifycapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.vfy_default_opts.argtypes = [vp]
    lib.vfy_default_opts.restype = None
    lib.vfy_sizes.argtypes = [vp, vp]
    lib.vfy_check.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.vfy_compact_mask.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.vfy_compact_mask.restype = None
    lib.vfy_compact_E.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.vfy_compact_E.restype = None
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_verify.py)
def _p(a):
    return None if a is None else a.ctypes.data


def _outputs(counts, q):
    return np.full(counts.size, -7, np.int32), np.full(q.size + 1, -7, np.int32), np.full(q.size + 1, -7, np.int32), np.full(counts.size, 9, np.uint8)


def _result(st, oc, oq, ot, kept):
    n = int(st.matches_out)
    return dict(stats={f: getattr(st, f) for f in STAT_FIELDS}, counts=oc, q=oq[:n].copy(), t=ot[:n].copy(), kept=kept.astype(bool))


def stub_compact_mask(vf, counts, q, t, mask, has, inliers, min_inliers=15):
    """V4 + V5 from one mask byte per match"""
    counts, q, t, inliers = i32(counts), i32(q), i32(t), i32(inliers)
    mask, has = np.ascontiguousarray(mask, np.uint8), np.ascontiguousarray(has, np.uint8)
    oc, oq, ot, kept = _outputs(counts, q)
    st = VerifyStats()
    vf.vfy_compact_mask(counts.size, _p(counts), _p(q), _p(t), _p(mask), _p(has), _p(inliers), int(min_inliers), _p(oc), _p(oq), _p(ot), _p(kept),
                        C.byref(st))
    return _result(st, oc, oq, ot, kept)


def stub_compact_E(vf, pairs, counts, q, t, xy_ptr, xy, K, E, has, inliers, threshold=1.0, min_inliers=15):
    """V1 + V3 + V4 + V5 from each pair's E"""
    pairs, counts, q, t, inliers, xy_ptr = i32(pairs).reshape(-1), i32(counts), i32(q), i32(t), i32(inliers), i32(xy_ptr)
    xy, K = np.ascontiguousarray(xy, np.float64).reshape(-1), np.ascontiguousarray(K, np.float64).reshape(9)
    E, has = np.ascontiguousarray(E, np.float64).reshape(-1), np.ascontiguousarray(has, np.uint8)
    oc, oq, ot, kept = _outputs(counts, q)
    st = VerifyStats()
    vf.vfy_compact_E(counts.size, _p(pairs), _p(counts), _p(q), _p(t), _p(xy_ptr), _p(xy), _p(K), float(threshold), _p(E), _p(has), _p(inliers),
                     int(min_inliers), _p(oc), _p(oq), _p(ot), _p(kept), C.byref(st))
    return _result(st, oc, oq, ot, kept)


def stub_check(vf, n_feat, pairs, counts, q, t, xy_ptr, xy, K, prob=0.999):
    """0: accepted, 1: refused (V6).  xy_ptr, xy and K may be None."""
    n_feat, pairs, counts, q, t = i32(n_feat), i32(pairs).reshape(-1), i32(counts), i32(q), i32(t)
    xy_ptr = None if xy_ptr is None else i32(xy_ptr)
    xy = None if xy is None else np.ascontiguousarray(xy, np.float64).reshape(-1)
    K = None if K is None else np.ascontiguousarray(K, np.float64).reshape(9)
    o = VerifyOpts(prob, 1.0, 15, 0)
    return vf.vfy_check(n_feat.size, _p(n_feat), counts.size, _p(pairs), _p(counts), _p(q), _p(t), _p(xy_ptr), _p(xy), _p(K), C.byref(o))


def np_filter(counts, q, t, mask, has, inliers, min_inliers):
    """V4 + V5 in numpy: (counts, q, t, kept)"""
    counts, q, t, mask = np.asarray(counts), np.asarray(q), np.asarray(t), np.asarray(mask).astype(bool)
    kept = (np.asarray(has) != 0) & (np.asarray(inliers) >= min_inliers)
    sel = mask & np.repeat(kept, counts)
    pair_of = np.repeat(np.arange(counts.size), counts)
    return i32(np.bincount(pair_of[sel], minlength=counts.size)), i32(q[sel]), i32(t[sel]), kept


def gather(pairs, counts, q, t, xy_ptr, xy):
    """the left and right pixels of every match, per pair (V1's indexing on the host)"""
    xy, off = np.asarray(xy, np.float64).reshape(-1, 2), np.concatenate([[0], np.cumsum(counts)])
    return [(xy[xy_ptr[a] + q[off[p]:off[p + 1]]], xy[xy_ptr[b] + t[off[p]:off[p + 1]]]) for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2))]


# ---------------------------------------------------------------- V4, V5
def test_struct_sizes_and_defaults(vf):
    a, b = C.c_int(), C.c_int()
    vf.vfy_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(VerifyOpts), C.sizeof(VerifyStats)) == (24, 40)
    o = VerifyOpts(0, 0, 0, 9)
    vf.vfy_default_opts(C.byref(o))
    assert (o.prob, o.threshold, o.min_inliers, o.reserved) == (0.999, 1.0, 15, 0)


def hand_lists():
    """five pairs: a RANSAC model with 20 inliers of 30, exactly five matches (has 2), no model, an empty pair, a model with
    every match an inlier; q and t are distinct everywhere, so that a wrong order or a wrong source shows"""
    rng = np.random.default_rng(4)
    counts = np.array([30, 5, 12, 0, 17])
    has = np.array([1, 2, 0, 0, 1], np.uint8)
    n = int(counts.sum())
    q, t = rng.permutation(1000)[:n], 2000 + rng.permutation(1000)[:n]
    mask = np.zeros(n, np.uint8)
    mask[rng.permutation(30)[:20]] = 1
    mask[30:35] = 1
    mask[47:] = 1
    inliers = np.array([20, 5, 0, 0, 17])
    return counts, q, t, mask, has, inliers


@pytest.mark.parametrize("min_inliers", [0, 5, 6, 17, 18, 20, 21, 1000])
def test_compaction_against_numpy(vf, min_inliers):
    counts, q, t, mask, has, inliers = hand_lists()
    got = stub_compact_mask(vf, counts, q, t, mask, has, inliers, min_inliers)
    rc, rq, rt, rkept = np_filter(counts, q, t, mask, has, inliers, min_inliers)
    assert got["counts"].tolist() == rc.tolist() and got["q"].tolist() == rq.tolist() and got["t"].tolist() == rt.tolist()
    assert got["kept"].tolist() == rkept.tolist()
    # inliers == min_inliers is kept, one below is dropped; a pair without a model is never kept, even at min_inliers 0
    assert got["kept"].tolist() == [20 >= min_inliers, 5 >= min_inliers, False, False, 17 >= min_inliers]
    assert all(c == i for c, i, k in zip(got["counts"], inliers, got["kept"]) if k) and not got["counts"][~got["kept"]].any()
    assert got["stats"] == dict(pairs=5, pairs_kept=int(rkept.sum()), pairs_no_model=2, matches_in=64, matches_out=int(rc.sum()))


def test_order_is_the_input_order(vf):
    counts, q, t, mask, has, inliers = hand_lists()
    got = stub_compact_mask(vf, counts, q, t, mask, has, inliers, 0)
    first = np.flatnonzero(mask[:30])
    assert got["q"][:20].tolist() == q[first].tolist() and got["t"][:20].tolist() == t[first].tolist()
    assert got["q"][20:25].tolist() == q[30:35].tolist() and got["q"][25:].tolist() == q[47:].tolist()


def test_mask_from_E_equals_the_masked_compaction(vf):
    """E = [t]x of a sideways translation: a match is an inlier when its pixels share a row.  has 2 keeps all five matches
    whatever E says; has 0 keeps none."""
    nf = 40
    rng = np.random.default_rng(8)
    xy_ptr = np.array([3, 3 + nf, 3 + nf, 3 + 2 * nf + 5])           # slack before, an empty image, slack after
    xy = rng.uniform(0, 600, (int(xy_ptr[-1]), 2))
    off_row = rng.random(nf) < 0.4
    xy[xy_ptr[2]:xy_ptr[2] + nf, 1] = xy[xy_ptr[0]:xy_ptr[0] + nf, 1] + 30.0 * off_row
    pairs, counts = [(0, 2), (2, 0), (0, 2)], np.array([nf, 5, 9])
    f = np.concatenate([rng.permutation(nf), rng.permutation(nf)[:5], rng.permutation(nf)[:9]])
    E = np.tile(np.array([0, 0, 0, 0, 0, -1, 0, 1, 0.0]), 3)
    has = np.array([1, 2, 0], np.uint8)
    mask = np.concatenate([~off_row[f[:nf]], np.ones(5, bool), np.zeros(9, bool)])
    inliers = np.array([int(mask[:nf].sum()), 5, 0])
    assert 5 < inliers[0] < nf
    got = stub_compact_E(vf, pairs, counts, f, f, xy_ptr, xy, K_RING, E, has, inliers, min_inliers=0)
    want = stub_compact_mask(vf, counts, f, f, mask, has, inliers, 0)
    assert got["stats"] == want["stats"] and all(got[k].tolist() == want[k].tolist() for k in ("counts", "q", "t", "kept"))
    assert got["counts"].tolist() == inliers.tolist()


def test_empty_inputs(vf):
    e = np.zeros(0, np.int32)
    got = stub_compact_mask(vf, e, e, e, e, e, e)
    assert got["stats"] == dict(pairs=0, pairs_kept=0, pairs_no_model=0, matches_in=0, matches_out=0)
    got = stub_compact_mask(vf, [0, 0], e, e, e, [0, 0], [0, 0])
    assert got["counts"].tolist() == [0, 0] and not got["kept"].any() and got["stats"]["pairs_no_model"] == 2
    assert stub_check(vf, [3, 3], e, e, e, e, [0, 3, 6], None, K_RING) == 0          # no match: xy may be missing
    assert stub_check(vf, [3, 3], [(0, 1)], [0], e, e, [0, 3, 6], None, K_RING) == 0


# ---------------------------------------------------------------- V6
XY6 = np.zeros((6, 2))
REFUSALS = [("q at n_feat", dict(q=[3])), ("t at n_feat", dict(t=[3])), ("negative q", dict(q=[-1])), ("negative t", dict(t=[-1])),
            ("self pair", dict(pairs=[(1, 1)])), ("image past the end", dict(pairs=[(0, 2)])), ("negative image", dict(pairs=[(-1, 1)])),
            ("negative count", dict(counts=[-1])), ("decreasing xy_ptr", dict(xy_ptr=[0, 4, 3])), ("negative xy_ptr", dict(xy_ptr=[-1, 3, 6])),
            ("an image with fewer pixels than features", dict(xy_ptr=[0, 2, 6])), ("prob 0", dict(prob=0.0)), ("prob 1", dict(prob=1.0)),
            ("prob NaN", dict(prob=float("nan"))), ("no K", dict(K=None)), ("no xy_ptr", dict(xy_ptr=None)), ("no xy with a match", dict(xy=None))]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_v6_refusals(vf, case):
    base = dict(n_feat=[3, 3], pairs=[(0, 1)], counts=[1], q=[0], t=[0], xy_ptr=[0, 3, 6], xy=XY6, K=K_RING, prob=0.999)
    assert stub_check(vf, **base) == 0
    assert stub_check(vf, **dict(base, **case[1])) == 1


# ---------------------------------------------------------------- the point of the feature, with the oracle alone
N_IMAGES, N_FEAT, N_WORLD, SEED, P_FALSE = 8, 200, 260, 7, 0.05
MIXED_CAP = 0.01


def false_edge_scene(seed=SEED, p_false=P_FALSE, n_images=N_IMAGES, n_feat=N_FEAT, n_world=N_WORLD, noise=0.3):
    """world_graph's lists over ring_scene's geometry: image i's feature feat_of[i, w] has the pixel of world point w in view
    i; a feature that shows no world point has a pixel drawn over the same window.  Returns (n_feat, pairs, counts, q, t,
    feat_of, xy_ptr, xy [n_images * n_feat, 2], world_of [n_images, n_feat] with -1 for no point)."""
    nf, pairs, counts, q, t, feat_of = world_graph(seed, n_images, n_feat, n_world, p_false=p_false)
    _, _, _, ring_xy, _ = ring_scene(seed, n_images, n_world, noise=noise)
    ring_xy = ring_xy.reshape(n_images, n_world, 2)
    rng = np.random.default_rng(seed + 1000)
    xy = rng.uniform(ring_xy.min(axis=(0, 1)), ring_xy.max(axis=(0, 1)), (n_images, n_feat, 2))
    world_of = np.full((n_images, n_feat), -1, np.int64)
    for i in range(n_images):
        w = np.flatnonzero(feat_of[i] >= 0)
        xy[i, feat_of[i, w]] = ring_xy[i, w]
        world_of[i, feat_of[i, w]] = w
    return nf, pairs, counts, q, t, feat_of, i32(np.arange(n_images + 1) * n_feat), xy.reshape(-1, 2), world_of


def mixed_tracks(ptr, view, feat, world_of):
    """the tracks whose nodes do not all show one world point"""
    w = world_of[view, feat]
    return sum(1 for k in range(ptr.size - 1) if (w[ptr[k]:ptr[k + 1]] < 0).any() or np.unique(w[ptr[k]:ptr[k + 1]]).size != 1)


def test_verified_lists_lose_fewer_tracks_to_false_matches(vf, tk):
    """Seed 7, p_false 0.05, 8 images x 200 features, 260 world points, 28 pairs: 1 827 matches of which 72 are false.  The
    raw lists give 46 conflicting components and 167 tracks, 2 of them mixing world points.  Filtered by the oracle's masks under
    V4 / V5 (the defaults: 0.999, 1 px, min_inliers 15) every pair is kept, 1 749 matches stay, none of them false: no
    conflicting component, 257 tracks, none mixed.  What is asserted are conditions on this input and on the oracle, not
    tolerances on the device: strictly fewer conflicting components, strictly more tracks, and at most MIXED_CAP = 1 % of the
    verified tracks mixing world points (a false match survives only when its pixel falls within the threshold of the epipolar
    line: about 2 px x 300 px of a 300 px x 300 px window, 0.7 % of the false matches, so far fewer than 1 % of the tracks)."""
    nf, pairs, counts, q, t, feat_of, xy_ptr, xy, world_of = false_edge_scene()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pts = gather(pairs, counts, q, t, xy_ptr, xy)
    left, right = np.concatenate([a for a, _ in pts]), np.concatenate([b for _, b in pts])
    inl, its, mask, flags = orc.score_essential_many(off, left, right, K_RING, want_mask=True)
    assert flags == 0
    has = np.where(inl > 0, np.where(counts == 5, 2, 1), 0)
    got = stub_compact_mask(vf, counts, q, t, mask, has, inl)
    assert got["counts"][got["kept"]].tolist() == inl[got["kept"]].tolist()
    rc, raw, rptr, rview, rfeat, _ = stub_build(tk, nf, pairs, counts, q, t)
    vc, ver, vptr, vview, vfeat, _ = stub_build(tk, nf, pairs, got["counts"], got["q"], got["t"])
    assert rc == 0 and vc == 0
    pa, pb = np.repeat(pairs[:, 0], counts), np.repeat(pairs[:, 1], counts)
    false_in = int((world_of[pa, q] != world_of[pb, t]).sum())
    va, vb = np.repeat(pairs[:, 0], got["counts"]), np.repeat(pairs[:, 1], got["counts"])
    false_out = int((world_of[va, got["q"]] != world_of[vb, got["t"]]).sum())
    raw_mixed, ver_mixed = mixed_tracks(rptr, rview, rfeat, world_of), mixed_tracks(vptr, vview, vfeat, world_of)
    print(f"MEASURE verify oracle: matches {int(counts.sum())} -> {got['stats']['matches_out']}, false {false_in} -> {false_out}, pairs kept "
          f"{got['stats']['pairs_kept']} of {len(counts)}; conflicting {raw['conflicting']} -> {ver['conflicting']}, tracks {raw['n_tracks']} -> "
          f"{ver['n_tracks']}, mixed tracks {raw_mixed} -> {ver_mixed}")
    assert false_in > 50 and raw["conflicting"] > 20                       # the input is dirty enough to show it
    assert ver["conflicting"] < raw["conflicting"] and ver["n_tracks"] > raw["n_tracks"]
    assert ver_mixed <= MIXED_CAP * ver["n_tracks"]
