"""GPU: the SIFT front end (reference src/Sfm.cpp:300-330) -- sfmhip_sift_detect_and_compute,
its _device variant and sfmhip_sift_batch against the numpy restatement of OpenCV 3.4.1's SIFT (oracle/sfm_oracle_sift.py;
PARITY UNPINNED: OpenCV is not in the image, see that file's header).  The device follows the restatement's order of
operations stage by stage, so every comparison is bit for bit: the six keypoint fields as int32 patterns, the descriptors
with array_equal.  The cases off the defaults and their images are tests/sift_images.py's; what those cases must exercise
is asserted on the restatement alone in tests/test_oracle_sift.py."""
import numpy as np
import pytest

from oracle import sfm_oracle_sift as S
from sfm_danpipeline_amd import features
from tests import sift_images as I

pytestmark = pytest.mark.gpu


def _blobs(h, w, n, seed, noise=2.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w))
    for _ in range(n):
        cx, cy, s, a = rng.uniform(8, w - 8), rng.uniform(8, h - 8), rng.uniform(1.2, 6), rng.uniform(40, 200)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(img + rng.normal(0, noise, (h, w)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape,seed", [((96, 128), 0), ((75, 101), 1), ((160, 120), 2)])
def test_keypoints_and_descriptors_match_the_restatement(ctx, shape, seed):
    img = _blobs(shape[0], shape[1], 30, seed)
    K, D = features.sift_detect_and_compute(img, ctx=ctx)
    Ko, Do = S.detect_and_compute(img)
    assert len(Ko) > 20
    assert K.shape == Ko.shape and D.shape == Do.shape, (K.shape, Ko.shape)
    # the same bit patterns: coordinates, size, angle, response, the octave / layer / xi word, and every descriptor entry (the
    # device follows the restatement's order of operations stage by stage; round 4 measured 8428 keypoints of the temple
    # frames identical in all six fields and 1 078 784 descriptor entries without one difference)
    assert np.array_equal(K.view(np.int32), Ko.astype(np.float32).view(np.int32))
    assert np.array_equal(D, Do.astype(np.float32))
    n = np.linalg.norm(D, axis=1)
    assert np.all((n > 480) & (n < 540)) and D.min() >= 0 and D.max() <= 255 and np.array_equal(D, np.rint(D))


def test_flat_and_tiny_images(ctx):
    K, D = features.sift_detect_and_compute(np.full((64, 64), 90, np.uint8), ctx=ctx)
    assert len(K) == 0 and D.shape == (0, 128)
    img = _blobs(24, 20, 3, 5)
    K, D = features.sift_detect_and_compute(img, ctx=ctx)
    Ko, Do = S.detect_and_compute(img)
    assert len(Ko) >= 1
    assert K.shape == Ko.shape and np.array_equal(K.view(np.int32), Ko.astype(np.float32).view(np.int32))
    assert D.shape == Do.shape and np.array_equal(D, Do.astype(np.float32))


def test_descriptors_feed_the_matcher(ctx):
    """two views of the same blobs (a shift): SIFT -> getMatching finds the shift"""
    from sfm_danpipeline_amd import matcher
    big = _blobs(140, 180, 60, 9, noise=1.0)
    a, b = big[10:130, 10:170], big[14:134, 18:178]                 # b(x, y) = a(x + 8, y + 4)
    Ka, Da = features.sift_detect_and_compute(a, ctx=ctx)
    Kb, Db = features.sift_detect_and_compute(b, ctx=ctx)
    q, t, d = matcher.get_matching(Da, Db, ratio=0.8, ctx=ctx)
    assert len(q) >= 15
    shift = Ka[q, :2] - Kb[t, :2]
    good = (np.abs(shift[:, 0] - 8) < 1.0) & (np.abs(shift[:, 1] - 4) < 1.0)
    assert good.mean() > 0.8


def test_cpp_host_mirror_extracts_the_same_features(ctx, tmp_path):
    """imagesLOAD + extractFeature of the C++ mirror (reference src/Sfm.cpp:118-198, 257-330) on PNG files: its gray
    images through the Python binding give the very same keypoints and descriptors, imagesPts2D = the keypoints' pt."""
    import struct
    import subprocess
    PIL = pytest.importorskip("PIL.Image")
    from sfm_danpipeline_amd import build
    d = tmp_path / "imgs"
    d.mkdir()
    for i in range(2):
        g = _blobs(120, 160, 40, 40 + i)
        PIL.fromarray(np.stack([g, g, g], 2)).save(d / ("v%d.png" % i))
    exe = build.build_io_demo()
    r = subprocess.run([exe, "--features", str(d), str(tmp_path / "f.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(tmp_path / "f.bin", "rb").read()
    n = struct.unpack_from("<i", raw, 0)[0]
    pos = 4
    assert n == 2
    for i in range(n):
        rows, cols = struct.unpack_from("<ii", raw, pos); pos += 8
        gray = np.frombuffer(raw, np.uint8, rows * cols, pos).reshape(rows, cols); pos += rows * cols
        nk = struct.unpack_from("<i", raw, pos)[0]; pos += 4
        K = np.frombuffer(raw, np.float32, 6 * nk, pos).reshape(nk, 6); pos += 24 * nk
        D = np.frombuffer(raw, np.float32, 128 * nk, pos).reshape(nk, 128); pos += 512 * nk
        P = np.frombuffer(raw, np.float64, 2 * nk, pos).reshape(nk, 2); pos += 16 * nk
        Kp, Dp = features.sift_detect_and_compute(gray, ctx=ctx)
        assert nk > 20 and np.array_equal(K.view(np.int32), Kp.view(np.int32)) and np.array_equal(D, Dp)
        assert np.array_equal(P, K[:, :2].astype(np.float64))


def _render_views(n_views=3, n_blobs=220, seed=17, h=240, w=320):
    """a cloud of blobs seen by cameras on an arc (pinhole, f = 400): the image of a blob is a Gaussian at its
    projection, its size falling with depth"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2.2, 2.2, n_blobs), rng.uniform(-1.6, 1.6, n_blobs), rng.uniform(5, 9, n_blobs)], 1)
    rad, amp = rng.uniform(0.02, 0.07, n_blobs), rng.uniform(50, 180, n_blobs)
    K = np.array([[400.0, 0, w / 2], [0, 400.0, h / 2], [0, 0, 1]])
    yy, xx = np.mgrid[0:h, 0:w]
    views, poses = [], []
    for v in range(n_views):
        a = 0.06 * (v - (n_views - 1) / 2)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([-0.5 * (v - (n_views - 1) / 2), 0.0, 0.0])
        Xc = X @ R.T + t
        uv = Xc[:, :2] / Xc[:, 2:] * 400.0 + [w / 2, h / 2]
        img = np.full((h, w), 20.0)
        for (u, vv), z, r, am in zip(uv, Xc[:, 2], rad, amp):
            s = 400.0 * r / z
            if -10 < u < w + 10 and -10 < vv < h + 10:
                y0, y1, x0, x1 = int(max(vv - 5 * s, 0)), int(min(vv + 5 * s + 1, h)), int(max(u - 5 * s, 0)), int(min(u + 5 * s + 1, w))
                img[y0:y1, x0:x1] += am * np.exp(-((xx[y0:y1, x0:x1] - u) ** 2 + (yy[y0:y1, x0:x1] - vv) ** 2) / (2 * s * s))
        views.append(np.clip(img + rng.normal(0, 1.0, (h, w)), 0, 255).astype(np.uint8))
        poses.append(np.hstack([R, t[:, None]]))
    return views, poses, K


def test_cfg1_shaped_pipeline_on_rendered_views(ctx):
    """the call order of BASELINE.json's cfg1 (SIFT -> all-pairs getMatching -> findBestPair's E-matrix score) through
    the Python bindings on rendered views of one scene (look-alike blobs: few inliers, RANSAC runs its full 1000
    iterations -- the hard regime for the scoring); cfg1 itself, the temple frames, is tests/test_gpu_cfg1.py"""
    from sfm_danpipeline_amd import matcher, scoring
    views, poses, K = _render_views()
    feats = [features.sift_detect_and_compute(v, ctx=ctx) for v in views]
    assert all(len(k) > 120 for k, _ in feats)
    iset = matcher.ImageSet([d for _, d in feats], ctx=ctx)
    pairs = [(0, 1), (0, 2), (1, 2)]
    plan = matcher.MatchPlan(iset, np.array(pairs, np.int32))
    iset.prepare_async()
    plan.run_async(0.8)
    cnt, q, t, d = plan.fetch()
    off = np.concatenate([[0], np.cumsum(cnt)])
    pts = []
    for p, (a, b) in enumerate(pairs):
        qa, tb = q[off[p]:off[p + 1]], t[off[p]:off[p + 1]]
        pts.append((features.keypoints_to_points(feats[a][0])[qa], features.keypoints_to_points(feats[b][0])[tb]))
    # (Gaussian blobs all look alike: the ratio test keeps ~60 of ~200 per pair, below the reference's cut of 120 at
    # :533, which real texture passes -- the cut is a parameter of the mirror)
    assert all(len(a) >= 40 for a, _ in pts), [len(a) for a, _ in pts]
    best = scoring.find_best_pair(pairs, pts, K, min_matches=40, ctx=ctx)
    assert len(best) >= 1 and all(0.3 < float(r) <= 1.0 for r, _ in best)        # a third and more of the matches obey one
    assert [float(r) for r, _ in best] == sorted(float(r) for r, _ in best)      # epipolar geometry to 1 px (look-alike blobs)
    from oracle import sfm_oracle_score as SC
    want = SC.find_best_pair_scores([(pairs[i], pts[i][0], pts[i][1]) for i in range(3)], K, min_matches=40)
    assert [(float(r), v) for r, v in best] == [(float(r), v) for r, v in want]


def test_batched_front_end_leaves_the_same_descriptors_in_hbm(ctx):
    """sfmhip_sift_batch (several images in flight on worker streams, descriptor rows left in HBM) against the one-image
    entry, image by image and bit for bit; the matcher adopts the device rows in place and finds the same matches as
    from uploaded host rows"""
    from sfm_danpipeline_amd import matcher
    big = _blobs(150, 200, 70, 21, noise=1.0)
    imgs = [big[10:130, 10:170], big[14:134, 18:178], _blobs(96, 128, 30, 3), np.full((40, 40), 7, np.uint8), _blobs(75, 101, 30, 4),
            big[0:120, 0:160], _blobs(64, 64, 12, 6), _blobs(160, 120, 30, 2), big[20:140, 30:190], _blobs(50, 70, 9, 8), _blobs(88, 99, 25, 9)]
    single = [features.sift_detect_and_compute(g, ctx=ctx) for g in imgs]
    for rep in range(2):                                            # (the second call reuses the worker contexts)
        batch = features.sift_batch(imgs, ctx=ctx)
        assert len(batch) == len(imgs)
        for i, ((K1, D1), (K2, dd)) in enumerate(zip(single, batch)):
            assert np.array_equal(K1.view(np.int32), K2.view(np.int32)), i
            assert dd.n == len(K1) and np.array_equal(D1, dd.download()), i
    assert len(single[3][0]) == 0 and batch[3][1].ptr in (None, 0)     # the flat image: no keypoints, no device rows
    use = [0, 1, 5, 8]
    a = matcher.ImageSet([single[i][1] for i in use], ctx=ctx)          # uploaded host rows
    b = matcher.ImageSet(n_rows=[batch[i][1].n for i in use], dim=128, dtype=matcher.F32, norm=matcher.L2, ctx=ctx)
    for j, i in enumerate(use):
        b.adopt_device(j, batch[i][1].ptr, keepalive=batch[i][1])
    pairs = np.array([[0, 1], [0, 2], [1, 3], [2, 3]], np.int32)
    res = []
    for s_ in (a, b):
        s_.prepare_async()
        pl = matcher.MatchPlan(s_, pairs)
        pl.run_async(0.8)
        res.append(pl.fetch())
    assert all(np.array_equal(x, y) for x, y in zip(*res)) and res[0][0].sum() > 30


# ---------------------------------------------------------------- the cases of tests/sift_images.py: widths past one block, layers,
# sigma, thresholds, windows off the image, degenerate sizes -- bit for bit against the restatement
def _assert_same(K, D, Ko, Do):
    assert K.dtype == np.float32 and D.dtype == np.float32
    assert K.shape == Ko.shape and D.shape == Do.shape, (K.shape, Ko.shape, D.shape, Do.shape)
    assert np.array_equal(K.view(np.int32), np.ascontiguousarray(Ko, np.float32).view(np.int32))       # all six fields
    assert np.array_equal(D, Do)


def _detect(img, p, ctx, **kw):
    return features.sift_detect_and_compute(img, p["n_layers"], p["contrast_thr"], p["edge_thr"], p["sigma"], ctx=ctx, **kw)


@pytest.mark.parametrize("name", list(I.CASES))
def test_case_matches_the_restatement(ctx, name):
    Ko, Do = I.reference(name)
    I.check_case(name)                                               # (on the restatement's answer: the case is not empty)
    K, D = _detect(I.image(name), I.params(name), ctx)
    _assert_same(K, D, Ko, Do)


@pytest.mark.parametrize("shape", I.DEGENERATE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_degenerate_geometry(ctx, shape):
    """octaves no higher or wider than twice the border, the clamp of the octave count, reflect-101 under a kernel
    wider than the image: the one-image entry and the batch against the restatement"""
    img = I.degenerate_image(shape)
    Ko, Do = I.degenerate_reference(shape)
    K, D = features.sift_detect_and_compute(img, ctx=ctx)
    _assert_same(K, D, Ko, Do)
    (Kb, dd), = features.sift_batch([img], ctx=ctx)
    _assert_same(Kb, dd.download(), Ko, Do)
    assert dd.n == len(Ko)
    if len(Ko) == 0:
        assert K.shape == (0, 6) and D.shape == (0, 128) and Kb.shape == (0, 6) and dd.ptr in (None, 0)
    else:
        assert dd.ptr not in (None, 0)


def test_batch_with_parameters(ctx):
    """one sfmhip_sift_batch call away from the defaults (5 layers, sigma 1.2) over textured, saturated, coarse, tiny and
    empty images: image by image the one-image entry at the same parameters; one of them against the restatement"""
    p = dict(I.DEFAULTS, n_layers=5, sigma=1.2)
    imgs = [I.image("texture_129"), I.degenerate_image((2, 2)), I.image("checker_132"), I.degenerate_image((11, 40)),
            np.full((40, 40), 7, np.uint8), I.image("corner_blob"), I.degenerate_image((2, 300)), I.image("blocks_150"),
            I.degenerate_image((200, 6)), I.degenerate_image((6, 200)), I.degenerate_image((5, 5))]
    single = [_detect(g, p, ctx) for g in imgs]
    batch = features.sift_batch(imgs, p["n_layers"], p["contrast_thr"], p["edge_thr"], p["sigma"], ctx=ctx)
    assert len(batch) == len(imgs)
    for i, ((K1, D1), (K2, dd)) in enumerate(zip(single, batch)):
        assert np.array_equal(K1.view(np.int32), K2.view(np.int32)) and K2.shape == K1.shape, i
        assert dd.n == len(K1) and np.array_equal(D1, dd.download()), i
        assert (dd.ptr in (None, 0)) == (len(K1) == 0), i
    assert [len(single[i][0]) for i in (1, 4, 6)] == [0, 0, 0] and sum(len(k) > 20 for k, _ in single) >= 3
    Ko, Do = I.degenerate_reference((11, 40), n_layers=5, sigma=1.2)
    assert len(Ko) >= 1
    _assert_same(batch[3][0], batch[3][1].download(), Ko, Do)


# ---------------------------------------------------------------- capacity and refusals through the C ABI
ERR_ARG = -3
_SENT = np.float32(-77.0)


class _Raw:
    """the two one-image entry points behind one call: run(gray, capacity, ...) -> (status, count, keypoints array,
    descriptors array or None, the device pointer the _device variant left).  The arrays are sentinel-filled; the host
    variant's descriptors come back in its array, the _device variant's are downloaded and freed."""

    def __init__(self, ctx, device):
        from sfm_danpipeline_amd import _lib
        self.ctx, self.device, self.L = ctx, device, _lib.lib()

    def run(self, g, capacity, room=None, p=I.DEFAULTS, rows=None, cols=None, null=()):
        """room: rows of the arrays handed over (default: capacity); null: arguments passed as NULL"""
        import ctypes as C
        room = max(capacity if room is None else room, 1)
        k, d = np.full((room, 6), _SENT, np.float32), np.full((room, 128), _SENT, np.float32)
        n, dptr = C.c_int32(-5), C.c_void_p(0xDEAD0)
        head = (self.ctx.h, None if "gray" in null else g.ctypes.data, g.shape[0] if rows is None else rows,
                g.shape[1] if cols is None else cols, int(p["n_layers"]), float(p["contrast_thr"]), float(p["edge_thr"]),
                float(p["sigma"]), capacity, None if "keypoints" in null else k.ctypes.data)
        np_ = None if "n_keypoints" in null else C.addressof(n)
        if self.device:
            rc = self.L.sfmhip_sift_detect_and_compute_device(*head, None if "descriptors" in null else C.pointer(dptr), np_)
            if rc == 0 and dptr.value and n.value > 0:
                assert self.L.sfmhip_device_download(self.ctx.h, d.ctypes.data, dptr, 512 * n.value) == 0
            if rc == 0 and dptr.value:
                self.L.sfmhip_device_free(dptr)
        else:
            rc = self.L.sfmhip_sift_detect_and_compute(*head, None if "descriptors" in null else d.ctypes.data, np_)
        return rc, n.value, k, d, dptr.value


@pytest.fixture(scope="module")
def roomy(ctx):
    """the capacity image and its full answer through the Python wrapper"""
    g = np.ascontiguousarray(I.image("texture_129"))
    K, D = features.sift_detect_and_compute(g, ctx=ctx)
    assert len(K) >= 20
    return g, K, D


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacity_rules(ctx, roomy, device):
    """include/sfmhip.h: capacity 0 counts; 0 < capacity < n is SFMHIP_ERR_ARG with the count, nothing written and no
    device rows left; capacity = n is enough; a refused call leaves the context as good as before"""
    g, K, D = roomy
    n, raw = len(K), _Raw(ctx, device)

    def full(capacity):
        rc, cnt, k, d, dptr = raw.run(g, capacity)
        assert (rc, cnt) == (0, n) and np.array_equal(k[:n].view(np.int32), K.view(np.int32)) and np.array_equal(d[:n], D)
        assert np.all(k[n:] == _SENT) and np.all(d[n:] == _SENT)
        assert not device or dptr not in (None, 0, 0xDEAD0)
    rc, cnt, k, d, dptr = raw.run(g, 0, null=("keypoints",) if device else ("keypoints", "descriptors"))
    assert (rc, cnt) == (0, n) and (not device or dptr in (None, 0))
    full(n)
    full(n + 300)
    for capacity in (n - 1, 1):
        rc, cnt, k, d, dptr = raw.run(g, capacity, room=n + 8)
        assert (rc, cnt) == (ERR_ARG, n)
        assert np.all(k == _SENT) and np.all(d == _SENT) and (not device or dptr in (None, 0))
        full(n + 300)


def test_the_wrapper_retries_with_the_reported_count(ctx, roomy, monkeypatch):
    g, K, D = roomy
    real, caps = features.lib(), []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def sfmhip_sift_detect_and_compute(self, *a):
            caps.append(a[8])
            return real.sfmhip_sift_detect_and_compute(*a)
    monkeypatch.setattr(features, "lib", lambda: Spy())
    K1, D1 = features.sift_detect_and_compute(g, ctx=ctx, capacity=1)
    assert caps == [1, len(K)]
    assert np.array_equal(K1.view(np.int32), K.view(np.int32)) and np.array_equal(D1, D)
    del caps[:]
    K2, D2 = features.sift_detect_and_compute(g, ctx=ctx, capacity=len(K))          # exactly enough: one call
    assert caps == [len(K)] and np.array_equal(K2.view(np.int32), K.view(np.int32)) and np.array_equal(D2, D)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            features.sift_detect_and_compute(g, ctx=ctx, capacity=bad)
    assert caps == [len(K)]                                            # (refused before any call)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(ctx, roomy, device):
    """every argument the entry points refuse on the host, before any launch: SFMHIP_ERR_ARG, arrays untouched"""
    g, K, D = roomy
    raw, cap = _Raw(ctx, device), len(K) + 8
    bad = [dict(rows=1), dict(cols=1), dict(p=dict(I.DEFAULTS, n_layers=0)), dict(p=dict(I.DEFAULTS, n_layers=9)),
           dict(p=dict(I.DEFAULTS, sigma=0.0)), dict(p=dict(I.DEFAULTS, sigma=-1.6)), dict(capacity=-1), dict(null=("gray",)),
           dict(null=("n_keypoints",)), dict(null=("keypoints",)), dict(null=("descriptors",))]
    for kw in bad:
        kw = dict(kw)
        rc, cnt, k, d, dptr = raw.run(g, kw.pop("capacity", cap), room=cap, **kw)
        assert rc == ERR_ARG, kw
        assert np.all(k == _SENT) and np.all(d == _SENT) and cnt == -5 and dptr == 0xDEAD0, kw
    rc, cnt, k, d, dptr = raw.run(g, cap)                              # and the context still answers
    assert (rc, cnt) == (0, len(K)) and np.array_equal(d[:cnt], D)


def test_batch_refusals(ctx, roomy):
    """n_images = 0 is fine; one bad image refuses the whole call before any output is written"""
    import ctypes as C
    from sfm_danpipeline_amd import _lib
    g, K, D = roomy
    L = _lib.lib()
    assert features.sift_batch([], ctx=ctx) == []
    assert L.sfmhip_sift_batch(ctx.h, 0, None, None, None, 3, 0.04, 10.0, 1.6, None, None, None) == 0
    small = np.ascontiguousarray(I.degenerate_image((11, 40)))
    for bad in ("rows", "gray"):
        ptrs = (C.c_void_p * 3)(g.ctypes.data, small.ctypes.data, None if bad == "gray" else small.ctypes.data)
        rows = np.array([g.shape[0], small.shape[0], 1 if bad == "rows" else small.shape[0]], np.int32)
        cols = np.array([g.shape[1], small.shape[1], small.shape[1]], np.int32)
        kp, dd = (C.c_void_p * 3)(0x1230, 0x1230, 0x1230), (C.c_void_p * 3)(0x4560, 0x4560, 0x4560)
        nk = np.full(3, -9, np.int32)
        rc = L.sfmhip_sift_batch(ctx.h, 3, ptrs, rows.ctypes.data, cols.ctypes.data, 3, 0.04, 10.0, 1.6, kp, dd, nk.ctypes.data)
        assert rc == ERR_ARG
        assert list(kp) == [0x1230] * 3 and list(dd) == [0x4560] * 3 and nk.tolist() == [-9] * 3, bad
    for nl, sg in ((0, 1.6), (9, 1.6), (3, 0.0)):
        with pytest.raises(_lib.SfmHipError):
            features.sift_batch([g, small], nl, 0.04, 10.0, sg, ctx=ctx)
    (Kb, ddb), _ = features.sift_batch([g, small], ctx=ctx)              # and the context still answers
    assert np.array_equal(Kb.view(np.int32), K.view(np.int32)) and np.array_equal(ddb.download(), D)
