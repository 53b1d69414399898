"""CPU: the numpy reference of the dense stereo (tests/mvs_reference.py, written from DESIGN.md f-10's rule list) against
the g++ build of csrc/mvs.h (tests/stub/mvs_capi.cpp), bit for bit: index, depth, score, point count, xyz, normals, rgb.
The kernel and the stub share warp_sample, ncc, Top, Winner and fuse_pixel; the reference shares nothing with them, so a
mistake both made in rules 3-5 or 7 shows here.  tests/test_gpu_mvs.py runs the same cases on the device and compares it
with the stub and with the reference.  This file also asserts each case's preconditions, on the reference's output
alone, so that no case can go vacuous.

The cases (K has fx != fy and a principal point off the half-integers, [[100, 0, 23.3], [0, 96, 16.8]], unless noted;
"all pixels": ncc_min -1, var_min 0 on smooth random textures seen shifted from view to view):

  S1   rotations of N(0, 0.05) per axis and centre jitter, 33 x 47, 5 views, D 17, w 3, 4 sources, best 2, all pixels
  S2   the same poses on a rendered plane, w 7 (T = 30), best 4, default ncc_min / var_min
  S3   a rendered plane under rotations of N(0, 0.04), centre jitter 0.02, default options, D 33 between depths 1 and 8,
       40 x 56, 5 views: every view's depth map, then the whole call; the analytic bound below
  S4   one source rolled 90 degrees about the optical axis, one yawed 80 degrees, 33 x 47, D 9, w 2, all pixels: c <= 0 on
       part of the image, u and v leaving on all four sides; and (S4-back, added here) a source yawed 180 degrees, whose
       every sample has c < 0 and would land inside the image if that were not asked
  S5   dmin 4, dmax 4 + 1e-7: every plane ties, every winner is index 0 with no parabola
  S6   winners on the first and the last plane: taken from S1
  S7   white images with one black pixel in 30, w 7, whole-pixel shifts (line cameras, fx = fy = 100), 40 x 60: a window's
       sum of q^2 passes 2^31
  S8   the left 27 columns of every view constant, default var_min: a tile that leaves early beside one that does not;
       and a reference view that is constant throughout
  S9   1 x 1, 1 x 40, 40 x 1, 2 x 2, 3 x 3 at w 1; 15 x 15, 15 x 17 at w 7 (no pixel with depth); 16 x 16, 17 x 17 at w 3;
       31 x 33 at w 7; 3 views, D 5
  S10  D 256, 8 sources, best 4, 24 x 37, 9 views, small rotations, all pixels
  S11  37 x 53 at level 2 and 67 x 45 at level 3, gray and BGR, against ref_pyramid; 3 x 3 at level 1 and 7 x 9 at level 2
       (a 1 x 1 and a 1 x 2 working image) created, swept and fused
  S12  the whole call with 2 views and n_src 4; with 5 views, n_src 8 and best 4; with per-view ranges; at D 9, 256 and
       9 again on one handle with a depth map in between
  S13  fusion under rotation: S3's depth maps given through set_depthmap, min_views 1, 3, 5, 6, eps 0 and 0.01, BGR
  S14  fusion where floor(u + 1/2) decides (a baseline of half a pixel, u = -0.5 and u = cols - 0.5, three pixels in four
       with depth so that the column matters), and depth maps holding NaN, +inf, -1, 0, a denormal and 1e30

Measured with the reference (equal to the header bit for bit): S1 has 82 462 of 84 850 existing samples with a vertical
weight (105 468 positions), S4 9 570 of 9 900 and 2 343 samples with c <= 0, S10 1 283 070 of 1 335 803.  S3: 6 206 pixels
with depth over the five views, refined inverse depth against render_posed's truth in hypothesis steps, median 0.0226,
95th percentile 0.6223 (the tail is the image border, where two sources see little); 1 295 fused points at min_views 3,
526 at 5, none at 6.  The bound asserted is twice the figures; the margin covers the texture's phase, not the platform.

What these cases do not catch is a contracted build: g++ -ffp-contract=fast -mfma on the stub (fused multiply-adds in
warp_sample and make_homographies) gave the reference's index, depth and score on S1, S3, S4 and S10.  A sample is
quantised to 1/32 pixel and a depth to float32, so a last-bit change shows only on a quantisation boundary."""
import numpy as np
import pytest

from tests import mvs_reference as R
from tests.test_mvs_cpu import StubMvs, _p, build_stub, opts

S3_BOUND = (2 * 0.0226, 2 * 0.6223)   # median, 95th percentile: twice the reference's figures (docstring)


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("mvsref") / "libmvscapi.so"))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def per_view(c, a):
    return np.broadcast_to(np.asarray(a, np.float64), (len(c.gray),))


# ---------------------------------------------------------------- preconditions, on the reference's output alone
def _vertical(r):
    assert 4 * r.stats["wy"] >= r.stats["valid"] > 0


def _pre_s1(c, r):
    _vertical(r)
    assert (r.idx >= 0).sum() >= 200
    assert (r.idx == 0).sum() >= 1 and (r.idx == c.opts["n_planes"] - 1).sum() >= 1            # S6


def _pre_s2(c, r):
    _vertical(r)
    assert (r.idx >= 0).sum() >= 100 and 16 + 2 * c.opts["window"] == 30


def _pre_s3(c, r):
    assert sum(int((m[0] >= 0).sum()) for m in r.maps) >= 3000 and len(r.points[0]) >= 500


def _pre_s4(c, r):
    assert r.stats["behind"] >= 500 and (r.idx >= 0).sum() >= 500


def _pre_s4_back(c, r):
    """every sample of the source that looks away is behind it, and would be inside the image"""
    H = R.ref_homographies(c.K, c.poses, 0, [2], 9, c.dmin, c.dmax)
    y, x = np.mgrid[0:33, 0:47]
    a, b, w = (H[4, 0, i, 0] * x + H[4, 0, i, 1] * y + H[4, 0, i, 2] for i in range(3))
    assert (w < 0).all() and ((a / w >= 0) & (a / w < 46) & (b / w >= 0) & (b / w < 32)).sum() >= 500
    assert r.stats["behind"] >= 9 * 33 * 47 and (r.idx >= 0).sum() >= 500


def _pre_s5(c, r):
    assert (r.idx >= 0).sum() >= 1000 and (r.idx <= 0).all()
    assert (r.depth[r.idx == 0] == np.float32(c.dmax)).all()                                   # no parabola: the far plane itself


def _pre_s7(c, r):
    H = R.ref_homographies(c.K, c.poses, c.ref, c.src, c.opts["n_planes"], c.dmin, c.dmax)
    y, x = np.mgrid[0:40, 0:60]
    q = R.ref_sample(c.gray[c.src[0]], H[4, 0], x, y)
    win = np.lib.stride_tricks.sliding_window_view(q, (15, 15))
    full = (win >= 0).all((2, 3))
    assert full.any() and ((win.astype(np.int64) ** 2).sum((2, 3))[full] >= 2 ** 31).any()
    assert (r.idx >= 0).sum() >= 500


def _pre_s8_seam(c, r):
    win = np.lib.stride_tricks.sliding_window_view(16 * c.gray[c.ref].astype(np.int64), (7, 7))
    vr = 49 * (win ** 2).sum((2, 3)) - win.sum((2, 3)) ** 2                                    # of the pixels 3 ... rows - 4, 3 ... cols - 4
    assert (vr[0:13, 0:13] < c.opts["var_min"]).all()                                          # the tile of rows and columns 0 ... 15
    assert (vr[0:13, 13:29] >= c.opts["var_min"]).any() and (vr[0:13, 13:29] < c.opts["var_min"]).any()   # columns 16 ... 31: mixed
    assert (r.idx >= 0).sum() >= 500 and (r.idx[:, :24] == -1).all()


def _pre_s8_flat(c, r):
    assert (r.idx == -1).all() and (r.score == 0).all()              # no pixel with depth, the scores finite


def _pre_s10(c, r):
    _vertical(r)
    assert (r.idx >= 0).sum() >= 200 and len(np.unique(r.idx)) >= 50
    assert (c.opts["n_planes"], c.opts["n_src"], c.opts["n_best"], len(c.src)) == (256, 8, 4, 8)


def _pre_points(c, r):
    assert len(r.points[0]) >= 100


def _pre_s12_short(c, r):
    """the source choice is short: fewer other views than n_src"""
    assert len(R.ref_sources(c.poses, c.ref, c.opts["n_src"])) == len(c.gray) - 1 < c.opts["n_src"]
    _pre_points(c, r)


def _pre_s9_empty(c, r):
    assert (r.idx == -1).all()


def _pre_s9_some(c, r):
    assert (r.idx >= 0).any()


PRE = {"S1": _pre_s1, "S2": _pre_s2, "S3": _pre_s3, "S4": _pre_s4, "S4-back": _pre_s4_back, "S5": _pre_s5, "S7": _pre_s7, "S8-seam": _pre_s8_seam,
       "S8-flat": _pre_s8_flat, "S10": _pre_s10, "S12-two": _pre_s12_short, "S12-five": _pre_s12_short, "S12-ranges": _pre_points,
       "S12-reuse-9": _pre_points, "S12-reuse-256": _pre_points}
PRE.update({f"S9-{a}x{b}": _pre_s9_empty for a, b, w in R.S9_EMPTY})
PRE.update({f"S9-{a}x{b}": _pre_s9_some for a, b, w in R.S9_SOME})


# ---------------------------------------------------------------- the transcriptions of rules 2, 3 and 6
@pytest.mark.parametrize("name", ["S1", "S4", "S7", "S10", "S12-ranges"])
def test_homographies_and_sources_equal_the_header(ms, name):
    c = R.case(name)
    for ref in range(len(c.gray)):
        for n_src in (1, 4, 8):
            src = np.zeros(8, np.int32)
            m = ms.mvs_sources(_p(np.ascontiguousarray(c.poses)), len(c.gray), ref, n_src, _p(src))
            assert list(src[:m]) == R.ref_sources(c.poses, ref, n_src) and m == min(n_src, len(c.gray) - 1)
        src = np.array(R.ref_sources(c.poses, ref, 8), np.int32)
        D, lo, hi = c.opts["n_planes"], per_view(c, c.dmin)[ref], per_view(c, c.dmax)[ref]
        H = np.zeros((D, len(src), 3, 3))
        ms.mvs_homographies(_p(np.ascontiguousarray(c.K)), _p(np.ascontiguousarray(c.poses)), ref, len(src), _p(src), D, lo, hi, _p(H))
        assert same(H, R.ref_homographies(c.K, c.poses, ref, list(src), D, lo, hi))


def test_source_ties_go_to_the_lower_index():
    P = np.zeros((6, 3, 4))
    P[:, :, :3] = np.eye(3)
    P[:, 0, 3] = -np.array([0.0, 1.0, 2.0, 4.0, 3.0, -1.0])                # tests/test_mvs_cpu.py's centres
    assert R.ref_sources(P, 1, 4) == [0, 2, 4, 5] and R.ref_sources(P, 3, 8) == [4, 2, 1, 0, 5]


@pytest.mark.parametrize("name", ["S1", "S4"])
def test_sample_equals_the_header(ms, name):
    c = R.case(name)
    H = R.ref_homographies(c.K, c.poses, c.ref, c.src, c.opts["n_planes"], c.dmin, c.dmax)
    rows, cols = c.gray.shape[1:]
    y, x = np.mgrid[0:rows, 0:cols]
    for k in (0, c.opts["n_planes"] - 1):
        for s, v in enumerate(c.src):
            img, h = np.ascontiguousarray(c.gray[v]), np.ascontiguousarray(H[k, s])
            want = np.array([[ms.mvs_sample(_p(img), rows, cols, _p(h), j, i) for j in range(cols)] for i in range(rows)])
            assert np.array_equal(R.ref_sample(img, h, x, y), want)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_equals_the_header_build(ms, name):
    c, r = R.case(name), R.reference(name)
    if name in PRE:
        PRE[name](c, r)
    o = opts(ms, **c.kw)
    with StubMvs(ms, c.gray, c.K, c.poses, c.bgr, c.level) as M:
        i, d, s = M.depthmap(c.ref, c.src, per_view(c, c.dmin)[c.ref], per_view(c, c.dmax)[c.ref], o)
        print(f"{name}: {int((r.idx >= 0).sum())} pixels with depth, samples {r.stats}; index / depth / score differ at "
              f"{int((i != r.idx).sum())} / {int((d != r.depth).sum())} / {int((s != r.score).sum())}")
        assert same(i, r.idx) and same(d, r.depth) and same(s, r.score)
        if r.points is not None:
            pts = M.run(c.dmin, c.dmax, o)
            print(f"    run: {len(pts[0])} points, the reference {len(r.points[0])}")
            assert all(same(a, b) for a, b in zip(pts, r.points))


def check_s3(make, mk):
    """every view's depth map with the sources of rule 6 against the reference, then the measured bound"""
    c, r = R.case("S3"), R.reference("S3")
    with make(c.gray, c.K, c.poses, c.bgr, 0) as M:
        maps = [M.depthmap(v, R.ref_sources(c.poses, v, 4), c.dmin, c.dmax, mk(**c.kw)) for v in range(5)]
    for got, want in zip(maps, r.maps):
        assert all(same(a, b) for a, b in zip(got, want))
    px, med, p95 = R.s3_step_errors(maps)
    print(f"S3: {px} pixels with depth, |inverse depth error| median {med:.4f} p95 {p95:.4f} steps")
    assert px >= 3000 and med <= S3_BOUND[0] and p95 <= S3_BOUND[1]


def test_s3_rendered_scene_under_rotation(ms):
    check_s3(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))


def check_s13(make, mk):
    """S3's depth maps (the reference's) through set_depthmap: the fusion alone, under rotated poses"""
    c, r = R.case("S3"), R.reference("S3")
    depth = np.stack([m[1] for m in r.maps])
    counts = {}
    with make(c.gray, c.K, c.poses, c.bgr, 0) as M:
        for v in range(5):
            M.set_depthmap(v, depth[v])
        for mv in (1, 3, 5, 6):
            for eps in (0.0, 0.01):
                want = R.ref_fuse(c.K, c.poses, depth, c.gray, c.bgr, eps, mv)
                got = M.fuse(mk(min_views=mv, eps=eps))
                counts[(mv, eps)] = len(want[0])
                assert all(same(a, b) for a, b in zip(got, want)), (mv, eps)
    print(f"S13: points per (min_views, eps): {counts}")
    assert counts[(1, 0.0)] == int((depth > 0).sum()) >= 3000                  # eps 0: nothing is consistent, every pixel its own owner
    assert counts[(3, 0.01)] >= 500 and 0 < counts[(5, 0.01)] < counts[(3, 0.01)] and counts[(6, 0.01)] == 0


def test_s13_fusion_under_rotation(ms):
    check_s13(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))


def check_s14_half_pixel(make, mk):
    for n in (3, 4):
        gray, bgr, P = R.fusion_line(n, 0.125)
        has = R.half_pixel_has(n)
        depth = np.where(has, np.float32(2.0), np.float32(0.0))
        with make(gray, R.FK, P, bgr, 0) as M:
            for v in range(n):
                M.set_depthmap(v, depth[v])
            for mv in range(1, n + 2):
                exp = R.half_pixel_expected(n, mv, has)
                want = R.ref_fuse(R.FK, P, depth, gray, bgr, 0.0, mv)
                got = M.fuse(mk(min_views=mv, eps=0.0))                       # (everything is dyadic: eps 0 holds)
                assert len(want[0]) == len(exp) and all(same(a, b) for a, b in zip(got, want)), (n, mv)
                if exp:
                    r, y, x = np.array(exp).T
                    assert np.array_equal(got[0], np.stack([(x - 3.5) / 4 + 0.125 * r, (y - 3.5) / 4, 0 * r + 2.0], 1).astype(np.float32))
        assert len(R.half_pixel_expected(n, 2, has)) > 8 and 0 < has.sum() < has.size


def test_s14_fusion_where_the_rounding_decides(ms):
    check_s14_half_pixel(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))


def check_s14_odd_depths(make, mk):
    for n in (3, 4):
        gray, bgr, P = R.fusion_line(n, 0.25)
        depth = R.odd_depth_maps(n)
        with make(gray, R.FK, P, bgr, 0) as M:
            for v in range(n):
                M.set_depthmap(v, depth[v])
            for mv in (1, 2):
                want = R.ref_fuse(R.FK, P, depth, gray, bgr, 0.01, mv)
                got = M.fuse(mk(min_views=mv))
                assert len(got[0]) == len(want[0]) > 0 and all(R.same_bits(a, b) for a, b in zip(got, want)), (n, mv)
                if mv == 1:   # NaN, -1 and 0 are no depth; +inf, the denormal and 1e30 are: three of the six per view are emitted
                    assert len(want[0]) >= 3 * n and not np.isfinite(want[0]).all()


def test_s14_fusion_of_odd_depths(ms):
    check_s14_odd_depths(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))


def check_s11_pyramid(make):
    rng = np.random.RandomState(112)
    for rows, cols, level in ((37, 53, 2), (67, 45, 3)):
        gray = rng.randint(0, 256, (3, rows, cols)).astype(np.uint8)
        bgr = rng.randint(0, 256, (3, rows, cols, 3)).astype(np.uint8)
        for b in (None, bgr):
            with make(gray, R.K_AWK, R.posed_cameras(3, None, 0.0, 0.0, 0.1), b, level) as M:
                assert (M.rows, M.cols) == (rows >> level, cols >> level) and same(M.K, R.ref_level_K(R.K_AWK, level))
                for v in range(3):
                    lg, lb = M.level_image(v)
                    assert same(lg, R.ref_pyramid(gray[v], level)) and (lb is None) == (b is None)
                    assert b is None or same(lb, R.ref_pyramid(bgr[v], level))


def test_s11_pyramid_levels_two_and_three(ms):
    check_s11_pyramid(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level))


def check_s11_tiny(make, mk):
    """a 1 x 1 and a 1 x 2 working image: depth 2 in every pixel, fused at min_views 1"""
    for name in ("S11-3x3", "S11-7x9"):
        c = R.case(name)
        g, b = (np.stack([R.ref_pyramid(im, c.level) for im in a]) for a in (c.gray, c.bgr))
        depth = np.full(g.shape, 2.0, np.float32)
        with make(c.gray, c.K, c.poses, c.bgr, c.level) as M:
            assert (M.rows, M.cols) == g.shape[1:] == ((1, 1) if name == "S11-3x3" else (1, 2))
            for v in range(3):
                M.set_depthmap(v, depth[v])
            want = R.ref_fuse(R.ref_level_K(c.K, c.level), c.poses, depth, g, b, 0.01, 1)
            got = M.fuse(mk(min_views=1))
            assert len(want[0]) > 0 and all(same(a, b) for a, b in zip(got, want))


def test_s11_images_of_one_and_two_pixels(ms):
    check_s11_tiny(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))


def check_s12_reuse(make, mk):
    """one handle: the whole call at 9 planes, at 256, at 9 again, a depth map in between; the third equals the first"""
    c9, c256 = R.case("S12-reuse-9"), R.case("S12-reuse-256")
    r9, r256 = R.reference("S12-reuse-9"), R.reference("S12-reuse-256")
    with make(c9.gray, c9.K, c9.poses, None, 0) as M:
        first = M.run(c9.dmin, c9.dmax, mk(**c9.kw))
        M.depthmap(0, [1, 2], 2.0, 3.0, mk(**c9.kw))
        big = M.run(c256.dmin, c256.dmax, mk(**c256.kw))
        i, d, s = M.depthmap(c256.ref, c256.src, c256.dmin, c256.dmax, mk(**c256.kw))
        third = M.run(c9.dmin, c9.dmax, mk(**c9.kw))
    assert all(same(a, b) for a, b in zip(first, r9.points)) and all(same(a, b) for a, b in zip(big, r256.points))
    assert same(i, r256.idx) and same(d, r256.depth) and same(s, r256.score)
    assert all(same(a, b) for a, b in zip(third, first)) and len(first[0]) >= 100 and len(big[0]) >= 100


def test_s12_one_handle_at_9_256_and_9_planes(ms):
    check_s12_reuse(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))
