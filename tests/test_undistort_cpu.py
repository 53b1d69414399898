"""CPU: the lens-distortion resampling in front of the dense stereo through tests/stub/undistort_capi.cpp:
the g++ build of csrc/undistort.h, the header the HIP kernels are compiled from.

There is no library to pin parity against, so the contract is the rule list: a literal Python transcription of rules 1-6
must equal the stub byte for byte.  That the step does what it is for is checked on the scenes of tests/test_mvs_cpu.py,
rendered through a distorted camera (the model inverted per pixel by fixed-point iteration to 1e-12), undistorted by the stub,
run through the stereo's host build and held to the bounds the pinhole path has to meet (SLANT_BOUND, SPHERE_BOUND: twice
the pinhole path's own figures, never the new code's).

Measured with this header: refined inverse depth against the analytic value over the accepted interior pixels, in hypothesis
steps, accepted pixels / median / 95th percentile, coefficient sets A = (-0.25, 0.08, 0.002, -0.0015, 0) and
B = (0.2, -0.05, -0.002, 0.001, 0.01):
  scene, set    undistorted first           fed as they are            pinhole render (tests/test_mvs_cpu.py)
  slanted, A    528 / 0.0437 / 0.1252       528 / 0.2609 / 0.7979      0.0421 / 0.1162
  slanted, B    528 / 0.0419 / 0.1134       528 / 0.2217 / 0.5330
  sphere, A     772 / 0.0382 / 0.0983       772 / 0.3216 / 0.7425      0.0218 / 0.0697
  sphere, B     772 / 0.0234 / 0.0891       772 / 0.1886 / 0.5594
The interior mask of the scenes (window + largest disparity from every border) lies inside set B's invalid margin, hence the
equal counts."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_mvs_cpu import (BASE, COLS, D, DMAX, DMIN, K0, LAM, ROWS, SLANT_BOUND, SPHERE_BOUND, StubMvs, hit_depth, interior,
                                line_cameras, opts, plane_inv, step_errors, texture)
from tests.test_mvs_cpu import build_stub as build_mvs_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "undistort_capi.cpp")
SET_A = (-0.25, 0.08, 0.002, -0.0015, 0.0)     # barrel: the edge pixels of the 64 x 96 scenes move by about 2.7 pixels
SET_B = (0.2, -0.05, -0.002, 0.001, 0.01)      # pincushion: leaves invalid margins
SET_T = (0.0, 0.0, 0.03, -0.02, 0.0)           # tangential only
K_ODD = np.array([[617.3, 0, 301.7], [0, 611.9, 243.1], [0, 0, 1]])
# accepted interior pixels of a numpy prototype of the rule list (the floors the tests hold the header to, less 10 % for the
# mask's details): (kind, set) -> count
FLOORS = {("slanted", SET_A): 528, ("slanted", SET_B): 311, ("sphere", SET_A): 772, ("sphere", SET_B): 626}


def build_stub(so):
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp, f64, ci = C.c_void_p, C.c_double, C.c_int
    lib.und_distort_pixel.argtypes = [vp, vp, ci, ci, vp]
    lib.und_distort_pixel.restype = None
    lib.und_quantise.argtypes = [f64, f64, ci, ci, vp]
    lib.und_quantise.restype = None
    lib.und_sample.argtypes = [vp, ci, ci, ci, ci, f64, f64]
    lib.und_undistort.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.und_level_mask.argtypes = [vp, ci, ci, ci, vp]
    lib.und_level_mask.restype = None
    lib.und_seam.argtypes = [vp, ci, ci, ci, vp, vp, vp]
    lib.und_seam.restype = None
    return lib


@pytest.fixture(scope="module")
def us(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("und") / "libundcapi.so"))


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_mvs_stub(str(tmp_path_factory.mktemp("mvs") / "libmvscapi.so"))


def _p(a):
    return a.ctypes.data


# ---------------------------------------------------------------- the stub behind numpy (shared with tests/test_gpu_undistort.py)
def stub_undistort(us, images, K, dist):
    """(images [n, rows, cols(, 3)] uint8, valid [rows, cols] uint8) of the header's host build"""
    src = [np.ascontiguousarray(im, np.uint8) for im in images]
    ch = 3 if src[0].ndim == 3 else 1
    rows, cols = src[0].shape[:2]
    out = np.zeros((len(src),) + src[0].shape, np.uint8)
    valid = np.zeros((rows, cols), np.uint8)
    sp = (C.c_void_p * len(src))(*[_p(im) for im in src])
    dp = (C.c_void_p * len(src))(*[out[i].ctypes.data for i in range(len(src))])
    K, dist = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(dist, np.float64).reshape(5)
    rc = us.und_undistort(len(src), rows, cols, ch, sp, _p(K), _p(dist), dp, _p(valid))
    if rc:
        raise ValueError(f"status {rc}")
    return out, valid


def stub_level_mask(us, valid0, level):
    v = np.ascontiguousarray(valid0, np.uint8)
    out = np.zeros((v.shape[0] >> level, v.shape[1] >> level), np.uint8)
    us.und_level_mask(_p(v), v.shape[0], v.shape[1], level, _p(out))
    return out


def stub_seam(us, valid, window, idx, depth, score):
    """rule 7 on copies of one depth map"""
    v = np.ascontiguousarray(valid, np.uint8)
    idx, depth, score = np.array(idx, np.int32), np.array(depth, np.float32), np.array(score, np.float32)
    assert idx.shape == depth.shape == score.shape == v.shape
    us.und_seam(_p(v), v.shape[0], v.shape[1], int(window), _p(idx), _p(depth), _p(score))
    return idx, depth, score


def stub_run(us, ms, M, poses, valid, dmin, dmax, o):
    """sfmhip_mvs_run on a handle created with distortion, staged on the stereo's host build M: per view rule 6 of f-10 for
    the sources, the depth map, f-14's rule 7 under the level mask `valid`, then the fusion."""
    poses = np.ascontiguousarray(poses, np.float64)
    lo, hi = np.broadcast_to(np.asarray(dmin, np.float64), (M.n,)), np.broadcast_to(np.asarray(dmax, np.float64), (M.n,))
    for v in range(M.n):
        src = np.zeros(8, np.int32)
        k = ms.mvs_sources(_p(poses), M.n, v, o.n_src, _p(src))
        idx, d, s = stub_seam(us, valid, o.window, *M.depthmap(v, src[:k], float(lo[v]), float(hi[v]), o))
        M.set_depthmap(v, d)
    return M.fuse(o)


# ---------------------------------------------------------------- rules 1-6, transcribed
def forward(xn, yn, dist):
    """the forward model of csrc/camera.h's project_point on normalised coordinates, in its operation order"""
    k1, k2, p1, p2, k3 = dist
    r2 = xn * xn + yn * yn
    r4 = r2 * r2
    r6 = r4 * r2
    a1 = 2 * xn * yn
    a2 = r2 + 2 * xn * xn
    a3 = r2 + 2 * yn * yn
    cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
    return xn * cdist + p1 * a1 + p2 * a2, yn * cdist + p1 * a3 + p2 * a1


def rule_quantise(u, v, rows, cols):
    """rules 2-3 for one position: (ix, iy, wx, wy) or None"""
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    fu, fv = math.floor(u), math.floor(v)
    ix, iy = int(fu), int(fv)
    wx, wy = math.floor((u - fu) * 32 + 0.5), math.floor((v - fv) * 32 + 0.5)
    if wx == 32:
        wx, ix = 0, ix + 1
    if wy == 32:
        wy, iy = 0, iy + 1
    for tx, ty, w in ((ix, iy, (32 - wx) * (32 - wy)), (ix + 1, iy, wx * (32 - wy)), (ix, iy + 1, (32 - wx) * wy), (ix + 1, iy + 1, wx * wy)):
        if w and not (0 <= tx < cols and 0 <= ty < rows):
            return None
    return ix, iy, wx, wy


def rule_undistort(images, K, dist):
    """rules 1-5 in plain Python floats and integers, one pixel at a time"""
    images = np.asarray(images)
    imgs = images.reshape(images.shape[:3] + (-1,)).astype(int)
    n, rows, cols, ch = imgs.shape
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    out, valid = np.zeros(imgs.shape, np.uint8), np.zeros((rows, cols), np.uint8)
    for y in range(rows):
        for x in range(cols):
            xd, yd = forward((x - cx) / fx, (y - cy) / fy, [float(d) for d in dist])
            q = rule_quantise(xd * fx + cx, yd * fy + cy, rows, cols)
            if q is None:
                continue
            ix, iy, wx, wy = q
            tap = lambda tx, ty, w: imgs[:, ty, tx] if w else 0          # a tap of weight zero is not read
            a, b = tap(ix, iy, 1), tap(ix + 1, iy, wx)
            c, d = tap(ix, iy + 1, wy), tap(ix + 1, iy + 1, wx * wy)
            out[:, y, x] = ((a * (32 - wx) + b * wx) * (32 - wy) + (c * (32 - wx) + d * wx) * wy + 512) >> 10
            valid[y, x] = 1
    return out.reshape(images.shape), valid


def rule_level_mask(valid0, level):
    """rule 6: all 2^L x 2^L level-0 pixels under a level-L pixel; a dropped odd row or column is absent"""
    s = 1 << level
    r, c = valid0.shape[0] >> level, valid0.shape[1] >> level
    return valid0[:r * s, :c * s].reshape(r, s, c, s).min(axis=(1, 3)).astype(np.uint8)


def near_invalid(valid, window):
    """the pixels whose (2 window + 1)^2 window holds an invalid pixel of the mask (by shifting, not by the header's loop)"""
    bad = np.pad(valid == 0, window)
    out = np.zeros(valid.shape, bool)
    for dy in range(2 * window + 1):
        for dx in range(2 * window + 1):
            out |= bad[dy:dy + valid.shape[0], dx:dx + valid.shape[1]]
    return out


# ---------------------------------------------------------------- scenes through a distorted camera (shared with the GPU file)
def invert_model(xd, yd, dist):
    """normalised pinhole coordinates whose forward model is (xd, yd): fixed-point iteration to 1e-12, then checked"""
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(500):
        r2 = x * x + y * y
        cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        nx = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / cd
        ny = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / cd
        step = max(np.abs(nx - x).max(), np.abs(ny - y).max())
        x, y = nx, ny
        if step < 1e-12:
            break
    else:
        raise AssertionError("the distortion model did not invert")
    return x, y


def surfaces_of(kind):
    z0 = 1 / plane_inv(16)
    return {"slanted": [("plane", (-np.sin(np.pi / 6), 0, np.cos(np.pi / 6)), z0 * np.cos(np.pi / 6))],
            "sphere": [("sphere", (0, 0, z0 + 0.9), 1.0), ("plane", (0, 0, 1), z0 + 1.2)]}[kind]


def distorted_scene(kind, dist, level=0):
    """(gray through the distorted camera at 2^level times 64 x 96, analytic PINHOLE depth at 64 x 96, K of level 0, poses):
    test_mvs_cpu.scene with the lens in front"""
    poses = line_cameras()
    f = 2 ** level
    Kr = np.array(K0)
    Kr[0, 0], Kr[1, 1], Kr[0, 2], Kr[1, 2] = K0[0, 0] * f, K0[1, 1] * f, (K0[0, 2] + 0.5) * f - 0.5, (K0[1, 2] + 0.5) * f - 0.5
    x, y = np.meshgrid(np.arange(COLS * f, dtype=float), np.arange(ROWS * f, dtype=float))
    xd, yd = (x - Kr[0, 2]) / Kr[0, 0], (y - Kr[1, 2]) / Kr[1, 1]
    dx, dy = invert_model(xd, yd, dist)
    bx, by = forward(dx, dy, dist)
    assert max(np.abs(bx * Kr[0, 0] + Kr[0, 2] - x).max(), np.abs(by * Kr[1, 1] + Kr[1, 2] - y).max()) < 1e-9   # the pixel comes back
    gray = []
    for P in poses:
        Cc = -P[:, 3]
        z = hit_depth(surfaces_of(kind), Cc, dx, dy)
        gray.append(np.clip(np.rint(127.5 + 110 * texture(Cc[0] + z * dx, Cc[1] + z * dy, LAM, 1)), 0, 255).astype(np.uint8))
    x, y = np.meshgrid(np.arange(COLS, dtype=float), np.arange(ROWS, dtype=float))
    px, py = (x - K0[0, 2]) / K0[0, 0], (y - K0[1, 2]) / K0[1, 1]
    depth = np.stack([hit_depth(surfaces_of(kind), -P[:, 3], px, py) for P in poses])
    return np.stack(gray), depth, Kr, poses


def surface_figures(idx, d, truth, kind, o):
    """(accepted interior pixels, median, 95th percentile in hypothesis steps): the mask and the error of test_mvs_cpu.check_surface"""
    mask = interior(o, 2 * BASE * 100 / truth[2].min()) & (idx >= 0)
    if kind == "sphere":
        x, y = np.meshgrid(np.arange(COLS), np.arange(ROWS))
        mask &= (x - K0[0, 2]) ** 2 + (y - K0[1, 2]) ** 2 < 22 ** 2
    return (int(mask.sum()),) + step_errors(d, truth[2], mask)


def check_undistorted_surface(kind, dist, bound, depthmap_of, o):
    """depthmap_of(gray, K, poses, dist or None) -> (idx, depth, score) of view 2 against the four others at level 0 with D
    planes and o's window: undistorted first and rule 7 applied with `dist`, the views as they are without.  Asserts the bound
    and the floor on the former, and that the latter miss the bound."""
    gray, truth, K, P = distorted_scene(kind, dist)
    n, med, p95 = surface_figures(*depthmap_of(gray, K, P, dist)[:2], truth, kind, o)
    rn, rmed, rp95 = surface_figures(*depthmap_of(gray, K, P, None)[:2], truth, kind, o)
    print(f"{kind} {dist}: undistorted first {n} pixels, median {med:.4f} p95 {p95:.4f} steps; fed as is {rn} pixels, "
          f"median {rmed:.4f} p95 {rp95:.4f}")
    assert n >= 0.9 * FLOORS[(kind, dist)]
    assert med <= bound[0] and p95 <= bound[1]
    assert rmed > bound[0] and rp95 > bound[1]            # the scene discriminates: the same views as they are miss the bound
    return n, med, p95


# ---------------------------------------------------------------- tests
SIZES = [(9, 11, 1), (9, 11, 3), (37, 53, 1), (37, 53, 3)]


@pytest.mark.parametrize("rows,cols,ch", SIZES)
def test_transcription_equals_the_header_build(us, rows, cols, ch):
    rng = np.random.RandomState(rows + ch)
    img = rng.randint(0, 256, (2, rows, cols) + ((3,) if ch == 3 else ())).astype(np.uint8)
    K = np.array([[0.9 * cols, 0, cols / 2 - 0.3], [0, 0.95 * cols, rows / 2 - 0.8], [0, 0, 1]])
    for dist in (SET_A, SET_B, SET_T):
        got, gv = stub_undistort(us, img, K, dist)
        want, wv = rule_undistort(img, K, dist)
        print(f"{rows} x {cols} x {ch} {dist}: {int(gv.sum())} of {rows * cols} pixels valid")
        assert np.array_equal(gv, wv) and np.array_equal(got, want)
        assert 0 < gv.sum() and ((got.reshape(2, rows, cols, -1)[:, gv == 0] == 0).all())
        for level in (1, 2):
            assert np.array_equal(stub_level_mask(us, gv, level), rule_level_mask(wv, level))
    uv = np.zeros(2)
    d = np.array(SET_A)
    us.und_distort_pixel(_p(K.reshape(9).copy()), _p(d), 3, 2, _p(uv))    # rule 1 alone, to the bit
    xd, yd = forward((3 - K[0, 2]) / K[0, 0], (2 - K[1, 2]) / K[1, 1], SET_A)
    assert uv[0] == xd * K[0, 0] + K[0, 2] and uv[1] == yd * K[1, 1] + K[1, 2]


def test_sample_units(us):
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (9, 11)).astype(np.uint8)
    s = lambda u, v, im=img: us.und_sample(_p(im), im.shape[0], im.shape[1], 1, 0, u, v)
    q = np.zeros(5, np.int32)

    def quant(u, v):
        us.und_quantise(u, v, 9, 11, _p(q))
        return tuple(int(a) for a in q)

    for y in range(9):
        for x in range(11):
            assert s(float(x), float(y)) == int(img[y, x])                # an integer map is a copy, last row and column included
    assert quant(2 + 31.5 / 32, 4.0) == (3, 4, 0, 0, 1)                   # fraction 31.5/32 rounds to weight 32: a carry
    assert s(2 + 31.5 / 32, 4.0) == int(img[4, 3])
    assert quant(-1e-15, 3.0) == (0, 3, 0, 0, 1) and s(-1e-15, 3.0) == int(img[3, 0])   # floor of a negative, then the carry
    assert quant(3.0, -1e-15) == (3, 0, 0, 0, 1)
    assert quant(10.0, 8.0) == (10, 8, 0, 0, 1)                           # the taps right of / below it weigh zero: not needed
    assert quant(9 + 31.5 / 32, 7 + 31.5 / 32) == (10, 8, 0, 0, 1)        # ... also after a carry
    assert s(10.0 + 1 / 32, 3.0) == -1 and s(3.0, 8.0 + 1 / 32) == -1     # a tap of weight 1 off the image: invalid
    assert s(-1 / 32, 3.0) == -1 and s(3.0, -0.5) == -1 and s(-1.0, 3.0) == -1
    assert s(10.0 + 0.4 / 32, 3.0) == int(img[3, 10])                     # ... a weight that rounds to zero is none
    assert s(11.0, 3.0) == -1 and s(3.0, 9.0) == -1 and s(1e300, 3.0) == -1 and s(-1e300, 3.0) == -1
    assert s(float("nan"), 3.0) == -1 and s(3.0, float("inf")) == -1 and s(float("-inf"), 3.0) == -1
    a, b, c, d = (int(v) for v in (img[4, 2], img[4, 3], img[5, 2], img[5, 3]))
    for fx, fy in ((0.5, 0.0), (0.0, 0.5), (0.25, 0.75), (15.4 / 32, 0.49 / 32), (15.5 / 32, 0.5 / 32), (31.4 / 32, 31.4 / 32)):
        wx, wy = int(np.floor(fx * 32 + 0.5)), int(np.floor(fy * 32 + 0.5))
        assert s(2 + fx, 4 + fy) == ((a * (32 - wx) + b * wx) * (32 - wy) + (c * (32 - wx) + d * wx) * wy + 512) >> 10
    two = np.array([[0, 1], [0, 0]], np.uint8)                            # the rounding constant: 1 * 16 * 32 = 512 of 1024 rounds up,
    assert s(0.5, 0.0, two) == 1 and s(15 / 32, 0.0, two) == 0            # 480 does not
    white = np.full((4, 4), 255, np.uint8)
    assert s(1.5, 1.5, white) == 255                                      # no overflow, no drift of a flat picture
    bgr = rng.randint(0, 256, (5, 6, 3)).astype(np.uint8)                 # interleaved channels: taps one pixel, not one byte, apart
    for c3 in range(3):
        e = (int(bgr[2, 1, c3]) * 16 + int(bgr[2, 2, c3]) * 16) * 32 + 512 >> 10
        assert us.und_sample(_p(bgr), 5, 6, 3, c3, 1.5, 2.0) == e


def test_zero_coefficients_copy_the_picture(us):
    """rule 5: (x - cx) / fx * fx + cx may miss x by an ulp; the quantisation to 1/32 and its carry absorb it"""
    rng = np.random.RandomState(5)
    for shape in ((48, 64), (48, 64, 3)):
        img = rng.randint(0, 256, (2,) + shape).astype(np.uint8)
        got, valid = stub_undistort(us, img, K_ODD, np.zeros(5))
        assert np.array_equal(got, img) and (valid == 1).all()


def test_refusals(us):
    img = np.zeros((1, 4, 5), np.uint8)
    stub_undistort(us, img, K0, SET_A)
    for K, dist in ((np.diag([0.0, 100, 1]), SET_A), (np.diag([100.0, 0, 1]), SET_A), (K0, (np.nan, 0, 0, 0, 0)), (K0, (0, 0, 0, 0, np.inf)),
                    (K0 * np.array([[1, 1, np.nan], [1, 1, 1], [1, 1, 1]]), SET_A)):
        with pytest.raises(ValueError, match="status -3"):
            stub_undistort(us, img, K, dist)
    with pytest.raises(ValueError, match="status -3"):
        stub_undistort(us, np.zeros((1, 0, 5), np.uint8), K0, SET_A)
    K, d, out = np.ascontiguousarray(K0.reshape(9)), np.array(SET_A), np.zeros((4, 5, 2), np.uint8)
    sp, dp = (C.c_void_p * 1)(_p(img)), (C.c_void_p * 1)(_p(out))
    assert us.und_undistort(1, 4, 5, 2, sp, _p(K), _p(d), dp, None) == -3       # channels
    assert us.und_undistort(1, 4, 5, 1, sp, _p(K), _p(d), dp, None) == 0        # the mask is nullable
    assert us.und_undistort(1, 4, 5, 1, (C.c_void_p * 1)(None), _p(K), _p(d), dp, None) == -3
    assert us.und_undistort(1, 4, 5, 1, sp, None, _p(d), dp, None) == -3 and us.und_undistort(1, 4, 5, 1, sp, _p(K), None, dp, None) == -3


class Host:
    """the stereo's host build behind depthmap_of of check_undistorted_surface"""

    def __init__(self, us, ms):
        self.us, self.ms = us, ms

    def __call__(self, gray, K, P, dist):
        o = opts(self.ms, n_planes=D)
        views, valid = (gray, None) if dist is None else stub_undistort(self.us, gray, K, dist)
        with StubMvs(self.ms, views, K, P, level=0) as M:
            idx, d, s = M.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, o)
        return (idx, d, s) if dist is None else stub_seam(self.us, valid, o.window, idx, d, s)


@pytest.mark.parametrize("kind,bound", [("slanted", SLANT_BOUND), ("sphere", SPHERE_BOUND)])
@pytest.mark.parametrize("dist", [SET_A, SET_B])
def test_distorted_views_meet_the_pinhole_bounds_once_undistorted(us, ms, kind, bound, dist):
    check_undistorted_surface(kind, dist, bound, Host(us, ms), opts(ms, n_planes=D))


def test_no_depth_at_the_seam(us, ms):
    """rules 6 and 7 with the pincushion set at level 1: the mask equals the transcription's, every pixel within the window
    of an invalid level pixel loses its depth and no other pixel changes"""
    gray, truth, K, P = distorted_scene("slanted", SET_B, level=1)
    und, valid0 = stub_undistort(us, gray, K, SET_B)
    assert np.array_equal(valid0, rule_undistort(gray[:1], K, SET_B)[1])
    valid = stub_level_mask(us, valid0, 1)
    assert valid.shape == (ROWS, COLS) and np.array_equal(valid, rule_level_mask(valid0, 1))
    assert 0 < (valid == 0).sum() < valid.size / 4                        # pincushion: an invalid margin, not an invalid picture
    odd = stub_level_mask(us, valid0[:-1, :-3], 2)                        # 127 x 189: the dropped row and columns are absent
    assert odd.shape == (31, 47) and np.array_equal(odd, rule_level_mask(valid0[:-1, :-3], 2))
    o = opts(ms, n_planes=D)
    with StubMvs(ms, und, K, P, level=1) as M:
        raw = M.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, o)
    idx, d, s = stub_seam(us, valid, o.window, *raw)
    near = near_invalid(valid, o.window)
    print(f"seam: {int((valid == 0).sum())} invalid level pixels, {int(near.sum())} within the window, "
          f"{int((raw[0][near] >= 0).sum())} of them had a depth")
    assert (idx[near] == -1).all() and (d[near] == 0).all() and (s[near] == 0).all()
    assert all(np.array_equal(a[~near], b[~near]) for a, b in zip((idx, d, s), raw))
    assert (idx[~near] >= 0).sum() > 1000
    for w in (1, 7):                                                      # on a map that has a depth everywhere
        full = stub_seam(us, valid, w, np.full(valid.shape, 5), np.ones(valid.shape), np.ones(valid.shape))
        hit = near_invalid(valid, w)
        assert np.array_equal(full[0], np.where(hit, -1, 5)) and np.array_equal(full[1], np.where(hit, 0, 1).astype(np.float32))
        assert np.array_equal(full[2], full[1])


def test_undistort_under_asan_ubsan(tmp_path):
    """a stand-alone program over the header (its own main: -DUND_MAIN), run as a child process"""
    exe = str(tmp_path / "und_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DUND_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("checksum ")
