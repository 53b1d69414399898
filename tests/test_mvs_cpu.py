"""CPU: the dense multi-view stereo of map3D step 7 through tests/stub/mvs_capi.cpp: the g++ build of
csrc/mvs.h, the header the HIP kernels are compiled from.

pmvs2 expands patches, so parity is UNPINNED and it is used nowhere here; the contract is the rule list.  It is checked on
scenes this file renders itself: a texture of four sines (wavelengths >= 6 pixels of the working level) on an analytic
surface, seen by five cameras on a line with one orientation, so that every pixel's depth is known in closed form.

Measured with this header, refined inverse depth against the analytic value over the accepted interior pixels, in
hypothesis steps (median / 95th percentile): slanted plane (30 degrees) 0.0421 / 0.1162, sphere 0.0218 / 0.0697.  The
tests assert twice these figures; the margin covers the texture's phase, not the platform (the device is bit-equal).

Every scene of this file has identity rotations (v == y, no vertical weight, c == 1).  Rotated views, the option ceilings,
tiny images and an independent numpy reference of the rule list are tests/test_mvs_reference_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "mvs_capi.cpp")
THREADS = min(16, os.cpu_count() or 1)
SLANT_BOUND = (2 * 0.0421, 2 * 0.1162)   # median, 95th percentile: twice the host build's figures (docstring)
SPHERE_BOUND = (2 * 0.0218, 2 * 0.0697)


class MvsOpts(C.Structure):
    _fields_ = [("n_planes", C.c_int32), ("window", C.c_int32), ("n_src", C.c_int32), ("n_best", C.c_int32),
                ("min_views", C.c_int32), ("pad", C.c_int32), ("ncc_min", C.c_double), ("eps", C.c_double),
                ("var_min", C.c_double)]


def build_stub(so):
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp, f64, ci = C.c_void_p, C.c_double, C.c_int
    lib.mvs_default_opts.argtypes = [C.POINTER(MvsOpts)]
    lib.mvs_default_opts.restype = None
    lib.mvs_sample.argtypes = [vp, ci, ci, vp, ci, ci]
    lib.mvs_ncc_window.argtypes = [vp, vp, ci, vp]
    lib.mvs_sources.argtypes = [vp, ci, ci, ci, vp]
    lib.mvs_homographies.argtypes = [vp, vp, ci, ci, vp, ci, f64, f64, vp]
    lib.mvs_create.argtypes = [ci, ci, ci, vp, vp, vp, vp, ci]
    lib.mvs_create.restype = vp
    lib.mvs_free.argtypes = [vp]
    lib.mvs_free.restype = None
    lib.mvs_level.argtypes = [vp, vp, vp, vp, ci, vp, vp]
    lib.mvs_level.restype = None
    lib.mvs_depthmap.argtypes = [vp, ci, ci, vp, f64, f64, C.POINTER(MvsOpts), vp, vp, vp, ci]
    lib.mvs_set_depthmap.argtypes = [vp, ci, vp]
    lib.mvs_fuse.argtypes = [vp, C.POINTER(MvsOpts)]
    lib.mvs_run.argtypes = [vp, vp, vp, C.POINTER(MvsOpts), ci]
    lib.mvs_download.argtypes = [vp, vp, vp, vp]
    lib.mvs_download.restype = None
    return lib


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("mvs") / "libmvscapi.so"))


def opts(ms, **kw):
    o = MvsOpts()
    ms.mvs_default_opts(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k)
        setattr(o, k, v)
    return o


def _p(a):
    return a.ctypes.data


class StubMvs:
    """the host build behind the interface of sfm_danpipeline_amd.mvs.Mvs (shared with tests/test_gpu_mvs.py)"""

    def __init__(self, ms, gray, K, poses, bgr=None, level=1):
        self.ms = ms
        g = [np.ascontiguousarray(im, np.uint8) for im in gray]
        b = [np.ascontiguousarray(im, np.uint8) for im in bgr] if bgr is not None else None
        gp = (C.c_void_p * len(g))(*[_p(im) for im in g])
        bp = (C.c_void_p * len(b))(*[_p(im) for im in b]) if b else None
        K, poses = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(poses, np.float64).reshape(-1)
        rows, cols = g[0].shape
        self.h = ms.mvs_create(len(g), rows, cols, gp, bp, _p(K), _p(poses), level)
        if not self.h:
            raise ValueError("status -3")
        self.n, self.colour = len(g), b is not None
        r, c, k = C.c_int32(0), C.c_int32(0), np.zeros(9)
        ms.mvs_level(self.h, C.addressof(r), C.addressof(c), _p(k), -1, None, None)
        self.rows, self.cols, self.K = r.value, c.value, k.reshape(3, 3)

    def level_image(self, view):
        g = np.zeros((self.rows, self.cols), np.uint8)
        b = np.zeros((self.rows, self.cols, 3), np.uint8) if self.colour else None
        r, c = C.c_int32(0), C.c_int32(0)
        self.ms.mvs_level(self.h, C.addressof(r), C.addressof(c), None, view, _p(g), _p(b) if self.colour else None)
        return g, b

    def depthmap(self, ref, src, dmin, dmax, o=None):
        o = o or opts(self.ms)
        src = np.ascontiguousarray(src, np.int32).reshape(-1)
        idx, d, s = (np.zeros((self.rows, self.cols), t) for t in (np.int32, np.float32, np.float32))
        rc = self.ms.mvs_depthmap(self.h, ref, len(src), _p(src), dmin, dmax, C.byref(o), _p(idx), _p(d), _p(s), THREADS)
        if rc:
            raise ValueError(f"status {rc}")
        return idx, d, s

    def set_depthmap(self, view, depth):
        d = np.ascontiguousarray(depth, np.float32)
        assert d.shape == (self.rows, self.cols)
        if self.ms.mvs_set_depthmap(self.h, view, _p(d)):
            raise ValueError("status -3")

    def _points(self, m):
        if m < 0:
            raise ValueError(f"status {m}")
        xyz, nrm, rgb = np.zeros((max(m, 1), 3), np.float32), np.zeros((max(m, 1), 3), np.float32), np.zeros(max(m, 1), np.uint32)
        self.ms.mvs_download(self.h, _p(xyz), _p(nrm), _p(rgb))
        return xyz[:m].copy(), nrm[:m].copy(), rgb[:m].copy()

    def fuse(self, o=None):
        return self._points(self.ms.mvs_fuse(self.h, C.byref(o or opts(self.ms))))

    def run(self, dmin, dmax, o=None):
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(dmin, np.float64), (self.n,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(dmax, np.float64), (self.n,)))
        return self._points(self.ms.mvs_run(self.h, _p(lo), _p(hi), C.byref(o or opts(self.ms)), THREADS))

    def close(self):
        if self.h:
            self.ms.mvs_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---------------------------------------------------------------- scenes (shared with tests/test_gpu_mvs.py)
BASE = 0.16   # 9 pixels of disparity between neighbours on plane 16, 0.4375 pixels per hypothesis step


def line_cameras(n=5, baseline=BASE):
    """n cameras on the x axis around 0, identity rotation: poses [n, 3, 4] with t = -C"""
    P = np.zeros((n, 3, 4))
    P[:, :, :3] = np.eye(3)
    P[:, 0, 3] = -(np.arange(n) - (n - 1) / 2) * baseline
    return P


def texture(X, Y, lam, seed):
    """four sines of world wavelengths lam * (1, 1.5, 2.3, 3.7) in fixed directions, phases from the seed; in [-1, 1]"""
    rng = np.random.RandomState(seed)
    t = np.zeros_like(X)
    for m, ang in zip((1.0, 1.5, 2.3, 3.7), (0.3, 1.9, 1.1, 2.6)):
        t += np.sin(2 * np.pi * (np.cos(ang) * X + np.sin(ang) * Y) / (lam * m) + rng.uniform(0, 2 * np.pi))
    return t / 4


def hit_depth(surfaces, C, dx, dy):
    """depth (= ray parameter: the rays are (dx, dy, 1), the rotation is the identity) of the nearest surface"""
    best = np.full(dx.shape, np.inf)
    for s in surfaces:
        if s[0] == "plane":      # n . X = d, optionally only where X < xmax
            n, d = np.asarray(s[1], float), s[2]
            t = (d - n @ C) / (n[0] * dx + n[1] * dy + n[2])
            if len(s) > 3:
                t = np.where(C[0] + t * dx < s[3], t, np.inf)
        else:                    # sphere: centre, radius
            c, r = np.asarray(s[1], float), s[2]
            oc = C - c
            a = dx * dx + dy * dy + 1
            b = 2 * (oc[0] * dx + oc[1] * dy + oc[2])
            disc = b * b - 4 * a * (oc @ oc - r * r)
            t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        best = np.where((t > 0) & (t < best), t, best)
    return best


def render(K, rows, cols, poses, surfaces, lam, seed=1):
    """(gray [n, rows, cols] uint8, depth [n, rows, cols]) of the scene; the texture lives in the world's X, Y"""
    x, y = np.meshgrid(np.arange(cols, dtype=float), np.arange(rows, dtype=float))
    dx, dy = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]
    gray, depth = [], []
    for P in poses:
        Cc = -P[:, 3]
        z = hit_depth(surfaces, Cc, dx, dy)
        t = texture(Cc[0] + z * dx, Cc[1] + z * dy, lam, seed)
        gray.append(np.clip(np.rint(127.5 + 110 * t), 0, 255).astype(np.uint8))
        depth.append(z)
    return np.stack(gray), np.stack(depth)


def level_K(K, level):
    K = np.array(K, float)
    for _ in range(level):
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K[0, 0] / 2, K[1, 1] / 2, (K[0, 2] + 0.5) / 2 - 0.5, (K[1, 2] + 0.5) / 2 - 0.5
    return K


ROWS, COLS, D = 64, 96, 33
K0 = np.array([[100.0, 0, 47.5], [0, 100.0, 31.5], [0, 0, 1]])
DMIN, DMAX = 1.0, 8.0
STEP = (1 / DMIN - 1 / DMAX) / (D - 1)
LAM = 8 * 1.78 / 100   # 8 pixels at the scenes' depth


def plane_inv(k):
    return 1 / DMAX + k * STEP


def scene(kind, level=0):
    """(gray, analytic depth at the working level, K of level 0, poses, margin of pixels the sources may not see)"""
    poses = line_cameras()
    z0 = 1 / plane_inv(16)
    surfaces = {"fronto": [("plane", (0, 0, 1), z0)],
                "slanted": [("plane", (-np.sin(np.pi / 6), 0, np.cos(np.pi / 6)), z0 * np.cos(np.pi / 6))],
                "sphere": [("sphere", (0, 0, z0 + 0.9), 1.0), ("plane", (0, 0, 1), z0 + 1.2)],
                "edge": [("plane", (0, 0, 1), 1 / plane_inv(20), 0.02), ("plane", (0, 0, 1), 1 / plane_inv(10))]}[kind]
    Kr = np.array(K0)
    if level:  # rendered at 2^level times the size, so that the working level is the same picture
        f = 2 ** level
        Kr[0, 0], Kr[1, 1], Kr[0, 2], Kr[1, 2] = K0[0, 0] * f, K0[1, 1] * f, (K0[0, 2] + 0.5) * f - 0.5, (K0[1, 2] + 0.5) * f - 0.5
    gray, _ = render(Kr, ROWS << level, COLS << level, poses, surfaces, LAM)
    _, depth = render(K0, ROWS, COLS, poses, surfaces, LAM)
    return gray, depth, Kr, poses


def timing_scene(n=10, rows=480, cols=640):
    """n views of rows x cols on a line: a sphere in front of a plane, texture wavelengths of 8 level-1 pixels and up"""
    K = np.array([[600.0, 0, cols / 2 - 0.5], [0, 600.0, rows / 2 - 0.5], [0, 0, 1]])
    P = line_cameras(n, BASE / 2)
    gray, _ = render(K, rows, cols, P, [("sphere", (0, 0, 2.7), 1.0), ("plane", (0, 0, 1), 3.0)], 16 * 1.78 / 600)
    return gray, K, P


def interior(o, max_disp):
    """the pixels at least window + the largest disparity away from every border (rule 3 wants all four taps inside, so a
    source's last row and column give no sample: a margin of the window alone does not do, even without vertical disparity)"""
    m = o.window + int(np.ceil(max_disp))
    mask = np.zeros((ROWS, COLS), bool)
    mask[m:ROWS - m, m:COLS - m] = True
    return mask


def step_errors(depth, truth, mask):
    e = np.abs(1 / depth[mask].astype(np.float64) - 1 / truth[mask]) / STEP
    return float(np.median(e)), float(np.percentile(e, 95))


def check_fronto(M, o):
    idx, d, s = M.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, o)
    mask = interior(o, 2 * BASE * 100 * plane_inv(16))
    wrong = int((idx[mask] != 16).sum())
    print(f"fronto-parallel plane: {wrong} of {int(mask.sum())} interior pixels off index 16, mean score {s[mask].mean():.4f}")
    assert mask.sum() > 1000 and (idx[mask] >= 0).all() and wrong <= 0.01 * mask.sum()
    return idx, d, s


def check_surface(M, o, truth, kind, bound):
    idx, d, s = M.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, o)
    mask = interior(o, 2 * BASE * 100 / truth[2].min()) & (idx >= 0)
    if kind == "sphere":  # the sphere's face, away from its limb (where the texture is squeezed below the wavelength bound)
        x, y = np.meshgrid(np.arange(COLS), np.arange(ROWS))
        mask &= (x - K0[0, 2]) ** 2 + (y - K0[1, 2]) ** 2 < 22 ** 2
    med, p95 = step_errors(d, truth[2], mask)
    print(f"{kind}: {int(mask.sum())} accepted interior pixels, |inverse depth error| median {med:.4f} p95 {p95:.4f} steps")
    assert mask.sum() > 500 and med <= bound[0] and p95 <= bound[1]
    return idx, d, s


def check_edge(M, o):
    """two fronto-parallel planes, the near one ending at an occluding edge: no fused point between them.  Run as the host
    mirror runs step 7, min_views 5 of 5 views (the reference's minImageNum): a window that straddles the edge is refined to a
    fraction of a hypothesis step off its plane (one step is 4 % of the near plane's depth, eps is 1 %), and only agreement
    of every view removes all of those.  At the ABI's default of 3, 57 of 4685 points lie 1 - 12 % off."""
    assert o.min_views == 5
    xyz, nrm, rgb = M.run(DMIN, DMAX, o)
    z = xyz[:, 2].astype(np.float64)
    near, far = 1 / plane_inv(20), 1 / plane_inv(10)
    off = np.minimum(np.abs(z - near) / near, np.abs(z - far) / far)
    print(f"occluding edge: {len(z)} points, {int((np.abs(z - near) < np.abs(z - far)).sum())} on the near plane, worst relative offset {off.max():.5f}")
    assert len(z) > 500 and (np.abs(z - near) < 0.01 * near).sum() > 100 and (np.abs(z - far) < 0.01 * far).sum() > 100
    assert off.max() <= o.eps
    return xyz, nrm, rgb


# ---------------------------------------------------------------- fusion on hand-made maps (shared with the GPU file)
FK = np.array([[8.0, 0, 3.5], [0, 8.0, 3.5], [0, 0, 1]])


def fusion_views(n, seed=3):
    """n views of 8 x 8, centres 0.25 apart on x, a plane at depth 2: one pixel of disparity per view, all dyadic, so that
    pixel (x, y) of view r lands exactly on column x + r - v of view v"""
    P = np.zeros((n, 3, 4))
    P[:, :, :3] = np.eye(3)
    P[:, 0, 3] = -0.25 * np.arange(n)
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, 8, 8)).astype(np.uint8), rng.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8), P


def fusion_expected(n, min_views, has_depth=None):
    """(view, row, column) of the points rule 7 keeps, in order, by counting columns"""
    has = has_depth if has_depth is not None else np.ones((n, 8, 8), bool)
    out = []
    for r in range(n):
        for y in range(8):
            for x in range(8):
                if not has[r, y, x]:
                    continue
                cons = [v for v in range(n) if v != r and 0 <= x + r - v < 8 and has[v, y, x + r - v]]
                if 1 + len(cons) >= min_views and all(v > r for v in cons):
                    out.append((r, y, x))
    return out


def check_fusion(make, ms_opts):
    """make(gray, K, poses, bgr, level) -> an Mvs-like object; ms_opts(**kw) -> its options"""
    for n in (3, 4, 5):
        gray, bgr, P = fusion_views(n)
        with make(gray, FK, P, None, 0) as M:
            for v in range(n):
                M.set_depthmap(v, np.full((8, 8), 2.0, np.float32))
            for mv in range(1, n + 2):  # every count from one below the smallest to one above the largest
                exp = fusion_expected(n, mv)
                xyz, nrm, rgb = M.fuse(ms_opts(min_views=mv))
                assert len(xyz) == len(exp), (n, mv)
                if not exp:
                    continue
                r, y, x = np.array(exp).T
                want = np.stack([(x - 3.5) / 8 * 2 + 0.25 * r, (y - 3.5) / 8 * 2, np.full(len(r), 2.0)], 1)
                assert np.array_equal(xyz, want.astype(np.float32))            # the order: view, row, column (all exact)
                assert np.array_equal(rgb, gray[r, y, x].astype(np.uint32) * 0x010101)
                c = np.stack([0.25 * r, 0 * r, 0 * r], 1) - want
                assert np.abs(nrm - c / np.linalg.norm(c, axis=1, keepdims=True)).max() < 1e-6
                if mv == n:  # the same surface in n views: view 0 alone emits it
                    assert (r == 0).all() and len(r) == 8 * (8 - (n - 1))
    gray, bgr, P = fusion_views(4)
    with make(gray, FK, P, bgr, 0) as M:
        has = np.ones((4, 8, 8), bool)
        has[2, 3:6] = False                                   # rows without depth in one view
        for v in range(4):
            M.set_depthmap(v, np.where(has[v], 2.0, 0.0).astype(np.float32))
        exp = fusion_expected(4, 3, has)
        xyz, nrm, rgb = M.fuse(ms_opts(min_views=3))
        r, y, x = np.array(exp).T
        assert len(xyz) == len(exp)
        b = bgr[r, y, x].astype(np.uint32)
        assert np.array_equal(rgb, (b[:, 2] << 16) | (b[:, 1] << 8) | b[:, 0])
        # eps: view 1 at 2.015625, a relative offset of exactly 2^-7 from the 2.0 the others predict in it
        d1 = np.full((8, 8), 2.015625, np.float32)
        for v in range(4):
            M.set_depthmap(v, d1 if v == 1 else np.full((8, 8), 2.0, np.float32))
        inside = M.fuse(ms_opts(min_views=4, eps=2.0 ** -7))[0]
        outside = M.fuse(ms_opts(min_views=4, eps=2.0 ** -7 - 1e-9))[0]
        assert len(inside) == 40 and (inside[:, 2] == 2.0).all() and len(outside) == 0


# ---------------------------------------------------------------- tests
def test_sample_units(ms):
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (9, 11)).astype(np.uint8)
    I = np.eye(3).reshape(9)
    s = lambda H, x, y: ms.mvs_sample(_p(img), 9, 11, _p(np.ascontiguousarray(H, np.float64)), x, y)
    for y in range(8):
        for x in range(10):
            assert s(I, x, y) == 16 * int(img[y, x])                       # integer coordinates: 16 I
    assert s(I, 10, 3) == -1 and s(I, 3, 8) == -1                         # the right / lower tap is off the image
    sh = lambda dx, dy: np.array([1, 0, dx, 0, 1, dy, 0, 0, 1.0])
    assert s(sh(-0.25, 0), 0, 0) == -1 and s(sh(0, -1e-9), 2, 0) == -1   # taps left of / above it
    assert s(sh(31.5 / 32, 0), 2, 4) == 16 * int(img[4, 3])              # fraction 31.5/32 rounds to weight 32: a carry
    assert s(sh(31.5 / 32, 0), 9, 4) == -1                                # ... and the carried sample needs its own taps
    assert s(sh(0, 31.5 / 32), 2, 7) == -1
    a, b, c, d = (int(v) for v in (img[4, 2], img[4, 3], img[5, 2], img[5, 3]))
    for fx, fy in ((0.5, 0.0), (0.25, 0.75), (15.4 / 32, 0.49 / 32), (15.5 / 32, 0.5 / 32)):
        wx, wy = int(np.floor(fx * 32 + 0.5)), int(np.floor(fy * 32 + 0.5))
        want = ((a * (32 - wx) + b * wx) * (32 - wy) + (c * (32 - wx) + d * wx) * wy + 32) >> 6
        assert s(sh(fx, fy), 2, 4) == want
    assert s(np.array([1, 0, 0, 0, 1, 0, 0, 0, -1.0]), 2, 2) == -1        # behind the source
    white = np.full((4, 4), 255, np.uint8)
    half = sh(0.5, 0.5)
    assert ms.mvs_sample(_p(white), 4, 4, _p(half), 1, 1) == 4080


def test_score_units(ms):
    rng = np.random.RandomState(1)
    out = C.c_double(0)

    def ncc(r, q, side):
        r16, q16 = np.ascontiguousarray(r, np.uint16), np.ascontiguousarray(q, np.uint16)
        return ms.mvs_ncc_window(_p(r16), _p(q16), side, C.addressof(out)), out.value

    for side in (3, 7, 15):
        r = 16 * rng.randint(0, 100, (side, side))
        ok, v = ncc(r, 2 * r + 48, side)                                  # a ref + b, no clipping
        assert ok and v >= 1 - 1e-12
        ok, v = ncc(r, 4080 - 2 * r, side)
        assert ok and v <= -1 + 1e-12
        q = 16 * rng.randint(0, 256, (side, side))
        ok, v = ncc(r, q, side)
        want = np.corrcoef(r.ravel(), q.ravel())[0, 1]
        assert ok and abs(v - want) < 1e-12
        ok, v = ncc(r, np.full((side, side), 1600), side)                 # a constant window: invalid, never NaN
        assert not ok
        ok, v = ncc(np.full((side, side), 4080), q, side)
        assert not ok
        q[side // 2, 0] = 0xFFFF
        assert not ncc(r, q, side)[0]
    full = np.full((15, 15), 4080)                                        # the largest sums of the largest window fit u32
    full[0, 0] = 0
    ok, v = ncc(full, full, 15)
    assert ok and abs(v - 1) < 1e-12


def test_pyramid_and_sources(ms):
    rng = np.random.RandomState(2)
    g = rng.randint(0, 256, (3, 45, 71)).astype(np.uint8)
    b = rng.randint(0, 256, (3, 45, 71, 3)).astype(np.uint8)
    P = line_cameras(3)
    with StubMvs(ms, g, K0, P, b, level=1) as M:                           # level 1 of a 71 x 45 image: 35 x 22
        assert (M.rows, M.cols) == (22, 35)
        assert np.array_equal(M.K, level_K(K0, 1))
        for v in range(3):
            lg, lb = M.level_image(v)
            q = g[v, :44, :70].astype(int)
            assert np.array_equal(lg, (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2)
            q = b[v, :44, :70].astype(int)
            assert np.array_equal(lb, (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2)
    with StubMvs(ms, g, K0, P, None, level=2) as M:
        assert (M.rows, M.cols) == (11, 17)
    P = line_cameras(6)
    P[:, 0, 3] = -np.array([0.0, 1.0, 2.0, 4.0, 3.0, -1.0])                # centres; 1 has 0 and 2 at the same distance
    src = np.zeros(8, np.int32)
    assert ms.mvs_sources(_p(P), 6, 1, 4, _p(src)) == 4 and list(src[:4]) == [0, 2, 4, 5]
    assert ms.mvs_sources(_p(P), 6, 3, 8, _p(src)) == 5 and list(src[:5]) == [4, 2, 1, 0, 5]


def test_homography_maps_the_plane(ms):
    """rule 2 against a direct projection: a point of plane k seen from the reference lands where H says"""
    rng = np.random.RandomState(4)
    P = line_cameras(3)
    for v in range(3):  # general rotations and translations
        w = rng.normal(0, 0.1, 3)
        th = np.linalg.norm(w)
        kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        P[v, :, :3] = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
        P[v, :, 3] += rng.normal(0, 0.05, 3)
    src = np.array([0, 2], np.int32)
    H = np.zeros((D, 2, 3, 3))
    ms.mvs_homographies(_p(K0), _p(P), 1, 2, _p(src), D, DMIN, DMAX, _p(H))
    for k in (0, 7, 32):
        for s in (0, 1):
            for x, y in ((0, 0), (40, 20), (95, 63)):
                Xc = np.linalg.inv(K0) @ [x, y, 1] / plane_inv(k)
                X = P[1, :, :3].T @ (Xc - P[1, :, 3])
                p = K0 @ (P[src[s], :, :3] @ X + P[src[s], :, 3])
                q = H[k, s] @ [x, y, 1]
                assert np.allclose(p[:2] / p[2], q[:2] / q[2], atol=1e-9) and q[2] > 0


def test_fronto_parallel_plane(ms):
    gray, depth, K, P = scene("fronto")
    with StubMvs(ms, gray, K, P, level=0) as M:
        check_fronto(M, opts(ms, n_planes=D))


def test_slanted_plane(ms):
    gray, depth, K, P = scene("slanted")
    with StubMvs(ms, gray, K, P, level=0) as M:
        check_surface(M, opts(ms, n_planes=D), depth, "slanted plane", SLANT_BOUND)


def test_sphere(ms):
    gray, depth, K, P = scene("sphere")
    with StubMvs(ms, gray, K, P, level=0) as M:
        check_surface(M, opts(ms, n_planes=D), depth, "sphere", SPHERE_BOUND)


def test_fusion_on_hand_made_maps(ms):
    check_fusion(lambda g, K, P, b, level: StubMvs(ms, g, K, P, b, level), lambda **kw: opts(ms, **kw))


def test_occluding_edge(ms):
    gray, depth, K, P = scene("edge")
    with StubMvs(ms, gray, K, P, level=0) as M:
        check_edge(M, opts(ms, n_planes=D, min_views=5))


def test_level_one_run(ms):
    """the fronto-parallel scene rendered at twice the size and run at level 1: the same plane, index 16"""
    gray, depth, K, P = scene("fronto", level=1)
    with StubMvs(ms, gray, K, P, level=1) as M:
        assert (M.rows, M.cols) == (ROWS, COLS) and np.array_equal(M.K, K0)
        check_fronto(M, opts(ms, n_planes=D))


def test_edge_cases(ms):
    gray, depth, K, P = scene("fronto")
    with StubMvs(ms, gray, K, P, level=0) as M:
        idx, d, s = M.depthmap(2, [1, 3], DMIN, DMAX, opts(ms, n_planes=3))           # D = 3
        assert set(np.unique(idx)) <= {-1, 0, 1, 2} and ((d > 0) == (idx >= 0)).all() and np.isfinite(d).all()
        idx, d, s = M.depthmap(2, [3], DMIN, DMAX, opts(ms, n_planes=D, n_best=1))     # one source, best of one
        m = interior(opts(ms), 12)
        assert (idx[m] == 16).mean() > 0.99
        idx, d, s = M.depthmap(2, [3], DMIN, DMAX, opts(ms, n_planes=D, n_best=2))     # n_best above the sources: nothing
        assert (idx == -1).all() and (d == 0).all() and (s == 0).all()
        idx, d, s = M.depthmap(2, [1, 3], DMIN, DMAX, opts(ms, n_planes=D, window=1))
        assert (idx[1:-1, 30:-30] >= 0).mean() > 0.5 and (idx[0] == -1).all() and (idx[:, 0] == -1).all()
        idx, d, s = M.depthmap(0, [1, 2], 0.05, 0.06, opts(ms, n_planes=D))            # planes no source sees the view on
        assert (idx == -1).all()
    black = gray.copy()
    black[2] = 0
    with StubMvs(ms, black, K, P, level=0) as M:                                       # an all-black view: no depth in it
        idx, d, s = M.depthmap(2, [1, 3], DMIN, DMAX, opts(ms, n_planes=D))
        assert (idx == -1).all() and np.isfinite(s).all()
        idx, d, s = M.depthmap(1, [0, 2], DMIN, DMAX, opts(ms, n_planes=D, n_best=1))   # ... and none through it as a source
        assert np.isfinite(s).all() and (idx[interior(opts(ms), 12)] == 16).mean() > 0.99
        xyz, nrm, rgb = M.run(DMIN, DMAX, opts(ms, n_planes=D, min_views=2))
        assert len(xyz) > 0 and np.isfinite(xyz).all() and np.isfinite(nrm).all()


def test_argument_errors(ms):
    gray, depth, K, P = scene("fronto")
    for bad in (lambda: StubMvs(ms, gray[:1], K, P[:1], level=0), lambda: StubMvs(ms, gray[:, :1, :1], K, P, level=1),
                lambda: StubMvs(ms, gray[:, :0], K, P, level=0)):
        with pytest.raises(ValueError, match="status -3"):
            bad()
    with StubMvs(ms, gray, K, P, level=0) as M:
        check_refusals(M, lambda **kw: opts(ms, **kw))


def check_refusals(M, mk):
    for src, lo, hi, kw in (([1, 3], 2.0, 2.0, {}), ([1, 3], 3.0, 2.0, {}), ([1, 3], 0.0, 2.0, {}), ([1, 3], -1.0, 2.0, {}),
                            ([1, 3], 1.0, np.inf, {}), ([1, 3], 1.0, 8.0, dict(n_planes=2)), ([1, 3], 1.0, 8.0, dict(n_planes=257)),
                            ([1, 2], 1.0, 8.0, {}), ([1, 1], 1.0, 8.0, {}), ([1, 5], 1.0, 8.0, {}), ([], 1.0, 8.0, {}),
                            ([1, 3], 1.0, 8.0, dict(window=8)), ([1, 3], 1.0, 8.0, dict(window=0)), ([1, 3], 1.0, 8.0, dict(n_best=0)),
                            ([1, 3], 1.0, 8.0, dict(n_best=5)), ([1, 3], 1.0, 8.0, dict(eps=-0.1)), ([1, 3], 1.0, 8.0, dict(ncc_min=2.0))):
        with pytest.raises(Exception, match="status -3"):
            M.depthmap(2, src, lo, hi, mk(**kw))
    with pytest.raises(Exception, match="status -3"):
        M.depthmap(7, [1, 3], 1.0, 8.0, mk())
    with pytest.raises(Exception, match="status -3"):
        M.run([1, 1, 1, 0, 1], 8.0, mk())
    with pytest.raises(Exception, match="status -3"):
        M.run(1.0, 8.0, mk(n_src=9))
    with pytest.raises(Exception, match="status -3"):
        M.fuse(mk(min_views=0))
