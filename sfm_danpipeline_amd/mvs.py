"""map3D's step 7 on the GPU (the reference shells out to pmvs2, src/Sfm.cpp:62-67): plane-sweep depth maps per view, then
cross-view consistency fusion into one coloured, oriented cloud (include/sfmhip.h, sfmhip_mvs_*; csrc/mvs.hip).

`densify(gray, K, poses, dmin, dmax)` returns (xyz [m, 3] float32, normals [m, 3] float32, rgb [m] uint32 0x00RRGGBB);
`Mvs` is the staged form: depthmap(ref, src, dmin, dmax), set_depthmap, fuse, run.  Parity with pmvs2 is UNPINNED
(DESIGN.md f-10): depth-map fusion for its patch expansion, camera-facing normals for its patch normals.

`dist` (k1 k2 p1 p2 k3 of the calibration file) on either form: the views are undistorted on the device into the pinhole
camera of the same K before anything else (undistort.py), `Mvs.valid()` is the mask of the working level and
a reference pixel whose window touches an invalid pixel gets no depth."""
import ctypes as C

import numpy as np

from . import _lib


class MvsOpts(C.Structure):
    _fields_ = [("n_planes", C.c_int32), ("window", C.c_int32), ("n_src", C.c_int32), ("n_best", C.c_int32),
                ("min_views", C.c_int32), ("pad", C.c_int32), ("ncc_min", C.c_double), ("eps", C.c_double),
                ("var_min", C.c_double)]


def default_opts(**kw):
    """128 planes, window 3, 4 sources, best 2, min_views 3, ncc_min 0.7, eps 0.01; keyword arguments override fields."""
    o = MvsOpts()
    _lib.lib().sfmhip_mvs_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no option {k}")
        setattr(o, k, v)
    return o


def _p(a):
    return a.ctypes.data


def image_pointers(images, ch):
    """(contiguous uint8 arrays, a C array of pointers to them) of n images [rows, cols(, 3)]"""
    keep = [np.ascontiguousarray(im, np.uint8) for im in images]
    for im in keep:
        if im.shape != keep[0].shape or im.ndim != (2 if ch == 1 else 3) or (ch == 3 and im.shape[2] != 3):
            raise ValueError("images must share one shape, [rows, cols] gray or [rows, cols, 3] BGR")
    return keep, (C.c_void_p * len(keep))(*[_p(im) for im in keep])


class Mvs:
    """Views on the device at pyramid level `level`: gray [n, rows, cols] uint8 (bgr [n, rows, cols, 3] optional), one K
    [3, 3], poses [n, 3, 4] = [R | t]; dist: None for pinhole views, else the five distortion coefficients."""

    def __init__(self, gray, K, poses, bgr=None, level=1, ctx=None, dist=None):
        self.ctx = ctx or _lib.default_context()
        g, gp = image_pointers(gray, 1)
        bp = None
        if bgr is not None:
            b, bp = image_pointers(bgr, 3)
            if len(b) != len(g) or b[0].shape[:2] != g[0].shape:
                raise ValueError("bgr must match gray")
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1)
        if len(poses) != 12 * len(g):
            raise ValueError("poses must be [n, 3, 4]")
        rows, cols = g[0].shape if g else (0, 0)
        self.h = C.c_void_p()
        if dist is None:
            _lib.check(_lib.lib().sfmhip_mvs_create(self.ctx.h, len(g), rows, cols, gp, bp, _p(K), _p(poses), int(level), C.byref(self.h)),
                       "sfmhip_mvs_create")
        else:
            dist = np.ascontiguousarray(dist, np.float64).reshape(-1)
            if len(dist) != 5:
                raise ValueError("dist must be the five coefficients k1 k2 p1 p2 k3")
            _lib.check(_lib.lib().sfmhip_mvs_create_distorted(self.ctx.h, len(g), rows, cols, gp, bp, _p(K), _p(dist), _p(poses), int(level),
                                                              C.byref(self.h)), "sfmhip_mvs_create_distorted")
        self.n, self.colour = len(g), bgr is not None
        r, c, k = C.c_int32(0), C.c_int32(0), np.zeros(9)
        _lib.check(_lib.lib().sfmhip_mvs_level(self.h, C.byref(r), C.byref(c), _p(k), -1, None, None), "sfmhip_mvs_level")
        self.rows, self.cols, self.K = r.value, c.value, k.reshape(3, 3)

    def level_image(self, view):
        """(gray [rows, cols], bgr [rows, cols, 3] or None) of one view at the working level"""
        g = np.zeros((self.rows, self.cols), np.uint8)
        b = np.zeros((self.rows, self.cols, 3), np.uint8) if self.colour else None
        _lib.check(_lib.lib().sfmhip_mvs_level(self.h, None, None, None, int(view), _p(g), _p(b) if self.colour else None),
                   "sfmhip_mvs_level")
        return g, b

    def valid(self):
        """the mask of the working level [rows, cols] uint8: all ones without `dist`"""
        m = np.zeros((self.rows, self.cols), np.uint8)
        _lib.check(_lib.lib().sfmhip_mvs_valid(self.h, _p(m)), "sfmhip_mvs_valid")
        return m

    def depthmap(self, ref, src, dmin, dmax, opts=None):
        """(winner index int32, depth float32, score float32), each [rows, cols]; the depth map stays on the handle"""
        opts = opts or default_opts()
        src = np.ascontiguousarray(src, np.int32).reshape(-1)
        idx, d, s = (np.zeros((self.rows, self.cols), t) for t in (np.int32, np.float32, np.float32))
        _lib.check(_lib.lib().sfmhip_mvs_depthmap(self.h, int(ref), len(src), _p(src), float(dmin), float(dmax), C.byref(opts), _p(idx), _p(d),
                                                  _p(s)), "sfmhip_mvs_depthmap")
        return idx, d, s

    def set_depthmap(self, view, depth):
        d = np.ascontiguousarray(depth, np.float32)
        if d.shape != (self.rows, self.cols):
            raise ValueError("depth must be [rows, cols] of the working level")
        _lib.check(_lib.lib().sfmhip_mvs_set_depthmap(self.h, int(view), _p(d)), "sfmhip_mvs_set_depthmap")

    def _points(self, m):
        xyz, nrm, rgb = np.zeros((max(m, 1), 3), np.float32), np.zeros((max(m, 1), 3), np.float32), np.zeros(max(m, 1), np.uint32)
        _lib.check(_lib.lib().sfmhip_mvs_download(self.h, _p(xyz), _p(nrm), _p(rgb)), "sfmhip_mvs_download")
        return xyz[:m].copy(), nrm[:m].copy(), rgb[:m].copy()

    def fuse(self, opts=None):
        opts, m = opts or default_opts(), C.c_int32(0)
        _lib.check(_lib.lib().sfmhip_mvs_fuse(self.h, C.byref(opts), C.byref(m)), "sfmhip_mvs_fuse")
        return self._points(m.value)

    def run(self, dmin, dmax, opts=None):
        opts, m = opts or default_opts(), C.c_int32(0)
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(dmin, np.float64), (self.n,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(dmax, np.float64), (self.n,)))
        _lib.check(_lib.lib().sfmhip_mvs_run(self.h, _p(lo), _p(hi), C.byref(opts), C.byref(m)), "sfmhip_mvs_run")
        return self._points(m.value)

    def last_timing(self):
        """ms of the last run / fuse: depth maps (timed apart only under Context.set_timing), fusion, whole call"""
        ms = np.zeros(3, np.float64)
        _lib.check(_lib.lib().sfmhip_mvs_last_timing(self.h, _p(ms)), "sfmhip_mvs_last_timing")
        return dict(zip(("depthmaps", "fusion", "total"), map(float, ms)))

    def close(self):
        if self.h:
            _lib.lib().sfmhip_mvs_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def densify(gray, K, poses, dmin, dmax, bgr=None, level=1, opts=None, ctx=None, dist=None):
    """Step 7 in one call: (xyz, normals, rgb) of the fused cloud."""
    with Mvs(gray, K, poses, bgr=bgr, level=level, ctx=ctx, dist=dist) as m:
        return m.run(dmin, dmax, opts)
