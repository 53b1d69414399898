"""Two device-resident clouds of cloud.py meet (include/sfmhip.h, sfmhip_cloud_nearest / _register / _transform / _concat;
DESIGN.md f-17): the nearest target point of every source point, rigid and similarity ICP around that search, and the two
calls that keep the result on the device.  A similarity registration against a metric cloud is where the `scale` the
dendrometry takes comes from.

`nearest(target, source, T, max_dist)` returns (idx, d2) per source point; `icp(target, source, init, **opts)` a
RegisterResult (T, iterations, pairs, converged, flags, mse; with return_pairs also the idx array); `transform(cloud, T)` and
`concat(a, b)` new Clouds born on the device.  `Transform` carries x -> scale R x + t with host-only helpers (matrix, inverse,
compose).  Parity with PCL is UNPINNED."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .cloud import Cloud

FEW, DEGENERATE = 1, 2                       # bits of RegisterResult.flags
LIMIT, FIXED_POINT, EPS = 0, 1, 2            # RegisterResult.converged


class Transform(C.Structure):
    """x -> scale R x + t (R row-major, all f64)."""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("scale", C.c_double)]

    @classmethod
    def make(cls, R=None, t=None, scale=1.0):
        T = cls()
        T.R = (C.c_double * 9)(*np.asarray(np.eye(3) if R is None else R, np.float64).reshape(9))
        T.t = (C.c_double * 3)(*np.asarray(np.zeros(3) if t is None else t, np.float64).reshape(3))
        T.scale = float(scale)
        return T

    @classmethod
    def from_matrix(cls, M):
        """From a 4 x 4 similarity [s R | t]: scale = cbrt(det(s R))."""
        M = np.asarray(M, np.float64)
        s = float(np.cbrt(np.linalg.det(M[:3, :3])))
        return cls.make(M[:3, :3] / s, M[:3, 3], s)

    def rotation(self):
        return np.array(self.R, np.float64).reshape(3, 3)

    def translation(self):
        return np.array(self.t, np.float64)

    def matrix(self):
        """The 4 x 4 [scale R | t; 0 0 0 1]."""
        M = np.eye(4)
        M[:3, :3] = self.scale * self.rotation()
        M[:3, 3] = self.translation()
        return M

    def inverse(self):
        R = self.rotation().T
        return Transform.make(R, -(R @ self.translation()) / self.scale, 1.0 / self.scale)

    def compose(self, first):
        """The transform that applies `first`, then this one."""
        R = self.rotation() @ first.rotation()
        return Transform.make(R, self.scale * (self.rotation() @ first.translation()) + self.translation(), self.scale * first.scale)

    def apply(self, xyz):
        """Rule 2 in numpy: float32 [n, 3] of the f64 image (what `transform` writes for the finite points)."""
        p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
        R, out = self.rotation(), np.empty((len(p), 3), np.float64)
        with np.errstate(all="ignore"):
            for r in range(3):
                out[:, r] = self.scale * ((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + self.t[r]
            return out.astype(np.float32)


class RegisterOpts(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("with_scale", C.c_int32), ("min_pairs", C.c_int32), ("reserved", C.c_int32),
                ("max_dist", C.c_double), ("eps", C.c_double)]


class RegisterResult(C.Structure):
    _fields_ = [("T", Transform), ("iterations", C.c_int32), ("pairs", C.c_int32), ("converged", C.c_int32), ("flags", C.c_int32),
                ("mse", C.c_double)]
    idx = None   # the pairs under T, with icp(return_pairs=True)


def set_opts(o, **kw):
    for k, v in kw.items():
        if not hasattr(o, k) or k == "reserved":
            raise TypeError(f"no option {k}")
        setattr(o, k, v)
    return o


def default_opts(**kw):
    """50 iterations, rigid, 3 pairs, max_dist +inf, eps off; keyword arguments override fields."""
    o = RegisterOpts()
    _lib.lib().sfmhip_register_default_opts(C.byref(o))
    return set_opts(o, **kw)


def _ref(T):
    return None if T is None else C.byref(T)


def nearest(target, source, T=None, max_dist=math.inf):
    """(idx int32 [n_src], d2 float32 [n_src]): the nearest finite target point of every source point moved by T, by (d2, index);
    idx -1 where d2 > (float)(max_dist ** 2) (d2 stays) or the point has no image (d2 +inf)."""
    n1 = max(source.n, 1)
    idx, d2 = np.empty(n1, np.int32), np.empty(n1, np.float32)
    _lib.check(_lib.lib().sfmhip_cloud_nearest(target.h, source.h, _ref(T), float(max_dist), idx.ctypes.data, d2.ctypes.data),
               "sfmhip_cloud_nearest")
    return idx[:source.n].copy(), d2[:source.n].copy()


def icp(target, source, init=None, return_pairs=False, opts=None, **kw):
    """RegisterResult of the ICP that brings `source` onto `target` from `init` (identity without); options by keyword
    (max_iters, with_scale, min_pairs, max_dist, eps) or as a RegisterOpts."""
    o = set_opts(opts, **kw) if opts is not None else default_opts(**kw)
    res = RegisterResult()
    idx = np.empty(max(source.n, 1), np.int32) if return_pairs else None
    _lib.check(_lib.lib().sfmhip_cloud_register(target.h, source.h, C.byref(o), _ref(init), C.byref(res),
                                                None if idx is None else idx.ctypes.data), "sfmhip_cloud_register")
    if return_pairs:
        res.idx = idx[:source.n].copy()
    return res


def transform(cloud, T):
    """A new device cloud of the points moved by T (rule 2; a non-finite point stays), never on the host."""
    h = C.c_void_p()
    _lib.check(_lib.lib().sfmhip_cloud_transform(cloud.h, C.byref(T), C.byref(h)), "sfmhip_cloud_transform")
    return Cloud.from_handle(h, cloud.ctx)


def concat(a, b):
    """A new device cloud of a's points, then b's, copied device to device."""
    h = C.c_void_p()
    _lib.check(_lib.lib().sfmhip_cloud_concat(a.h, b.h, C.byref(h)), "sfmhip_cloud_concat")
    return Cloud.from_handle(h, a.ctx)


def last_timing(target):
    """ms of the last icp with this target, summed over its iterations, with Context.set_timing on: search, sums, update; and
    the iterations."""
    ms, it = (C.c_double * 3)(), C.c_int32(0)
    _lib.check(_lib.lib().sfmhip_cloud_register_last_timing(target.h, ms, C.byref(it)), "sfmhip_cloud_register_last_timing")
    return dict(search=ms[0], sums=ms[1], update=ms[2], iterations=it.value)
