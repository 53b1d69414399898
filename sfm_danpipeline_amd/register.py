"""Two device-resident clouds of cloud.py meet (include/sfmhip.h, sfmhip_cloud_nearest / _register / _transform / _concat;
DESIGN.md f-17): the nearest target point of every source point, rigid and similarity ICP around that search, and the two
calls that keep the result on the device.  A similarity registration against a metric cloud is where the `scale` the
dendrometry takes comes from.

`nearest(target, source, T, max_dist)` returns (idx, d2) per source point; `icp(target, source, init, **opts)` a
RegisterResult (T, iterations, pairs, converged, flags, mse; with return_pairs also the idx array); `transform(cloud, T)` and
`concat(a, b)` new Clouds born on the device.  `Transform` carries x -> scale R x + t with host-only helpers (matrix, inverse,
compose).  Parity with PCL is UNPINNED.

The coarse alignment needs no `init`: `icp_batch(target, source, inits, **opts)` runs many starts in one
lock-step loop (each result is `icp`'s from that start, byte for byte), `align_vote(target, source, target_frame,
source_frame, **opts)` lists candidate poses of two levelled clouds by a height-keyed vote, `align(...)` runs the batch from
them and returns the winner, whose `.reg.T` is the `init` for `icp` on the full clouds.  `Frame.from_ground(result)` makes
a frame of a ground-plane result; `scale_guess(stats)` is the ratio of the two clouds' heights.

The second entry adds rejectors and a second estimator: `icp_ex(target, source, normals, init, **opts)` takes
every option of IcpOpts (metric, trim, one_to_one, ...) and returns an IcpResult; `icp_plane(...)` is the point-to-plane
metric with the target's normals (computed by `Cloud.normals(k)` when not given); `icp_ex_batch` / `icp_plane_batch` run many
starts in one lock-step loop, each result the single call's from that start, byte for byte."""
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


# ---------------------------------------------------------------- the coarse alignment (f-18)
EMPTY, NO_WINNER = 1, 2                      # bits of AlignResult.flags (AlignStats.flags: EMPTY only)


class Frame(C.Structure):
    """A levelled frame: the ground plane's up, north and offset (up . p = offset on the ground)."""
    _fields_ = [("up", C.c_double * 3), ("north", C.c_double * 3), ("offset", C.c_double)]

    @classmethod
    def make(cls, up=(0, 0, 1), north=(0, 1, 0), offset=0.0):
        f = cls()
        f.up, f.north, f.offset = (C.c_double * 3)(*up), (C.c_double * 3)(*north), float(offset)
        return f

    @classmethod
    def from_ground(cls, ground):
        """Of a GroundResult that has a plane (sfmhip_frame_from_ground)."""
        f = cls()
        _lib.check(_lib.lib().sfmhip_frame_from_ground(C.byref(ground), C.byref(f)), "sfmhip_frame_from_ground")
        return f


class AlignOpts(C.Structure):
    _fields_ = [("scale_lo", C.c_double), ("scale_hi", C.c_double), ("clear_rel", C.c_double), ("h_tol", C.c_double),
                ("window_rel", C.c_double), ("icp_dist_bins", C.c_double), ("n_scale", C.c_int32), ("n_yaw", C.c_int32),
                ("bins", C.c_int32), ("src_samples", C.c_int32), ("tgt_samples", C.c_int32), ("n_cand", C.c_int32),
                ("icp_max_iters", C.c_int32), ("reserved", C.c_int32)]


class AlignCandidate(C.Structure):
    _fields_ = [("T", Transform), ("votes", C.c_int32), ("k", C.c_int32), ("m", C.c_int32), ("bin", C.c_int32)]


class AlignStats(C.Structure):
    _fields_ = [("hmax_src", C.c_double), ("hmax_tgt", C.c_double), ("w", C.c_double), ("window", C.c_double),
                ("n_above_src", C.c_int32), ("n_above_tgt", C.c_int32), ("n_src", C.c_int32), ("n_tgt", C.c_int32),
                ("n_hyp", C.c_int32), ("flags", C.c_int32)]


class AlignResult(C.Structure):
    _fields_ = [("reg", RegisterResult), ("cand", AlignCandidate), ("cand_index", C.c_int32), ("n_same", C.c_int32),
                ("n_cand", C.c_int32), ("flags", C.c_int32), ("stats", AlignStats)]


def align_default_opts(**kw):
    """The table of f-18 rule V1; scale_lo, scale_hi and h_tol have no default and must be given."""
    o = AlignOpts()
    _lib.lib().sfmhip_align_default_opts(C.byref(o))
    return set_opts(o, **kw)


def icp_batch(target, source, inits, return_pairs=False, opts=None, **kw):
    """A list of RegisterResult, one per Transform of `inits`: what `icp` returns from that start, from one lock-step loop
    (with return_pairs each carries its idx row)."""
    o = set_opts(opts, **kw) if opts is not None else default_opts(**kw)
    n = len(inits)
    starts = (Transform * max(n, 1))(*inits)
    res = (RegisterResult * max(n, 1))()
    idx = np.empty((max(n, 1), max(source.n, 1)), np.int32) if return_pairs else None   # (rows of source.n entries when it is > 0)
    _lib.check(_lib.lib().sfmhip_cloud_register_batch(target.h, source.h, C.byref(o), starts, n, res,
                                                      None if idx is None else idx.ctypes.data), "sfmhip_cloud_register_batch")
    out = []
    for b in range(n):
        r = RegisterResult.from_buffer_copy(res[b])
        if return_pairs:
            r.idx = idx[b, :source.n].copy()
        out.append(r)
    return out


def align_vote(target, source, target_frame, source_frame, opts=None, **kw):
    """(candidates, stats): the first n_cand poses of the vote as AlignCandidate, best first, and the AlignStats."""
    o = set_opts(opts, **kw) if opts is not None else align_default_opts(**kw)
    cands, n, stats = (AlignCandidate * max(int(o.n_cand), 1))(), C.c_int32(0), AlignStats()
    _lib.check(_lib.lib().sfmhip_cloud_align_vote(target.h, source.h, C.byref(target_frame), C.byref(source_frame), C.byref(o), cands,
                                                  C.byref(n), C.byref(stats)), "sfmhip_cloud_align_vote")
    return [AlignCandidate.from_buffer_copy(cands[i]) for i in range(n.value)], stats


def align(target, source, target_frame, source_frame, opts=None, **kw):
    """AlignResult: the vote, ICP from every candidate, the winner (reg.T: the `init` for `icp` on the full clouds)."""
    o = set_opts(opts, **kw) if opts is not None else align_default_opts(**kw)
    out = AlignResult()
    _lib.check(_lib.lib().sfmhip_cloud_align(target.h, source.h, C.byref(target_frame), C.byref(source_frame), C.byref(o), C.byref(out)),
               "sfmhip_cloud_align")
    return out


def scale_guess(stats):
    """hmax of the target over hmax of the source: the scale when both clouds show the same tallest point above their ground."""
    return stats.hmax_tgt / stats.hmax_src


def align_last_timing(target):
    """Host-clock ms of the last align_vote / align with this target: vote, batch ICP, the whole call."""
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().sfmhip_cloud_align_last_timing(target.h, ms), "sfmhip_cloud_align_last_timing")
    return dict(vote=ms[0], icp=ms[1], total=ms[2])


def batch_last_timing(target):
    """As last_timing, of the last icp_batch with this target; iterations: those of its longest problem."""
    ms, it = (C.c_double * 3)(), C.c_int32(0)
    _lib.check(_lib.lib().sfmhip_cloud_register_batch_last_timing(target.h, ms, C.byref(it)), "sfmhip_cloud_register_batch_last_timing")
    return dict(search=ms[0], sums=ms[1], update=ms[2], iterations=it.value)


def last_timing(target):
    """ms of the last icp with this target, summed over its iterations, with Context.set_timing on: search, sums, update; and
    the iterations."""
    ms, it = (C.c_double * 3)(), C.c_int32(0)
    _lib.check(_lib.lib().sfmhip_cloud_register_last_timing(target.h, ms, C.byref(it)), "sfmhip_cloud_register_last_timing")
    return dict(search=ms[0], sums=ms[1], update=ms[2], iterations=it.value)


# ---------------------------------------------------------------- point-to-plane, trimmed and one-to-one ICP (f-22)
POINT, PLANE = 0, 1                          # IcpOpts.metric
PLANE_EPS = 1e-9                             # icp_plane's default eps (metric 1 needs one)


class IcpOpts(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("with_scale", C.c_int32), ("min_pairs", C.c_int32), ("metric", C.c_int32),
                ("one_to_one", C.c_int32), ("normal_stride", C.c_int32), ("max_dist", C.c_double), ("eps", C.c_double),
                ("trim", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("T", Transform), ("iterations", C.c_int32), ("pairs", C.c_int32), ("converged", C.c_int32), ("flags", C.c_int32),
                ("mse", C.c_double), ("plane_mse", C.c_double), ("trim_d2", C.c_double)]
    idx = None   # the kept pairs under T, with return_pairs=True


def icp_default_opts(**kw):
    """f-17's defaults, metric 0, no rejector (trim 1, one_to_one 0), normal_stride 4; keyword arguments override fields."""
    o = IcpOpts()
    _lib.lib().sfmhip_icp_default_opts(C.byref(o))
    return set_opts(o, **kw)


def plane_opts(kw):
    """icp_plane's options: metric 1, eps 1e-9 and min_pairs 6 (7 with scale) unless given."""
    kw = dict(kw)
    kw.setdefault("eps", PLANE_EPS)
    kw.setdefault("min_pairs", 7 if kw.get("with_scale") else 6)
    kw["metric"] = PLANE
    return kw


def _normals(target, normals, o, k):
    """The host array of the target's normals and its stride written into o (None for metric 0 without normals)."""
    if normals is None:
        if o.metric != PLANE:
            return None
        from .cloud import K_NORMALS
        normals = target.normals(K_NORMALS if k is None else k)
    normals = np.ascontiguousarray(normals, np.float32)
    if normals.ndim != 2 or normals.shape[0] != target.n or normals.shape[1] not in (3, 4):
        raise ValueError("normals: one row of 3 or 4 floats per target point")
    o.normal_stride = normals.shape[1]
    return normals


def icp_ex(target, source, normals=None, init=None, return_pairs=False, opts=None, k=None, **kw):
    """IcpResult of sfmhip_cloud_register_icp: options by keyword (every field of IcpOpts) or as an IcpOpts; `normals` [n_target,
    3 or 4] float32, or None (metric 1 then computes them with target.normals(k))."""
    o = set_opts(opts, **kw) if opts is not None else icp_default_opts(**kw)
    nrm = _normals(target, normals, o, k)
    res = IcpResult()
    idx = np.empty(max(source.n, 1), np.int32) if return_pairs else None
    _lib.check(_lib.lib().sfmhip_cloud_register_icp(target.h, source.h, None if nrm is None else nrm.ctypes.data, C.byref(o), _ref(init),
                                                    C.byref(res), None if idx is None else idx.ctypes.data), "sfmhip_cloud_register_icp")
    if return_pairs:
        res.idx = idx[:source.n].copy()
    return res


def icp_ex_batch(target, source, inits, normals=None, return_pairs=False, opts=None, k=None, **kw):
    """A list of IcpResult, one per Transform of `inits`: what `icp_ex` returns from that start (with return_pairs its idx row)."""
    o = set_opts(opts, **kw) if opts is not None else icp_default_opts(**kw)
    nrm = _normals(target, normals, o, k)
    n = len(inits)
    starts = (Transform * max(n, 1))(*inits)
    res = (IcpResult * max(n, 1))()
    idx = np.empty((max(n, 1), max(source.n, 1)), np.int32) if return_pairs else None
    _lib.check(_lib.lib().sfmhip_cloud_register_icp_batch(target.h, source.h, None if nrm is None else nrm.ctypes.data, C.byref(o), starts, n,
                                                          res, None if idx is None else idx.ctypes.data), "sfmhip_cloud_register_icp_batch")
    out = []
    for b in range(n):
        r = IcpResult.from_buffer_copy(res[b])
        if return_pairs:
            r.idx = idx[b, :source.n].copy()
        out.append(r)
    return out


def icp_plane(target, source, normals=None, init=None, return_pairs=False, k=None, **kw):
    """Point-to-plane ICP (f-22 metric 1) against the target's normals; trim=, one_to_one= and f-17's options by keyword."""
    return icp_ex(target, source, normals, init, return_pairs, k=k, **plane_opts(kw))


def icp_plane_batch(target, source, inits, normals=None, return_pairs=False, k=None, **kw):
    """icp_plane from every start of `inits` in one lock-step loop."""
    return icp_ex_batch(target, source, inits, normals, return_pairs, k=k, **plane_opts(kw))


def icp_last_timing(target):
    """ms of the last icp_ex / icp_plane (or their batch) with this target, with Context.set_timing on: search, rejectors, sums,
    update; and the iterations of its longest problem."""
    ms, it = (C.c_double * 4)(), C.c_int32(0)
    _lib.check(_lib.lib().sfmhip_cloud_register_icp_last_timing(target.h, ms, C.byref(it)), "sfmhip_cloud_register_icp_last_timing")
    return dict(search=ms[0], rejectors=ms[1], sums=ms[2], update=ms[3], iterations=it.value)
