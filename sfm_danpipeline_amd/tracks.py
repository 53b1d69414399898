"""Multi-view feature tracks and their N-view triangulation (include/sfmhip.h, sfmhip_tracks_*): the
components of the match graph as the CSR `incremental.find_2d3d` takes, numbered by their least node, conflicting ones
(two features of one image) dropped, and one DLT point per track over every view that has a pose.

`build(ctx, n_feat, pairs, counts, q, t, **opts)` takes host lists in MatchPlan.fetch's layout, `build_from_plan(plan, **opts)`
reads the lists of the plan's last run where they lie on the device, `build_from_verified(verified, **opts)` those of a
verify.Verified; all return a `Tracks`, whose `stats`, `download()`,
`triangulate(...)`, `last_timing()` and `close()` mirror the C entry points."""
import ctypes as C

import numpy as np

from . import _lib

STAGES = ("check", "hook", "sort", "number", "buckets", "triangulate")


class TracksOpts(C.Structure):
    _fields_ = [("min_len", C.c_int32), ("front_only", C.c_int32)]


class TracksStats(C.Structure):
    _fields_ = [("nodes", C.c_int64), ("edges", C.c_int64), ("components", C.c_int64), ("conflicting", C.c_int64),
                ("short_tracks", C.c_int64), ("n_tracks", C.c_int64), ("n_obs", C.c_int64)]


def default_opts(**kw):
    """min_len = 2, front_only = 0; keyword arguments override fields."""
    o = TracksOpts()
    _lib.lib().sfmhip_tracks_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no tracks option {k!r}")
        setattr(o, k, v)
    return o


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Tracks:
    def __init__(self, handle):
        self.h = handle
        self.stats = TracksStats()
        _lib.check(_lib.lib().sfmhip_tracks_counts(self.h, C.byref(self.stats)), "sfmhip_tracks_counts")

    def download(self):
        """(trk_ptr [n_tracks + 1], trk_view [n_obs], trk_feat [n_obs], node_track [nodes])"""
        s = self.stats
        ptr, view, feat = np.zeros(s.n_tracks + 1, np.int32), np.zeros(s.n_obs, np.int32), np.zeros(s.n_obs, np.int32)
        node = np.zeros(s.nodes, np.int32)
        _lib.check(_lib.lib().sfmhip_tracks_download(self.h, ptr.ctypes.data, view.ctypes.data, feat.ctypes.data, node.ctypes.data),
                   "sfmhip_tracks_download")
        return ptr, view, feat, node

    def triangulate(self, poses, has_pose, K, dist, xy_ptr, xy, max_err=6.0, min_views=2):
        """(X [n_tracks, 3], err [n_obs], n_used [n_tracks], keep [n_tracks] bool) of rules R1-R5.  poses: [n_images, 3, 4];
        xy: the pixels of every image one after the other, image v's at xy[xy_ptr[v]:xy_ptr[v + 1]]."""
        s = self.stats
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1)
        has = np.ascontiguousarray(has_pose, dtype=np.uint8)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(5)
        xy_ptr, xy = _i32(xy_ptr), np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        if poses.size != 12 * has.size or xy_ptr.size != has.size + 1 or (xy_ptr.size and xy.size < 2 * int(xy_ptr[-1])):
            raise ValueError("poses, has_pose, xy_ptr and xy disagree about the number of images or pixels")
        X, err = np.zeros((s.n_tracks, 3), np.float64), np.zeros(s.n_obs, np.float32)
        used, keep = np.zeros(s.n_tracks, np.int32), np.zeros(s.n_tracks, np.uint8)
        _lib.check(_lib.lib().sfmhip_tracks_triangulate(self.h, poses.ctypes.data, has.ctypes.data, K.ctypes.data, dist.ctypes.data,
                                                        xy_ptr.ctypes.data, xy.ctypes.data, float(max_err), int(min_views), X.ctypes.data,
                                                        err.ctypes.data, used.ctypes.data, keep.ctypes.data), "sfmhip_tracks_triangulate")
        return X, err, used, keep.astype(bool)

    def last_timing(self):
        """seconds by stage (context timing on): check, hook, sort, number, buckets of the build; triangulate of the last call"""
        sec = np.zeros(len(STAGES), np.float64)
        _lib.check(_lib.lib().sfmhip_tracks_last_timing(self.h, sec.ctypes.data), "sfmhip_tracks_last_timing")
        return dict(zip(STAGES, map(float, sec)))

    def close(self):
        if self.h:
            _lib.lib().sfmhip_tracks_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build(ctx, n_feat, pairs, counts, q, t, **opts):
    """The tracks of host lists: pairs [n_pairs, 2], counts [n_pairs], q / t the matches of every pair one after the other."""
    ctx = ctx or _lib.default_context()
    n_feat, pairs, counts, q, t = _i32(n_feat), _i32(pairs).reshape(-1), _i32(counts), _i32(q), _i32(t)
    if pairs.size != 2 * counts.size or q.size != t.size or (counts.size and (counts >= 0).all() and int(counts.sum()) != q.size):
        raise ValueError("pairs, counts and the match lists disagree")
    o, h = default_opts(**opts), C.c_void_p()
    _lib.check(_lib.lib().sfmhip_tracks_build(ctx.h, n_feat.size, n_feat.ctypes.data, counts.size, pairs.ctypes.data, counts.ctypes.data,
                                              q.ctypes.data, t.ctypes.data, C.byref(o), C.byref(h)), "sfmhip_tracks_build")
    return Tracks(h)


def build_from_plan(plan, **opts):
    """The tracks of the lists a matcher.MatchPlan's last run left on the device."""
    o, h = default_opts(**opts), C.c_void_p()
    _lib.check(_lib.lib().sfmhip_tracks_build_from_plan(plan.h, C.byref(o), C.byref(h)), "sfmhip_tracks_build_from_plan")
    return Tracks(h)


def build_from_verified(verified, **opts):
    """The tracks of a verify.Verified's lists, read where they lie on the device."""
    o, h = default_opts(**opts), C.c_void_p()
    _lib.check(_lib.lib().sfmhip_tracks_build_from_verified(verified.h, C.byref(o), C.byref(h)), "sfmhip_tracks_build_from_verified")
    return Tracks(h)
