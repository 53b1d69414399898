"""Two-view verification of match lists on the device before the multi-view tracks (include/sfmhip.h, sfmhip_verify_* /
sfmhip_verified_*): per pair findEssentialMat's RANSAC over the pixels the lists name, then the pair's inliers
in list order -- or nothing, for a pair without a model or with fewer than `min_inliers` inliers.

`verify_plan(plan, xy_ptr, xy, K, **opts)` reads the lists of a matcher.MatchPlan's last run where they lie on the device,
`verify_lists(ctx, n_feat, pairs, counts, q, t, xy_ptr, xy, K, **opts)` takes host lists in MatchPlan.fetch's layout; both
return a `Verified`, whose `stats`, `download()`, `last_timing()` and `close()` mirror the C entry points.
`tracks.build_from_verified(verified, **opts)` builds the tracks of its lists without a visit to the host."""
import ctypes as C

import numpy as np

from . import _lib

STAGES = ("gather", "ransac", "compact", "total")


class VerifyOpts(C.Structure):
    _fields_ = [("prob", C.c_double), ("threshold", C.c_double), ("min_inliers", C.c_int32), ("reserved", C.c_int32)]


class VerifyStats(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("pairs_kept", C.c_int64), ("pairs_no_model", C.c_int64), ("matches_in", C.c_int64),
                ("matches_out", C.c_int64)]


def default_opts(**kw):
    """prob = 0.999, threshold = 1.0, min_inliers = 15; keyword arguments override fields."""
    o = VerifyOpts()
    _lib.lib().sfmhip_verify_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no verify option {k!r}")
        setattr(o, k, v)
    return o


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    return None if a is None else a.ctypes.data


class Verified:
    def __init__(self, handle):
        self.h = handle
        self.stats = VerifyStats()
        _lib.check(_lib.lib().sfmhip_verified_counts(self.h, C.byref(self.stats)), "sfmhip_verified_counts")

    def download(self):
        """dict(counts [n_pairs], q, t [matches_out] packed pair after pair, inliers, iterations [n_pairs], E [n_pairs, 3, 3],
        kept [n_pairs] bool)"""
        s = self.stats
        n = int(s.pairs)
        counts, inl, its = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        q, t = np.zeros(s.matches_out, np.int32), np.zeros(s.matches_out, np.int32)
        E, kept = np.zeros((n, 3, 3), np.float64), np.zeros(n, np.uint8)
        _lib.check(_lib.lib().sfmhip_verified_download(self.h, counts.ctypes.data, q.ctypes.data, t.ctypes.data, inl.ctypes.data,
                                                       its.ctypes.data, E.ctypes.data, kept.ctypes.data), "sfmhip_verified_download")
        return dict(counts=counts, q=q, t=t, inliers=inl, iterations=its, E=E, kept=kept.astype(bool))

    def last_timing(self):
        """seconds of the call that made the handle: uploads + gather, the RANSAC, the compaction, the whole call"""
        sec = np.zeros(len(STAGES), np.float64)
        _lib.check(_lib.lib().sfmhip_verified_last_timing(self.h, sec.ctypes.data), "sfmhip_verified_last_timing")
        return dict(zip(STAGES, map(float, sec)))

    def close(self):
        if self.h:
            _lib.lib().sfmhip_verified_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pixels(xy_ptr, xy, K):
    xy_ptr = None if xy_ptr is None else _i32(xy_ptr)
    xy = None if xy is None else np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    K = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    if xy_ptr is not None and xy is not None and xy_ptr.size and xy.size < 2 * int(xy_ptr[-1]):
        raise ValueError("xy holds fewer pixels than xy_ptr names")
    return xy_ptr, xy, K


def verify_plan(plan, xy_ptr, xy, K, **opts):
    """The verified set of the lists a matcher.MatchPlan's last run left on the device.  xy: the pixels of every image one
    after the other, image v's at xy[xy_ptr[v]:xy_ptr[v + 1]]."""
    xy_ptr, xy, K = _pixels(xy_ptr, xy, K)
    if xy_ptr is not None and xy_ptr.size != len(plan.set.n_rows) + 1:
        raise ValueError("xy_ptr and the image set disagree about the number of images")
    o, h = default_opts(**opts), C.c_void_p()
    _lib.check(_lib.lib().sfmhip_matchplan_verify(plan.h, _ptr(xy_ptr), _ptr(xy), _ptr(K), C.byref(o), C.byref(h)), "sfmhip_matchplan_verify")
    return Verified(h)


def verify_lists(ctx, n_feat, pairs, counts, q, t, xy_ptr, xy, K, **opts):
    """The verified set of host lists: pairs [n_pairs, 2], counts [n_pairs], q / t the matches of every pair one after the other."""
    ctx = ctx or _lib.default_context()
    n_feat, pairs, counts, q, t = _i32(n_feat), _i32(pairs).reshape(-1), _i32(counts), _i32(q), _i32(t)
    if pairs.size != 2 * counts.size or q.size != t.size or (counts.size and (counts >= 0).all() and int(counts.sum()) != q.size):
        raise ValueError("pairs, counts and the match lists disagree")
    xy_ptr, xy, K = _pixels(xy_ptr, xy, K)
    if xy_ptr is not None and xy_ptr.size != n_feat.size + 1:
        raise ValueError("xy_ptr and n_feat disagree about the number of images")
    o, h = default_opts(**opts), C.c_void_p()
    _lib.check(_lib.lib().sfmhip_verify_lists(ctx.h, n_feat.size, n_feat.ctypes.data, counts.size, pairs.ctypes.data, counts.ctypes.data,
                                              q.ctypes.data, t.ctypes.data, _ptr(xy_ptr), _ptr(xy), _ptr(K), C.byref(o), C.byref(h)),
               "sfmhip_verify_lists")
    return Verified(h)
