"""Dendrometry on the GPU: the measurements the reference's Dendrometry::estimate prints as blanks (src/DendrometryE.cpp:3-29)
-- tree height along the vertical, diameter at breast height (DAP / DBH), the stem taper profile, crown base height, live
crown length and crown spread N-S / E-W -- over the device-resident cloud of cloud.py (include/sfmhip.h,
sfmhip_cloud_dendrometry / sfmhip_cloud_dendro_profile).

`measure(cloud, labels, label)` returns the scalars, `profile(...)` the slice table, `measure_profile(...)` both from one run; `labels` is what
segment.segment_rgb returns (None: every finite point).  The reference has nothing to match: the contract is the rule
list of DESIGN.md f-11."""
import ctypes as C

import numpy as np

from . import _lib

MAX_SLICES = 4096
EMPTY, DBH_ONE_SLICE, NO_DBH, NO_CROWN = 1, 2, 4, 8    # bits of DendroResult.flags

SLICE_DTYPE = np.dtype([("count", "<i4"), ("stem", "<i4"), ("inliers", "<i4"), ("mask", "<i4"), ("ce", "<f8"), ("cn", "<f8"),
                        ("radius", "<f8"), ("rms", "<f8"), ("extent", "<f8")])


class DendroOpts(C.Structure):
    _fields_ = [("up", C.c_double * 3), ("north", C.c_double * 3), ("scale", C.c_double), ("ground", C.c_double),
                ("dbh_height", C.c_double), ("slice", C.c_double), ("inlier_tol", C.c_double), ("r_min", C.c_double),
                ("r_max", C.c_double), ("extent_q", C.c_double), ("extent_bin", C.c_double), ("crown_factor", C.c_double),
                ("ransac_iters", C.c_int32), ("min_inliers", C.c_int32), ("min_sectors", C.c_int32), ("crown_run", C.c_int32),
                ("min_slice_pts", C.c_int32), ("seed", C.c_uint32)]


class DendroResult(C.Structure):
    _fields_ = [("total_height", C.c_double), ("dbh", C.c_double), ("dbh_e", C.c_double), ("dbh_n", C.c_double),
                ("crown_base_height", C.c_double), ("live_crown", C.c_double), ("spread_ns", C.c_double), ("spread_ew", C.c_double),
                ("ground", C.c_double), ("n_selected", C.c_int32), ("n_slices", C.c_int32), ("crown_base_slice", C.c_int32),
                ("flags", C.c_int32)]


def set_opts(o, **kw):
    """Keyword arguments into the fields of an options structure (up / north take three numbers)."""
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no option {k}")
        if k in ("up", "north"):
            v = (C.c_double * 3)(*[float(x) for x in v])
        setattr(o, k, v)
    return o


def default_opts(**kw):
    """Rule 1's defaults (up +z, north +y, 1 m per unit, DBH at 1.3 m, 0.1 m slices, 256 iterations); keyword arguments
    override fields."""
    o = DendroOpts()
    _lib.lib().sfmhip_dendro_default_opts(C.byref(o))
    return set_opts(o, **kw)


def _labels(cloud, labels):
    if labels is None:
        return None, None
    lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
    if len(lab) != cloud.n:
        raise ValueError("labels must hold one entry per point")
    return lab, lab.ctypes.data


def measure(cloud, labels=None, label=0, opts=None):
    """DendroResult of the points with labels == label (every finite point without labels), in metres."""
    opts = opts or default_opts()
    lab, p = _labels(cloud, labels)
    out = DendroResult()
    _lib.check(_lib.lib().sfmhip_cloud_dendrometry(cloud.h, p, int(label), C.byref(opts), C.byref(out)), "sfmhip_cloud_dendrometry")
    return out


def measure_profile(cloud, labels=None, label=0, opts=None):
    """(DendroResult, slice table) from one run: the table is SLICE_DTYPE, one row per slice from the ground up, cloud units."""
    opts = opts or default_opts()
    lab, p = _labels(cloud, labels)
    rows, m, out = np.zeros(MAX_SLICES, SLICE_DTYPE), C.c_int32(0), DendroResult()
    _lib.check(_lib.lib().sfmhip_cloud_dendro_profile(cloud.h, p, int(label), C.byref(opts), MAX_SLICES, rows.ctypes.data, C.byref(m),
                                                      C.byref(out)), "sfmhip_cloud_dendro_profile")
    return out, rows[:m.value].copy()


def profile(cloud, labels=None, label=0, opts=None):
    """The slice table alone: the stem taper profile."""
    return measure_profile(cloud, labels, label, opts)[1]


def last_timing(cloud):
    """ms of the last call on the handle: frame, slice ordering, RANSAC, refit, extent + crown + spread, whole call."""
    ms = np.zeros(6, np.float64)
    _lib.check(_lib.lib().sfmhip_cloud_dendro_last_timing(cloud.h, ms.ctypes.data), "sfmhip_cloud_dendro_last_timing")
    return dict(zip(("frame", "slices", "ransac", "refit", "crown", "total"), map(float, ms)))
