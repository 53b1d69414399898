"""The colour region growing that follows map3D (reference src/Segmentation.cpp:3-66: pcl::RegionGrowingRGB over the
indices of a PassThrough on z) and Dendrometry::estimate's bounds (src/DendrometryE.cpp:3-29) on the GPU, over the
device-resident cloud of cloud.py (include/sfmhip.h, sfmhip_cloud_segment_* / sfmhip_cloud_minmax).

`segment_rgb(cloud, rgb, indices)` returns the final cluster of every point (-1 = in none); `color_based_growing_
segmentation(xyz, rgb)` runs the reference's call (PassThrough z in [0, 14], its four setters) on a loaded MAP3D.pcd
cloud.  Parity with PCL is UNPINNED."""
import ctypes as C

import numpy as np

from . import _lib
from .cloud import Cloud

PASS_AXIS, PASS_LO, PASS_HI = 2, 0.0, 14.0       # setFilterFieldName("z"), setFilterLimits(0.0, 14.0)
KMAX = 128


class SegmentOpts(C.Structure):
    _fields_ = [("region_neighbour_number", C.c_int32), ("neighbour_number", C.c_int32), ("min_cluster_size", C.c_int32),
                ("max_cluster_size", C.c_int32), ("distance_threshold", C.c_float), ("point_color_threshold", C.c_float),
                ("region_color_threshold", C.c_float)]


class SegmentStats(C.Structure):
    _fields_ = [("n_idx", C.c_int32), ("n_segments", C.c_int32), ("n_regions", C.c_int32), ("rounds", C.c_int32)]


def default_opts(**kw):
    """The reference's options (distance 10, point colour 6, region colour 5, min cluster 600; PCL's defaults: 100
    neighbours searched, 30 grown over, no upper cluster size); keyword arguments override fields."""
    o = SegmentOpts()
    _lib.lib().sfmhip_segment_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no option {k}")
        setattr(o, k, v)
    return o


def _p(a):
    return a.ctypes.data


def _rgb(cloud, rgb):
    rgb = np.ascontiguousarray(np.asarray(rgb).astype(np.uint32, copy=False).reshape(-1))
    if len(rgb) != cloud.n:
        raise ValueError("rgb must hold one packed colour per point")
    return rgb


def _indices(indices):
    ind = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1))
    return ind


def pack_rgb(r, g, b):
    """0x00RRGGBB per point from three 8-bit channels."""
    return (np.asarray(r, np.uint32) << 16) | (np.asarray(g, np.uint32) << 8) | np.asarray(b, np.uint32)


def subset_knn(cloud, indices, k):
    """(idx [n_idx, k] int32 cloud indices, d2 [n_idx, k] float32): the k nearest INDEXED points of every indexed
    point, itself included, in (d2, index) order; -1 / inf where the list is shorter."""
    if not 1 <= k <= KMAX:
        raise ValueError(f"k must be in 1..{KMAX}")
    ind = _indices(indices)
    idx, d2 = np.empty((max(len(ind), 1), k), np.int32), np.empty((max(len(ind), 1), k), np.float32)
    _lib.check(_lib.lib().sfmhip_cloud_subset_knn(cloud.h, _p(ind), len(ind), int(k), _p(idx), _p(d2)), "sfmhip_cloud_subset_knn")
    return idx[:len(ind)].copy(), d2[:len(ind)].copy()


def grow(cloud, rgb, indices, opts=None):
    """The growth alone: (segment [n] int32, -1 outside the list; segment count; propagation rounds)."""
    opts = opts or default_opts()
    rgb, ind = _rgb(cloud, rgb), _indices(indices)
    seg, ns, rounds = np.empty(max(cloud.n, 1), np.int32), C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().sfmhip_cloud_segment_grow(cloud.h, _p(rgb), _p(ind), len(ind), C.byref(opts), _p(seg), C.byref(ns),
                                                    C.byref(rounds)), "sfmhip_cloud_segment_grow")
    return seg[:cloud.n].copy(), ns.value, rounds.value


def segment_rgb(cloud, rgb, indices, opts=None):
    """(labels [n] int32: the final cluster of every point, -1 = in no cluster; cluster count; SegmentStats).  Cluster
    c is np.nonzero(labels == c)[0]: ascending indices, as PCL lists them."""
    opts = opts or default_opts()
    rgb, ind = _rgb(cloud, rgb), _indices(indices)
    labels, nc, st = np.empty(max(cloud.n, 1), np.int32), C.c_int32(0), SegmentStats()
    _lib.check(_lib.lib().sfmhip_cloud_segment_rgb(cloud.h, _p(rgb), _p(ind), len(ind), C.byref(opts), _p(labels), C.byref(nc),
                                                   C.byref(st)), "sfmhip_cloud_segment_rgb")
    return labels[:cloud.n].copy(), nc.value, st


def last_timing(cloud):
    """ms of the last segment_rgb call on the handle: subset k-NN, growth, segment statistics, host regions, whole call."""
    ms = np.zeros(5, np.float64)
    _lib.check(_lib.lib().sfmhip_cloud_segment_last_timing(cloud.h, _p(ms)), "sfmhip_cloud_segment_last_timing")
    return dict(zip(("knn", "growth", "statistics", "regions", "total"), map(float, ms)))


def minmax(cloud):
    """(min [3], max [3] float32, height): pcl::getMinMax3D over the finite points and Dendrometry's "Total Height"."""
    mn, mx, h = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_double(0)
    _lib.check(_lib.lib().sfmhip_cloud_minmax(cloud.h, _p(mn), _p(mx), C.byref(h)), "sfmhip_cloud_minmax")
    return mn, mx, h.value


def color_based_growing_segmentation(xyz, rgb, opts=None, ctx=None):
    """The reference's call on a loaded cloud: PassThrough on z in [0, 14], then RegionGrowingRGB with its setters.
    Returns (labels, cluster count, stats); zero clusters is the reference's failure and is the caller's to report."""
    with Cloud(xyz, ctx=ctx) as c:
        ind = c.passthrough(PASS_AXIS, PASS_LO, PASS_HI)
        if len(ind) == 0:
            return np.full(c.n, -1, np.int32), 0, SegmentStats()
        return segment_rgb(c, rgb, ind, opts)
