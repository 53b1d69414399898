"""Crown delineation on the canopy raster (include/sfmhip.h, sfmhip_chm_crowns / sfmhip_cloud_crowns): tree
tops as variable-window maxima of the smoothed canopy height model, crowns by steepest ascent with window merging, and a tree
number per point in the layout dendro.measure takes as labels.  It finds the trees of a cloud taken from above, whose stems
trees.py cannot see.

`chm_crowns(chm, c, opts)` works on any host raster and returns (labels [Dn, De], smooth [Dn, De], tops, CrownsResult);
`crowns(cloud, opts)` works on the rasters the last terrain.terrain call left on the handle and returns (tree_of, tops,
CrownsResult); `raster(cloud)` the rasters of the last crowns call as (smooth, labels); `inventory(cloud, ...)` runs the ground
plane, the terrain, the crowns and the dendrometry of every crown as one plot inventory that needs no stems;
`last_timing(cloud)` the stage times of the last call."""
import ctypes as C

import numpy as np

from . import _lib, dendro, ground, terrain

TILE = 64                    # cells a wave takes from one raster row (csrc/crowns.h)
BATCH = 4                    # doubling rounds between two reads of the counters
MAX_TREES = 65536
NO_CANOPY, OVERFLOW = 1, 4   # bits of CrownsResult.flags

TOP_DTYPE = np.dtype([("e", "<f8"), ("n", "<f8"), ("area", "<f8"), ("height", "<f4"), ("height_smooth", "<f4"), ("cell_id", "<i4"),
                      ("ix", "<i4"), ("iy", "<i4"), ("R2", "<i4"), ("cells", "<i4"), ("points", "<i4")])


class CrownsOpts(C.Structure):
    _fields_ = [("scale", C.c_double), ("min_height", C.c_double), ("win_a", C.c_double), ("win_b", C.c_double), ("r_min", C.c_double),
                ("r_max", C.c_double), ("crown_frac", C.c_double), ("max_crown_radius", C.c_double), ("ground_clear", C.c_double),
                ("smooth_passes", C.c_int32), ("max_trees", C.c_int32)]


class CrownsResult(C.Structure):
    _fields_ = [("c", C.c_double), ("e_min", C.c_float), ("n_min", C.c_float), ("De", C.c_int32), ("Dn", C.c_int32),
                ("n_canopy", C.c_int32), ("n_summits", C.c_int32), ("n_trees", C.c_int32), ("n_labelled_cells", C.c_int32),
                ("n_labelled", C.c_int32), ("max_depth", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32)]


set_opts = dendro.set_opts


def default_opts(**kw):
    """Rule 1's defaults (1 m per unit, canopy from 2 m, 2 smoothing passes, windows 0.6 + 0.06 h within 0.6 .. 5 m, crowns down
    to 0.3 of the top within 10 m, points from 0.3 m, 4096 trees); keyword arguments override fields."""
    o = CrownsOpts()
    _lib.lib().sfmhip_crowns_default_opts(C.byref(o))
    return set_opts(o, **kw)


def chm_crowns(chm, c, opts=None, cap=None, ctx=None):
    """(labels int32 [Dn, De], smooth float32 [Dn, De], tops, CrownsResult) of a canopy raster `chm` [Dn, De] (NaN: empty) with
    cells of `c` cloud units; tops is a TOP_DTYPE table of min(cap, n_trees, max_trees) rows, e and n from the origin (0, 0)."""
    opts = opts or default_opts()
    ctx = ctx or _lib.default_context()
    z = np.ascontiguousarray(np.asarray(chm, np.float32))
    if z.ndim != 2:
        raise ValueError("chm must be a [Dn, De] raster")
    dn, de = z.shape
    cap = MAX_TREES if cap is None else int(cap)
    m = max(dn * de, 1)
    labels, smooth, tops, out = np.full(m, -1, np.int32), np.full(m, np.nan, np.float32), np.zeros(max(cap, 1), TOP_DTYPE), CrownsResult()
    _lib.check(_lib.lib().sfmhip_chm_crowns(ctx.h, z.ctypes.data if z.size else None, de, dn, float(c), C.byref(opts), labels.ctypes.data,
                                            smooth.ctypes.data, cap, tops.ctypes.data, C.byref(out)), "sfmhip_chm_crowns")
    kept = min(cap, out.n_trees, opts.max_trees)
    return labels[:dn * de].reshape(dn, de), smooth[:dn * de].reshape(dn, de), tops[:kept].copy(), out


def crowns(cloud, opts=None, cap=None):
    """(tree_of, tops, CrownsResult) on the canopy raster of the last terrain.terrain call on the handle: tree_of[i] is the tree
    of point i or -1, the layout dendro.measure takes as labels."""
    opts = opts or default_opts()
    cap = MAX_TREES if cap is None else int(cap)
    tree_of, tops, out = np.full(max(cloud.n, 1), -1, np.int32), np.zeros(max(cap, 1), TOP_DTYPE), CrownsResult()
    _lib.check(_lib.lib().sfmhip_cloud_crowns(cloud.h, C.byref(opts), tree_of.ctypes.data, cap, tops.ctypes.data, C.byref(out)),
               "sfmhip_cloud_crowns")
    cloud._crowns_dims = (out.Dn, out.De)
    return tree_of[:cloud.n], tops[:min(cap, out.n_trees, opts.max_trees)].copy(), out


def raster(cloud):
    """(smooth float32, labels int32), each [Dn, De], of the last crowns call on the handle."""
    dn, de = getattr(cloud, "_crowns_dims", (0, 0))
    m = max(dn * de, 1)
    smooth, labels = np.empty(m, np.float32), np.empty(m, np.int32)
    _lib.check(_lib.lib().sfmhip_cloud_crowns_raster(cloud.h, smooth.ctypes.data, labels.ctypes.data), "sfmhip_cloud_crowns_raster")
    return smooth[:dn * de].reshape(dn, de).copy(), labels[:dn * de].reshape(dn, de).copy()


def inventory(cloud, ground_opts=None, cams=None, terrain_opts=None, crown_opts=None, dendro_opts=None):
    """The plot inventory without stems: ground plane, the terrain in its frame, the crowns on its canopy raster, then the
    dendrometry of every crown on the normalised cloud (up +z, north +y, ground 0, the caller's `scale`).  Returns
    (GroundResult, is_ground, hag, TerrainResult, tree_of, tops, CrownsResult, [DendroResult per tree]); tree_of indexes the
    original cloud."""
    g = ground.ground_plane(cloud, None, 0, ground_opts, cams)
    is_ground, hag, tres = terrain.terrain(cloud, None, 0, terrain.opts_from_ground(g, terrain_opts or terrain.default_opts()))
    tree_of, tops, res = crowns(cloud, crown_opts)
    dopts = set_opts(dendro_opts or dendro.default_opts(), up=(0, 0, 1), north=(0, 1, 0), ground=0.0)
    with terrain.normalize(cloud) as nc:
        per_tree = [dendro.measure(nc, tree_of, j, dopts) for j in range(len(tops))]
    return g, is_ground, hag, tres, tree_of, tops, res, per_tree


def last_timing(cloud):
    """ms of the last call on the handle: smoothing, ascent, windows, labels, points, whole call; and the doubling rounds of the
    ascent and of the parents."""
    ms, rounds = np.zeros(6, np.float64), np.zeros(2, np.int32)
    _lib.check(_lib.lib().sfmhip_cloud_crowns_last_timing(cloud.h, ms.ctypes.data), "sfmhip_cloud_crowns_last_timing")
    _lib.check(_lib.lib().sfmhip_cloud_crowns_last_rounds(cloud.h, rounds.ctypes.data), "sfmhip_cloud_crowns_last_rounds")
    return dict(zip(("smooth", "ascent", "windows", "labels", "points", "total"), map(float, ms)), rounds_up=int(rounds[0]),
                rounds_parent=int(rounds[1]))
