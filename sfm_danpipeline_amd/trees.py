"""The trees of a plot on the device-resident cloud of cloud.py (include/sfmhip.h, sfmhip_cloud_trees): the
stems in a height band of the levelled cloud and, for every point above the ground, the number of the tree it belongs to --
the `labels` that dendro.py and ground.py take.

`trees(cloud, labels, label, opts)` returns (tree_of int32 [n], the stem table, TreesResult); `opts_from_ground(result, opts)`
writes a GroundResult's frame into a TreesOpts (up, north, ground = offset * scale); `inventory(cloud, ...)` runs the ground
plane, the trees and the dendrometry of every tree as one plot inventory; `last_timing(cloud)` the stage times of the last
call."""
import ctypes as C

import numpy as np

from . import _lib, dendro, ground

MAX_TREES = 4096
NONE_ABOVE, NO_STEM, TOO_MANY = 1, 2, 4    # bits of TreesResult.flags

STEM_DTYPE = np.dtype([("e", "<f8"), ("n", "<f8"), ("foot", "<f8", 3), ("cell_id", "<i4"), ("band_points", "<i4"), ("band_cells", "<i4"),
                       ("points", "<i4")])


class TreesOpts(C.Structure):
    _fields_ = [("up", C.c_double * 3), ("north", C.c_double * 3), ("scale", C.c_double), ("ground", C.c_double),
                ("ground_clear", C.c_double), ("band_lo", C.c_double), ("band_hi", C.c_double), ("stem_cell", C.c_double),
                ("max_stem_width", C.c_double), ("voxel", C.c_double), ("max_path", C.c_double), ("min_cell_pts", C.c_int32),
                ("min_stem_pts", C.c_int32), ("max_trees", C.c_int32), ("pad", C.c_int32)]


class TreesResult(C.Structure):
    _fields_ = [("n_selected", C.c_int32), ("n_above", C.c_int32), ("n_band", C.c_int32), ("n_trees", C.c_int32), ("n_voxels", C.c_int32),
                ("n_labelled", C.c_int32), ("max_cost", C.c_int32), ("flags", C.c_int32)]


set_opts = dendro.set_opts


def default_opts(**kw):
    """Rule 1's defaults (up +z, north +y, 1 m per unit, clearance 0.3 m, band 1.0 .. 1.6 m, 0.05 m cells, 0.15 m voxels);
    `ground` has none and must be given; keyword arguments override fields."""
    o = TreesOpts()
    _lib.lib().sfmhip_trees_default_opts(C.byref(o))
    return set_opts(o, **kw)


def opts_from_ground(result, opts=None):
    """The TreesOpts (a fresh default one without `opts`) with up, north and ground = offset * scale from `result`."""
    opts = opts or default_opts()
    _lib.check(_lib.lib().sfmhip_trees_opts_from_ground(C.byref(result), C.byref(opts)), "sfmhip_trees_opts_from_ground")
    return opts


def trees(cloud, labels=None, label=0, opts=None, cap=MAX_TREES):
    """(tree_of, stems, TreesResult) of the points with labels == label (every finite point without labels): tree_of[i] is the
    tree of point i or -1, stems a STEM_DTYPE table of min(cap, n_trees) rows."""
    if opts is None:
        raise ValueError("trees needs options with `ground` set (opts_from_ground, or default_opts(ground=...))")
    lab, p = dendro._labels(cloud, labels)
    tree_of, stems, out = np.full(max(cloud.n, 1), -1, np.int32), np.zeros(max(cap, 1), STEM_DTYPE), TreesResult()
    _lib.check(_lib.lib().sfmhip_cloud_trees(cloud.h, p, int(label), C.byref(opts), tree_of.ctypes.data, int(cap), stems.ctypes.data,
                                             C.byref(out)), "sfmhip_cloud_trees")
    return tree_of[:cloud.n], stems[:min(cap, out.n_trees)].copy(), out


def inventory(cloud, ground_opts=None, cams=None, trees_opts=None, dendro_opts=None):
    """The plot inventory: ground plane, trees, then the dendrometry of every tree in the ground's frame.  Returns
    (GroundResult, tree_of, stems, TreesResult, [DendroResult per tree]); trees_opts / dendro_opts give everything but the
    frame (their `scale` is the caller's)."""
    g = ground.ground_plane(cloud, None, 0, ground_opts, cams)
    topts = opts_from_ground(g, trees_opts or default_opts())
    dopts = ground.opts_from_ground(g, dendro_opts or dendro.default_opts())
    tree_of, stems, res = trees(cloud, None, 0, topts)
    return g, tree_of, stems, res, [dendro.measure(cloud, tree_of, s, dopts) for s in range(res.n_trees)]


def last_timing(cloud):
    """ms of the last call on the handle: frame + bounds, stems, voxels, sweeps, labels, whole call; and the sweeps enqueued."""
    ms, sweeps = np.zeros(6, np.float64), C.c_int32(0)
    _lib.check(_lib.lib().sfmhip_cloud_trees_last_timing(cloud.h, ms.ctypes.data, C.byref(sweeps)), "sfmhip_cloud_trees_last_timing")
    return dict(zip(("frame", "stems", "voxels", "sweeps", "labels", "total"), map(float, ms)), n_sweeps=sweeps.value)
