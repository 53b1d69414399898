"""The terrain model of the device-resident cloud of cloud.py (include/sfmhip.h, sfmhip_cloud_terrain): the
ground points by a progressive morphological filter on a raster, the digital terrain model (DTM) rasterised from them, every
point's height above it, the canopy raster and the normalised cloud on which trees.py and dendro.py run unchanged with
up = +z and ground = 0.

`terrain(cloud, labels, label, opts)` returns (is_ground int32 [n], hag float32 [n], TerrainResult); `raster(cloud)` the
rasters of the last call as (dtm, kind, chm), each [Dn, De]; `normalize(cloud)` the normalised cloud as a Cloud born on the
device; `opts_from_ground(result, opts)` writes a GroundResult's frame into a TerrainOpts; `inventory(cloud, ...)` runs the
ground plane, the terrain, the trees and the dendrometry of every tree as one plot inventory; `last_timing(cloud)` the stage
times of the last call."""
import ctypes as C

import numpy as np

from . import _lib, dendro, ground, trees
from .cloud import Cloud

TILE = 64                                    # the width of the opening's LDS tile (csrc/terrain.h)
NONE_SELECTED, UNFILLED, NO_WINDOW = 1, 2, 4  # bits of TerrainResult.flags
EMPTY, GROUND, FILLED = 0, 1, 2              # a cell's kind


class TerrainOpts(C.Structure):
    _fields_ = [("up", C.c_double * 3), ("north", C.c_double * 3), ("scale", C.c_double), ("cell", C.c_double),
                ("max_window", C.c_double), ("slope", C.c_double), ("initial_distance", C.c_double), ("max_distance", C.c_double),
                ("base", C.c_int32), ("exponential", C.c_int32), ("fill_rounds", C.c_int32), ("relax_sweeps", C.c_int32)]


class TerrainResult(C.Structure):
    _fields_ = [("c", C.c_double), ("e_min", C.c_float), ("n_min", C.c_float), ("t_min", C.c_float), ("t_max", C.c_float),
                ("hag_max", C.c_float), ("De", C.c_int32), ("Dn", C.c_int32), ("n_selected", C.c_int32), ("n_ground", C.c_int32),
                ("n_windows", C.c_int32), ("n_kind1", C.c_int32), ("n_kind2", C.c_int32), ("n_kind0", C.c_int32),
                ("fill_rounds", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32)]


set_opts = dendro.set_opts


def default_opts(**kw):
    """Rule 1's defaults (up +z, north +y, 1 m per unit, 0.5 m cells, windows up to 9 m, slope 1, distances 0.15 .. 2.5 m, base 2,
    exponential, 64 fill rounds, 32 relaxation sweeps); keyword arguments override fields."""
    o = TerrainOpts()
    _lib.lib().sfmhip_terrain_default_opts(C.byref(o))
    return set_opts(o, **kw)


def opts_from_ground(result, opts=None):
    """The TerrainOpts (a fresh default one without `opts`) with up and north from `result`."""
    opts = opts or default_opts()
    _lib.check(_lib.lib().sfmhip_terrain_opts_from_ground(C.byref(result), C.byref(opts)), "sfmhip_terrain_opts_from_ground")
    return opts


def terrain(cloud, labels=None, label=0, opts=None):
    """(is_ground, hag, TerrainResult) of the points with labels == label (every finite point without labels): is_ground[i] is
    1 for a ground point, hag[i] the height of point i above the terrain in cloud units, NaN for a point that is not selected."""
    opts = opts or default_opts()
    lab, p = dendro._labels(cloud, labels)
    is_ground, hag, out = np.zeros(max(cloud.n, 1), np.int32), np.full(max(cloud.n, 1), np.nan, np.float32), TerrainResult()
    _lib.check(_lib.lib().sfmhip_cloud_terrain(cloud.h, p, int(label), C.byref(opts), is_ground.ctypes.data, hag.ctypes.data,
                                               C.byref(out)), "sfmhip_cloud_terrain")
    cloud._terrain_dims = (out.Dn, out.De)
    return is_ground[:cloud.n], hag[:cloud.n], out


def raster(cloud):
    """(dtm float32, kind uint8, chm float32), each [Dn, De], of the last terrain call on the handle."""
    dn, de = getattr(cloud, "_terrain_dims", (0, 0))
    m = max(dn * de, 1)
    dtm, kind, chm = np.empty(m, np.float32), np.empty(m, np.uint8), np.empty(m, np.float32)
    _lib.check(_lib.lib().sfmhip_cloud_terrain_raster(cloud.h, dtm.ctypes.data, kind.ctypes.data, chm.ctypes.data),
               "sfmhip_cloud_terrain_raster")
    return tuple(a[:dn * de].reshape(dn, de).copy() for a in (dtm, kind, chm))


def normalize(cloud):
    """The normalised cloud of the last terrain call: row i = (e, n, hag) of point i, NaN where it has no height.  It is born on
    the device; the points never pass through the host."""
    h = C.c_void_p()
    _lib.check(_lib.lib().sfmhip_cloud_terrain_normalize(cloud.h, C.byref(h)), "sfmhip_cloud_terrain_normalize")
    return Cloud.from_handle(h, cloud.ctx)


def inventory(cloud, ground_opts=None, cams=None, terrain_opts=None, trees_opts=None, dendro_opts=None):
    """The plot inventory over a terrain: ground plane, the terrain in its frame, then the trees and the dendrometry of every
    tree on the normalised cloud (up +z, north +y, ground 0, the caller's `scale`).  Returns (GroundResult, is_ground, hag,
    TerrainResult, tree_of, stems, TreesResult, [DendroResult per tree]); tree_of indexes the original cloud."""
    g = ground.ground_plane(cloud, None, 0, ground_opts, cams)
    is_ground, hag, tres = terrain(cloud, None, 0, opts_from_ground(g, terrain_opts or default_opts()))
    flat = dict(up=(0, 0, 1), north=(0, 1, 0), ground=0.0)
    topts = set_opts(trees_opts or trees.default_opts(), **flat)
    dopts = set_opts(dendro_opts or dendro.default_opts(), **flat)
    with normalize(cloud) as nc:
        tree_of, stems, res = trees.trees(nc, None, 0, topts)
        per_tree = [dendro.measure(nc, tree_of, s, dopts) for s in range(res.n_trees)]
    return g, is_ground, hag, tres, tree_of, stems, res, per_tree


def last_timing(cloud):
    """ms of the last call on the handle: frame + raster, windows, point test + terrain raster, fill + relax, heights + canopy,
    whole call."""
    ms = np.zeros(6, np.float64)
    _lib.check(_lib.lib().sfmhip_cloud_terrain_last_timing(cloud.h, ms.ctypes.data), "sfmhip_cloud_terrain_last_timing")
    return dict(zip(("frame", "windows", "ground", "fill", "heights", "total"), map(float, ms)))
