"""map3D's step 10 (reference src/Sfm.cpp:94-102, bodies :1323-1383) on the GPU: PCL 1.8.1's PassThrough,
RadiusOutlierRemoval and k-nearest NormalEstimation over a device-resident cloud (include/sfmhip.h, sfmhip_cloud_*).

`Cloud(xyz)` uploads the points once; its methods share that upload and the grids built for it.  `map3d_step10(xyz)`
runs the three calls with the reference's constants, including its quirk: all three read the unfiltered cloud, so
the normals are those of every input point (then negated, as create_mesh does).  Parity with PCL is UNPINNED
(DESIGN.md f-6)."""
import ctypes as C

import numpy as np

from . import _lib

PASS_AXIS, PASS_LO, PASS_HI = 0, 0.003, 0.83     # cloudPointFilter: setFilterFieldName("x"), setFilterLimits(0.003, 0.83)
RADIUS, MIN_PTS = 0.07, 150                      # removePoints: setRadiusSearch(0.07), setMinNeighborsInRadius(150)
K_NORMALS = 10                                   # create_mesh: setKSearch(10)
KMAX = 32
MEAN_K_MAX = 63                                  # StatisticalOutlierRemoval's mean_k (one list slot per lane of a wave)
AXES = {"x": 0, "y": 1, "z": 2}


def _p(a):
    return a.ctypes.data


class MlsOpts(C.Structure):                      # sfmhip_mls_opts
    _fields_ = [("search_radius", C.c_double), ("polynomial_order", C.c_int32), ("compute_normals", C.c_int32),
                ("sqr_gauss_param", C.c_double)]


class MlsStats(C.Structure):                     # sfmhip_mls_stats
    _fields_ = [(k, C.c_int32) for k in ("n_out", "n_dropped", "n_plane_only", "n_degenerate", "n_fit_failed", "max_neighbours")]


class Cloud:
    """A cloud of n points (float32 [n, 3]) resident on the device of `ctx`."""

    def __init__(self, xyz, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
        self.n = len(self.xyz)
        self.h = C.c_void_p()
        _lib.check(_lib.lib().sfmhip_cloud_create(self.ctx.h, self.n, _p(self.xyz), C.byref(self.h)), "sfmhip_cloud_create")

    def passthrough(self, axis="x", lo=PASS_LO, hi=PASS_HI, negative=False):
        """Indices (input order) PassThrough keeps: finite points with lo <= v <= hi in float (outside, if negative)."""
        ax = AXES[axis] if isinstance(axis, str) else int(axis)
        if ax not in (0, 1, 2):
            raise ValueError("axis must be x, y or z")
        out, m = np.empty(max(self.n, 1), np.int32), C.c_int32(0)
        _lib.check(_lib.lib().sfmhip_cloud_passthrough(self.h, ax, float(np.float32(lo)), float(np.float32(hi)), int(bool(negative)),
                                                       _p(out), C.byref(m)), "sfmhip_cloud_passthrough")
        return out[:m.value].copy()

    def radius_count(self, radius, cap=0):
        """Per point: finite points with d2 < (float)(r * r), itself included (min(count, cap) when cap > 0)."""
        if not radius > 0:
            raise ValueError("radius must be > 0")
        out = np.empty(max(self.n, 1), np.int32)
        _lib.check(_lib.lib().sfmhip_cloud_radius_count(self.h, float(radius), int(cap), _p(out)), "sfmhip_cloud_radius_count")
        return out[:self.n].copy()

    def radius_outlier(self, radius=RADIUS, min_pts=MIN_PTS):
        """Indices RadiusOutlierRemoval keeps: count (above) > min_pts."""
        if not radius > 0 or min_pts < 0:
            raise ValueError("radius must be > 0 and min_pts >= 0")
        out, m = np.empty(max(self.n, 1), np.int32), C.c_int32(0)
        _lib.check(_lib.lib().sfmhip_cloud_radius_outlier(self.h, float(radius), int(min_pts), _p(out), C.byref(m)),
                   "sfmhip_cloud_radius_outlier")
        return out[:m.value].copy()

    def knn(self, k):
        """(idx [n, k] int32, d2 [n, k] float32): the k nearest finite points in (d2, index) order, -1 / inf padded."""
        if not 1 <= k <= KMAX:
            raise ValueError(f"k must be in 1..{KMAX}")
        idx, d2 = np.empty((max(self.n, 1), k), np.int32), np.empty((max(self.n, 1), k), np.float32)
        _lib.check(_lib.lib().sfmhip_cloud_knn(self.h, int(k), _p(idx), _p(d2)), "sfmhip_cloud_knn")
        return idx[:self.n].copy(), d2[:self.n].copy()

    def normals(self, k=K_NORMALS, viewpoint=(0.0, 0.0, 0.0)):
        """[n, 4] float32 (nx, ny, nz, curvature) of NormalEstimation with setKSearch(k), flipped towards viewpoint."""
        if not 1 <= k <= KMAX:
            raise ValueError(f"k must be in 1..{KMAX}")
        vp = np.ascontiguousarray(np.asarray(viewpoint, np.float32).reshape(3))
        out = np.empty((max(self.n, 1), 4), np.float32)
        _lib.check(_lib.lib().sfmhip_cloud_normals(self.h, int(k), _p(vp), _p(out)), "sfmhip_cloud_normals")
        return out[:self.n].copy()

    @classmethod
    def from_handle(cls, h, ctx):
        """A cloud born on the device (the voxel grid's centroids, a selection): `xyz` is None until download()."""
        self = cls.__new__(cls)
        self.ctx, self.h, self.xyz = ctx, h, None
        n = C.c_int32(0)
        _lib.check(_lib.lib().sfmhip_cloud_size(self.h, C.byref(n), None), "sfmhip_cloud_size")
        self.n = n.value
        return self

    def download(self):
        """The points as float32 [n, 3] (kept as `xyz` from then on)."""
        if self.xyz is None:
            out = np.empty((max(self.n, 1), 3), np.float32)
            _lib.check(_lib.lib().sfmhip_cloud_download(self.h, _p(out)), "sfmhip_cloud_download")
            self.xyz = out[:self.n].copy()
        return self.xyz

    def select(self, idx):
        """A new device cloud of the points idx (any order, duplicates allowed), gathered on the device."""
        idx = np.ascontiguousarray(np.asarray(idx, np.int32).reshape(-1))
        h = C.c_void_p()
        _lib.check(_lib.lib().sfmhip_cloud_select(self.h, _p(idx) if len(idx) else None, len(idx), C.byref(h)), "sfmhip_cloud_select")
        return Cloud.from_handle(h, self.ctx)

    def voxel_grid(self, leaf, min_points=0, rgb=None, normals=None, return_cloud=False):
        """PCL's VoxelGrid: a dict with `xyz` [m, 3] (the centroids, ascending voxel index), `voxel_of` [n]
        (each point's output row, -1 for none), `rgb` [m] / `normals` [m, 3] when given (downsample_all_data) and, with
        return_cloud, `cloud`: the centroids as a device cloud that was never on the host.  `leaf`: one size or three."""
        lf = np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, np.float32), (3,)))
        n1 = max(self.n, 1)
        col = None if rgb is None else np.ascontiguousarray(np.asarray(rgb, np.uint32).reshape(-1))
        nrm = None if normals is None else np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
        if (col is not None and len(col) != self.n) or (nrm is not None and len(nrm) != self.n):
            raise ValueError("rgb / normals must have one row per point")
        oxyz, vox = np.empty((n1, 3), np.float32), np.empty(n1, np.int32)
        ocol = None if col is None else np.empty(n1, np.uint32)
        onrm = None if nrm is None else np.empty((n1, 3), np.float32)
        m, h = C.c_int32(0), C.c_void_p()
        opt = lambda a: None if a is None else _p(a)
        _lib.check(_lib.lib().sfmhip_cloud_voxel_grid(self.h, _p(lf), int(min_points), opt(col), opt(nrm), _p(oxyz), opt(ocol), opt(onrm),
                                                      _p(vox), C.byref(m), C.byref(h) if return_cloud else None),
                   "sfmhip_cloud_voxel_grid")
        out = {"xyz": oxyz[:m.value].copy(), "voxel_of": vox[:self.n].copy()}
        if ocol is not None:
            out["rgb"] = ocol[:m.value].copy()
        if onrm is not None:
            out["normals"] = onrm[:m.value].copy()
        if return_cloud:
            out["cloud"] = Cloud.from_handle(h, self.ctx)
        return out

    def statistical_outlier(self, mean_k=50, std_mul=1.0, negative=False, return_distances=False):
        """Indices (input order) PCL's StatisticalOutlierRemoval keeps: mean distance to the mean_k nearest <= mean +
        std_mul * stddev of those means (above it, if negative).  With return_distances: (indices, mean_dist [n], threshold)."""
        if not 1 <= mean_k <= MEAN_K_MAX:
            raise ValueError(f"mean_k must be in 1..{MEAN_K_MAX}")
        out, m = np.empty(max(self.n, 1), np.int32), C.c_int32(0)
        md, thr = np.empty(max(self.n, 1), np.float32), C.c_double(0.0)
        _lib.check(_lib.lib().sfmhip_cloud_statistical_outlier(self.h, int(mean_k), float(std_mul), int(bool(negative)), _p(out),
                                                               C.byref(m), _p(md), C.byref(thr)), "sfmhip_cloud_statistical_outlier")
        kept = out[:m.value].copy()
        return (kept, md[:self.n].copy(), thr.value) if return_distances else kept

    def mls(self, radius, order=2, normals=True, sqr_gauss=0.0, return_cloud=False):
        """PCL's MovingLeastSquares without upsampling: every point moved onto the plane (order 0) or the
        polynomial of order 1 or 2 fitted to its neighbours within `radius`.  A dict with `xyz` [m, 3], `normals` [m, 4] (nx,
        ny, nz, curvature; None without `normals`), `src_index` [m] (the input index of each row: points with fewer than 3
        neighbours and non-finite points are dropped), `stats` (a dict of sfmhip_mls_stats) and `cloud`: with return_cloud, the
        smoothed points as a device cloud that was never on the host, else None."""
        o = MlsOpts(float(radius), int(order), int(bool(normals)), float(sqr_gauss))
        n1 = max(self.n, 1)
        oxyz, onrm, src = np.empty((n1, 3), np.float32), np.empty((n1, 4), np.float32), np.empty(n1, np.int32)
        m, st, h = C.c_int32(0), MlsStats(), C.c_void_p()
        _lib.check(_lib.lib().sfmhip_cloud_mls(self.h, C.addressof(o), _p(oxyz), _p(onrm) if normals else None, _p(src), C.addressof(m),
                                               C.addressof(st), C.byref(h) if return_cloud else None), "sfmhip_cloud_mls")
        return {"xyz": oxyz[:m.value].copy(), "normals": onrm[:m.value].copy() if normals else None, "src_index": src[:m.value].copy(),
                "stats": {k: getattr(st, k) for k, _ in MlsStats._fields_},
                "cloud": Cloud.from_handle(h, self.ctx) if return_cloud else None}

    def mls_last_timing(self):
        """ms of the last mls call (radius grid, fit, compaction) with Context.set_timing on; zeros otherwise."""
        ms = (C.c_double * 3)()
        _lib.check(_lib.lib().sfmhip_cloud_mls_last_timing(self.h, ms), "sfmhip_cloud_mls_last_timing")
        return list(ms)

    def filter_last_timing(self):
        """ms of the last voxel grid (key + sort, reduce) and outlier call (neighbour means, threshold + compaction) with
        Context.set_timing on; zeros otherwise."""
        ms = (C.c_double * 4)()
        _lib.check(_lib.lib().sfmhip_cloud_filter_last_timing(self.h, ms), "sfmhip_cloud_filter_last_timing")
        return list(ms)

    def close(self):
        if self.h:
            _lib.lib().sfmhip_cloud_destroy(self.h)
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


def map3d_step10(xyz, viewpoint=(0.0, 0.0, 0.0), ctx=None):
    """The reference's step 10 on a loaded MAP3D.pcd cloud: cloudPointFilter, removePoints and create_mesh's normals,
    each on the UNFILTERED cloud as map3D passes it.  Returns (passthrough indices, radius-outlier indices, normals
    [n, 4] with the normal negated)."""
    with Cloud(xyz, ctx=ctx) as c:
        keep_pass = c.passthrough(PASS_AXIS, PASS_LO, PASS_HI)
        keep_radius = c.radius_outlier(RADIUS, MIN_PTS)
        nrm = c.normals(K_NORMALS, viewpoint)
    nrm[:, :3] = -nrm[:, :3]
    return keep_pass, keep_radius, nrm
