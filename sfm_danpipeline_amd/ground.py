"""The ground plane of the device-resident cloud of cloud.py (include/sfmhip.h, sfmhip_cloud_ground_plane):
the vertical frame dendro.py measures in.  A structure-from-motion cloud stands in the first camera's frame, so `up`, `north`
and `ground` have to be found before a height "1.3 m above the ground" means anything.

`ground_plane(cloud, labels, label, opts, cam_centres)` returns a GroundResult (up, north, offset, the counts and flags);
`opts_from_ground(result, dendro_opts)` writes it into a DendroOpts (up, north, ground = offset * scale: the metric scale stays
the caller's); `last_timing(cloud)` the stage times of the last call."""
import ctypes as C

import numpy as np

from . import _lib, dendro

FEW_POINTS, NO_PLANE, REFIT_KEPT, NORTH_REPLACED = 1, 2, 4, 8    # bits of GroundResult.flags


class GroundOpts(C.Structure):
    _fields_ = [("inlier_tol", C.c_double), ("inlier_rel", C.c_double), ("below_max", C.c_double), ("up_hint", C.c_double * 3),
                ("max_tilt_deg", C.c_double), ("north_hint", C.c_double * 3), ("ransac_iters", C.c_int32), ("min_inliers", C.c_int32),
                ("refit_rounds", C.c_int32), ("seed", C.c_uint32)]


class GroundResult(C.Structure):
    _fields_ = [("up", C.c_double * 3), ("north", C.c_double * 3), ("offset", C.c_double), ("rms", C.c_double), ("tol", C.c_double),
                ("n_selected", C.c_int32), ("inliers", C.c_int32), ("below", C.c_int32), ("above", C.c_int32), ("winner", C.c_int32),
                ("flags", C.c_int32)]


def set_opts(o, **kw):
    """Keyword arguments into the fields of a GroundOpts (up_hint / north_hint take three numbers)."""
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no option {k}")
        if k in ("up_hint", "north_hint"):
            v = (C.c_double * 3)(*[float(x) for x in v])
        setattr(o, k, v)
    return o


def default_opts(**kw):
    """Rule 1's defaults (tolerance 0.005 of the box diagonal, 1 % allowed below, no hint, 512 iterations, 2 refits); keyword
    arguments override fields."""
    o = GroundOpts()
    _lib.lib().sfmhip_ground_default_opts(C.byref(o))
    return set_opts(o, **kw)


def ground_plane(cloud, labels=None, label=0, opts=None, cam_centres=None):
    """GroundResult of the points with labels == label (every finite point without labels); cam_centres: [n_cam, 3] camera
    centres in the cloud's frame, which settle which side of the plane is up."""
    opts = opts or default_opts()
    lab, p = dendro._labels(cloud, labels)
    cams, cp, nc = None, None, 0
    if cam_centres is not None:
        cams = np.ascontiguousarray(np.asarray(cam_centres, np.float64).reshape(-1, 3))
        cp, nc = cams.ctypes.data, len(cams)
    out = GroundResult()
    _lib.check(_lib.lib().sfmhip_cloud_ground_plane(cloud.h, p, int(label), C.byref(opts), cp, nc, C.byref(out)), "sfmhip_cloud_ground_plane")
    return out


def opts_from_ground(result, opts=None):
    """The DendroOpts (a fresh default one without `opts`) with up, north and ground = offset * scale from `result`."""
    opts = opts or dendro.default_opts()
    _lib.check(_lib.lib().sfmhip_dendro_opts_from_ground(C.byref(result), C.byref(opts)), "sfmhip_dendro_opts_from_ground")
    return opts


def last_timing(cloud):
    """ms of the last call on the handle: select + bounds, score, refit, whole call."""
    ms = np.zeros(4, np.float64)
    _lib.check(_lib.lib().sfmhip_cloud_ground_last_timing(cloud.h, ms.ctypes.data), "sfmhip_cloud_ground_last_timing")
    return dict(zip(("select", "score", "refit", "total"), map(float, ms)))
