"""The second half of StructFromMotion::create_mesh (reference src/Sfm.cpp:1365-1381: pcl::Poisson at depth 7, point
weight 4, scale 1.1 on the cloud and its flipped normals) on the GPU, over the device-resident cloud of cloud.py
(include/sfmhip.h, sfmhip_cloud_poisson and its staged entries).

`reconstruct(cloud, normals)` returns (vertices [nv, 3] float32, triangles [nt, 3] int32, PoissonSummary);
`create_mesh(xyz)` runs the reference's call: the normals of the cloud (k = 10, viewpoint 0), flipped, then Poisson.
Parity with PCL is UNPINNED: a uniform grid for PCL's octree, marching tetrahedra for its cubes."""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from .cloud import Cloud


class PoissonOpts(C.Structure):
    _fields_ = [("depth", C.c_int32), ("scale", C.c_double), ("point_weight", C.c_double), ("cg_rtol", C.c_double),
                ("cg_max_iter", C.c_int32), ("normal_stride", C.c_int32)]


class PoissonSummary(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("cg_iterations", C.c_int32),
                ("cg_relative_residual", C.c_double), ("iso_value", C.c_double), ("origin", C.c_double * 3), ("cell", C.c_double),
                ("grid", C.c_int32)]


def default_opts(**kw):
    """The reference's setters (depth 7, point weight 4, scale 1.1), cg_rtol 1e-8, cg_max_iter 0 = 4 * 2^depth;
    keyword arguments override fields."""
    o = PoissonOpts()
    _lib.lib().sfmhip_poisson_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no option {k}")
        setattr(o, k, v)
    return o


def _p(a):
    return a.ctypes.data


def _normals(cloud, normals, opts):
    """normals as [n, 3] or [n, 4] float32 (the layout Cloud.normals returns); the stride goes into the options"""
    nrm = np.asarray(normals, np.float32)
    nrm = np.ascontiguousarray(nrm.reshape(cloud.n, -1) if cloud.n else nrm.reshape(0, 3))
    if nrm.shape[1] not in (3, 4):
        raise ValueError("normals must be [n, 3] or [n, 4]")
    opts.normal_stride = nrm.shape[1]
    return nrm


def _mesh(h):
    L = _lib.lib()
    try:
        nv, nt = C.c_int32(0), C.c_int32(0)
        _lib.check(L.sfmhip_mesh_counts(h, C.byref(nv), C.byref(nt)), "sfmhip_mesh_counts")
        v, t = np.zeros((max(nv.value, 1), 3), np.float32), np.zeros((max(nt.value, 1), 3), np.int32)
        _lib.check(L.sfmhip_mesh_download(h, _p(v), _p(t)), "sfmhip_mesh_download")
        return v[:nv.value].copy(), t[:nt.value].copy()
    finally:
        L.sfmhip_mesh_destroy(h)


def reconstruct(cloud, normals, opts=None):
    """(vertices, triangles, PoissonSummary) of the cloud with the given normals (rows with a non-finite or zero normal
    are skipped, as non-finite points are)."""
    opts = opts or default_opts()
    nrm = _normals(cloud, normals, opts)
    h, s = C.c_void_p(), PoissonSummary()
    _lib.check(_lib.lib().sfmhip_cloud_poisson(cloud.h, _p(nrm), C.byref(opts), C.byref(h), C.byref(s)), "sfmhip_cloud_poisson")
    v, t = _mesh(h)
    return v, t, s


def splat(cloud, normals, opts=None):
    """Rules 1-4 alone: (V [3, N^3], W [N^3], rhs [N^3] float64, PoissonSummary with the cube)."""
    opts = opts or default_opts()
    nrm = _normals(cloud, normals, opts)
    n3 = (1 << opts.depth) ** 3
    V, W, rhs, s = np.zeros((3, n3)), np.zeros(n3), np.zeros(n3), PoissonSummary()
    _lib.check(_lib.lib().sfmhip_cloud_poisson_splat(cloud.h, _p(nrm), C.byref(opts), _p(V), _p(W), _p(rhs), C.byref(s)),
               "sfmhip_cloud_poisson_splat")
    return V, W, rhs, s


def solve(depth, rhs, W, point_weight=4.0, cg_rtol=1e-8, cg_max_iter=0, ctx=None):
    """Rule 5 from a given right-hand side: (chi [N^3], iterations, (final, initial) squared residual)."""
    ctx = ctx or _lib.default_context()
    n3 = (1 << depth) ** 3
    rhs, W = np.ascontiguousarray(rhs, np.float64).reshape(-1), np.ascontiguousarray(W, np.float64).reshape(-1)
    if len(rhs) != n3 or len(W) != n3:
        raise ValueError("rhs and W must hold N^3 values")
    chi, it, rb = np.zeros(n3), C.c_int32(0), np.zeros(2)
    _lib.check(_lib.lib().sfmhip_poisson_solve(ctx.h, int(depth), _p(rhs), _p(W), float(point_weight), float(cg_rtol), int(cg_max_iter),
                                               _p(chi), C.byref(it), _p(rb)), "sfmhip_poisson_solve")
    return chi, it.value, rb


def extract(chi, iso, origin=(0.0, 0.0, 0.0), cell=1.0, ctx=None):
    """Rule 7 from a given field [n, n, n] (z, y, x): (vertices, triangles)."""
    ctx = ctx or _lib.default_context()
    chi = np.ascontiguousarray(chi, np.float64)
    n = chi.shape[0]
    if chi.shape != (n, n, n):
        raise ValueError("chi must be [n, n, n]")
    o, h = np.asarray(origin, np.float64), C.c_void_p()
    _lib.check(_lib.lib().sfmhip_poisson_extract(ctx.h, n, _p(chi), float(iso), _p(o), float(cell), C.byref(h)), "sfmhip_poisson_extract")
    return _mesh(h)


def last_timing(cloud):
    """ms of the last reconstruct call on the handle: samples + splat, solve, iso-value + extraction, whole call."""
    ms = np.zeros(4, np.float64)
    _lib.check(_lib.lib().sfmhip_cloud_poisson_last_timing(cloud.h, _p(ms)), "sfmhip_cloud_poisson_last_timing")
    return dict(zip(("splat", "solve", "extraction", "total"), map(float, ms)))


def create_mesh(xyz, opts=None, ctx=None):
    """The reference's create_mesh on a loaded cloud: computeNormals (k = 10, viewpoint 0), every normal times -1, then
    Poisson.  Returns (vertices, triangles, PoissonSummary).  Without options the solve runs as the host mirror's does:
    cg_max_iter = 8 * 2^depth, since the default of 4 * 2^depth steps does not reach cg_rtol at depth 7;
    a solve that still ends at its cap is warned about with its residual."""
    if opts is None:
        opts = default_opts()
        opts.cg_max_iter = 8 << opts.depth
    with Cloud(xyz, ctx=ctx) as c:
        nrm = c.normals()
        nrm[:, :3] *= -1.0
        v, t, s = reconstruct(c, nrm, opts)
    cap = opts.cg_max_iter or 4 << opts.depth
    if s.cg_iterations >= cap and s.cg_relative_residual > opts.cg_rtol:
        warnings.warn(f"the Poisson solve stopped at its cap of {cap} steps with relative residual "
                      f"{s.cg_relative_residual:.3e} (cg_rtol {opts.cg_rtol:.1e})")
    return v, t, s
