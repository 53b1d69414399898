"""Finishing a mesh against the device-resident cloud it was made from (include/sfmhip.h, sfmhip_cloud_mesh_finish; rules M1-M7,
DESIGN.md f-24): the trim of the surface no point supports, the drop of small components, per-vertex colours, normals and
nearest points, area and volume.

`finish(cloud, vertices, triangles, rgb, opts)` returns a FinishedMesh; `create_mesh(xyz, rgb)` runs poisson.create_mesh's
steps on one cloud handle and finishes the mesh with support_radius = 1.5 cells of the Poisson cube, the half-width of the
splat's kernel, and min_support = 1.  Nobody has measured that these are good values on real plots."""
import ctypes as C
import warnings
from collections import namedtuple

import numpy as np

from . import _lib, poisson
from .cloud import Cloud


class MeshFinishOpts(C.Structure):
    _fields_ = [("support_radius", C.c_double), ("min_support", C.c_int32), ("min_component_triangles", C.c_int32),
                ("keep_largest", C.c_int32), ("reserved", C.c_int32)]


class MeshFinishSummary(C.Structure):
    _fields_ = [("n_vertices_in", C.c_int32), ("n_triangles_in", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32),
                ("n_unsupported_vertices", C.c_int32), ("n_trimmed_triangles", C.c_int32), ("n_components", C.c_int32),
                ("n_components_kept", C.c_int32), ("area", C.c_double), ("volume", C.c_double)]


FinishedMesh = namedtuple("FinishedMesh", "vertices triangles normals rgb support nearest nearest_d2 vertex_src triangle_src summary")
SUPPORT_CELLS = 1.5   # create_mesh's support radius in cells of the Poisson cube: the half-width of the splat's kernel


def default_opts(**kw):
    """support_radius 0 (it has no default: set it), min_support 1, the component filters off; keyword arguments override fields."""
    o = MeshFinishOpts()
    _lib.lib().sfmhip_mesh_finish_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"no option {k}")
        setattr(o, k, v)
    return o


def _p(a):
    return a.ctypes.data


def finish(cloud, vertices, triangles, rgb=None, opts=None):
    """The mesh (vertices [nv, 3] float32, triangles [nt, 3] int32) finished against `cloud`; rgb: the cloud's colours, one
    0x00RRGGBB per point, or None (the result's rgb is then None)."""
    if opts is None:
        raise ValueError("finish needs options with a support_radius: default_opts(support_radius=...)")
    L = _lib.lib()
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(triangles, np.int32).reshape(-1, 3))
    col = None
    if rgb is not None:
        col = np.ascontiguousarray(np.asarray(rgb, np.uint32).reshape(-1))
        if len(col) != cloud.n:
            raise ValueError("rgb must hold one colour per point of the cloud")
    hin, hout, s = C.c_void_p(), C.c_void_p(), MeshFinishSummary()
    _lib.check(L.sfmhip_mesh_create(_p(v), len(v), _p(t), len(t), C.byref(hin)), "sfmhip_mesh_create")
    try:
        _lib.check(L.sfmhip_cloud_mesh_finish(cloud.h, _p(col) if col is not None else None, hin, C.byref(opts), C.byref(hout), C.byref(s)),
                   "sfmhip_cloud_mesh_finish")
    finally:
        L.sfmhip_mesh_destroy(hin)
    try:
        nv, nt = s.n_vertices, s.n_triangles
        ov, ot = np.zeros((max(nv, 1), 3), np.float32), np.zeros((max(nt, 1), 3), np.int32)
        _lib.check(L.sfmhip_mesh_download(hout, _p(ov), _p(ot)), "sfmhip_mesh_download")
        nrm, orgb = np.zeros((max(nv, 1), 3), np.float32), np.zeros(max(nv, 1), np.uint32)
        sup, near, vsrc = (np.zeros(max(nv, 1), np.int32) for _ in range(3))
        nd2, tsrc = np.zeros(max(nv, 1), np.float32), np.zeros(max(nt, 1), np.int32)
        _lib.check(L.sfmhip_mesh_attributes(hout, _p(nrm), _p(orgb) if col is not None else None, _p(sup), _p(near), _p(nd2), _p(vsrc),
                                            _p(tsrc)), "sfmhip_mesh_attributes")
    finally:
        L.sfmhip_mesh_destroy(hout)
    return FinishedMesh(ov[:nv].copy(), ot[:nt].copy(), nrm[:nv].copy(), orgb[:nv].copy() if col is not None else None, sup[:nv].copy(),
                        near[:nv].copy(), nd2[:nv].copy(), vsrc[:nv].copy(), tsrc[:nt].copy(), s)


def last_timing(cloud):
    """ms of the last finish call on the handle (timing on): search, trim + components, compaction + normals + sums, whole call."""
    ms = np.zeros(4, np.float64)
    _lib.check(_lib.lib().sfmhip_cloud_mesh_last_timing(cloud.h, _p(ms)), "sfmhip_cloud_mesh_last_timing")
    return dict(zip(("search", "components", "compaction", "total"), map(float, ms)))


def create_mesh(xyz, rgb=None, poisson_opts=None, finish_opts=None, ctx=None):
    """poisson.create_mesh's steps (normals with k = 10 and viewpoint 0, flipped, then Poisson with cg_max_iter = 8 * 2^depth),
    then the finishing on the same handle.  Without finish_opts: support_radius = 1.5 * the Poisson summary's cell,
    min_support = 1, the component filters off.  Returns (FinishedMesh, PoissonSummary)."""
    if poisson_opts is None:
        poisson_opts = poisson.default_opts()
        poisson_opts.cg_max_iter = 8 << poisson_opts.depth
    with Cloud(xyz, ctx=ctx) as c:
        nrm = c.normals()
        nrm[:, :3] *= -1.0
        v, t, ps = poisson.reconstruct(c, nrm, poisson_opts)
        cap = poisson_opts.cg_max_iter or 4 << poisson_opts.depth
        if ps.cg_iterations >= cap and ps.cg_relative_residual > poisson_opts.cg_rtol:
            warnings.warn(f"the Poisson solve stopped at its cap of {cap} steps with relative residual "
                          f"{ps.cg_relative_residual:.3e} (cg_rtol {poisson_opts.cg_rtol:.1e})")
        if finish_opts is None:
            finish_opts = default_opts(support_radius=SUPPORT_CELLS * ps.cell if ps.cell > 0 else 1.0)
        return finish(c, v, t, rgb, finish_opts), ps
