"""What the mesh-finishing tests share (tests/test_mesh_cpu.py, tests/test_mesh_sanitizers_cpu.py, tests/test_gpu_mesh.py): the
build of the CPU stub (tests/stub/mesh_capi.cpp over csrc/mesh.h) with numpy-facing wrappers, the hand-made meshes, the two
Poisson scenes of the issue, and a plain numpy restatement of the rules M1-M7 of include/sfmhip.h that shares nothing with the
header: a brute-force float32 radius search, the grid's cell ids written out, float64 sums in the written order, a union-find of
its own and the 256-slot tree restated with slices."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "mesh_capi.cpp")
NAN_BITS = 0x7FC00000
OK, ERR_ARG, ERR_STATE = 0, -3, -6
COUNTS = ("n_vertices_in", "n_triangles_in", "n_vertices", "n_triangles", "n_unsupported_vertices", "n_trimmed_triangles", "n_components",
          "n_components_kept")
ARRAYS = ("vertices", "triangles", "normals", "rgb", "support", "nearest", "nearest_d2", "vertex_src", "triangle_src")
THREADS = 16


def build_stub(directory):
    so = str(directory / "libmeshcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp, ci, f64 = C.c_void_p, C.c_int, C.c_double
    lib.msh_finish.argtypes = [ci, vp, vp, ci, vp, ci, vp, f64, ci, ci, ci, ci, ci, C.POINTER(vp)]
    lib.msh_counts.argtypes = [vp, vp, vp]
    lib.msh_counts.restype = None
    lib.msh_get.argtypes = [vp] * 10
    lib.msh_get.restype = None
    lib.msh_free.argtypes = [vp]
    lib.msh_free.restype = None
    lib.msh_sum.argtypes = [vp, ci]
    lib.msh_sum.restype = f64
    return lib


def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def _t(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 3))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def stub_finish(lib, xyz, rgb, verts, tris, radius, min_support=1, min_component=0, keep_largest=0, search=0, threads=THREADS):
    """(status, dict of ARRAYS and "summary" -- the summary's fields by name -- or None on a refusal); rgb None: no colours"""
    xyz, verts, tris = _f(xyz), _f(verts), _t(tris)
    col = None if rgb is None else np.ascontiguousarray(rgb, np.uint32)
    h = C.c_void_p()
    rc = lib.msh_finish(len(xyz), xyz.ctypes.data, None if col is None else col.ctypes.data, len(verts), verts.ctypes.data, len(tris),
                        tris.ctypes.data, float(radius), int(min_support), int(min_component), int(keep_largest), int(search), int(threads),
                        C.byref(h))
    if rc != OK:
        return rc, None
    cnt, sums = np.zeros(8, np.int32), np.zeros(2)
    lib.msh_counts(h, cnt.ctypes.data, sums.ctypes.data)
    nv, nt = int(cnt[2]), int(cnt[3])
    out = {"vertices": np.zeros((nv, 3), np.float32), "triangles": np.zeros((nt, 3), np.int32), "normals": np.zeros((nv, 3), np.float32),
           "rgb": np.zeros(nv, np.uint32), "support": np.zeros(nv, np.int32), "nearest": np.zeros(nv, np.int32),
           "nearest_d2": np.zeros(nv, np.float32), "vertex_src": np.zeros(nv, np.int32), "triangle_src": np.zeros(nt, np.int32)}
    lib.msh_get(h, *(out[k].ctypes.data if out[k].size else None for k in ARRAYS))
    lib.msh_free(h)
    if col is None:
        out["rgb"] = None
    out["summary"] = dict(zip(COUNTS, (int(v) for v in cnt)), area=float(sums[0]), volume=float(sums[1]))
    return rc, out


def stub_sum(lib, x):
    x = np.ascontiguousarray(x, np.float64)
    return float(lib.msh_sum(x.ctypes.data, len(x)))


def same(got, want):
    """every array and every summary field of two results (dicts as stub_finish returns them), bit for bit"""
    assert {k: v for k, v in got["summary"].items() if k in COUNTS} == {k: v for k, v in want["summary"].items() if k in COUNTS}
    for k in ("area", "volume"):
        assert np.float64(got["summary"][k]).view(np.uint64) == np.float64(want["summary"][k]).view(np.uint64), (k, got["summary"][k], want["summary"][k])
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k


# ---- hand-made meshes: (vertices, triangles)

TET_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
TET_T = np.int32([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])          # outward: volume 1/6


def tetrahedron():
    return TET_V.copy(), TET_T.copy()


def two_tetrahedra(shared):
    """two tetrahedra: disjoint (8 vertices), or sharing vertex 3 of the first as vertex 0 of the second (7 vertices)"""
    second = TET_V + np.float32([0, 0, 1] if shared else [3, 0, 0])
    if not shared:
        return np.concatenate([TET_V, second]), np.concatenate([TET_T, TET_T + 4])
    remap = np.int32([3, 4, 5, 6])
    return np.concatenate([TET_V, second[1:]]), np.concatenate([TET_T, remap[TET_T]])


def strip(n_triangles=1000):
    """a wavy strip: two rows of vertices, n_triangles triangles in a zigzag"""
    m = (n_triangles + 1) // 2 + 1
    x = np.arange(m, dtype=np.float64) * 0.01
    lo = np.stack([x, 0 * x, 0.02 * np.sin(7 * x)], 1)
    hi = np.stack([x, 0 * x + 0.01, 0.02 * np.cos(5 * x)], 1)
    v = np.concatenate([lo, hi]).astype(np.float32)
    i = np.arange(m - 1, dtype=np.int32)
    t = np.stack([np.stack([i, i + 1, i + m], 1), np.stack([i + 1, i + m + 1, i + m], 1)], 1).reshape(-1, 3)
    return v, t[:n_triangles].astype(np.int32)


def fan(n_triangles=100):
    """an open fan: vertex 0 in n_triangles triangles over a wavy rim"""
    a = np.linspace(0, 1.9 * np.pi, n_triangles + 1)
    rim = np.stack([0.1 * np.cos(a), 0.1 * np.sin(a), 0.01 * np.sin(9 * a)], 1)
    v = np.concatenate([[[0, 0, 0.02]], rim]).astype(np.float32)
    i = np.arange(1, n_triangles + 1, dtype=np.int32)
    return v, np.stack([0 * i, i, i + 1], 1).astype(np.int32)


def cloud_near(verts, seed, per_vertex=3, spread=0.004):
    """(points, colours): a few points around every vertex, with random colours"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64)
    v = v[np.isfinite(v).all(1)]
    xyz = (np.repeat(v, per_vertex, 0) + rng.uniform(-spread, spread, (len(v) * per_vertex, 3))).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    return xyz, rng.integers(0, 1 << 24, len(xyz), dtype=np.uint32)


# ---- the two Poisson scenes of the issue, through the Poisson CPU stub (tests/test_poisson_cpu.py's)

def capped_sphere(ps):
    """(points, vertices, triangles, h): sphere_cloud(20000, 31) with z > 0.5 cut away, its depth-5 mesh and the cube's cell"""
    from tests.test_poisson_cpu import cg_cap, sphere_cloud, stub_reconstruct
    xyz, nrm = sphere_cloud(20000, 31)
    keep = xyz[:, 2] <= 0.5
    xyz, nrm = xyz[keep], nrm[keep]
    m = stub_reconstruct(ps, xyz, nrm, want_chi=False, depth=5, cg_max_iter=cg_cap(5))
    assert m.iterations < cg_cap(5)
    return xyz, m.verts, m.tris, float(m.h)


def two_spheres(ps):
    """(points, vertices, triangles, h): sphere_cloud(20000, 32) and a sphere of radius 0.15 at x = 1.6, depth 5"""
    from tests.test_poisson_cpu import cg_cap, sphere_cloud, stub_reconstruct
    a, na = sphere_cloud(20000, 32)
    b, nb = sphere_cloud(1500, 33)
    xyz = np.concatenate([a, (0.15 * b + np.float32([1.6, 0, 0])).astype(np.float32)])
    m = stub_reconstruct(ps, xyz, np.concatenate([na, nb]), want_chi=False, depth=5, cg_max_iter=cg_cap(5))   # (ends at the cap: fine here)
    return xyz, m.verts, m.tris, float(m.h)


# ---- the rules in plain numpy

def grid_keys(xyz, radius):
    """M2's order: the cell id of every point (-1: non-finite) in the grid of cells r (1 + 1/1024) over the finite points' box,
    doubled while it exceeds 2^22 cells, axes capped at 2^12, ids x-fastest"""
    x = _f(xyz)
    fin = np.isfinite(x).all(1)
    keys = np.full(len(x), -1, np.int64)
    if not fin.any():
        return keys
    lo, hi = x[fin].min(0).astype(np.float64), x[fin].max(0).astype(np.float64)
    cell = float(radius) * (1.0 + 1.0 / 1024.0)
    while True:
        D = np.minimum(np.floor((hi - lo) / cell) + 1.0, 4096.0).astype(np.int64)
        if D.prod() <= 1 << 22:
            break
        cell *= 2
    c = np.clip(np.floor((x[fin].astype(np.float64) - lo) / cell), 0, D - 1).astype(np.int64)
    keys[fin] = (c[:, 2] * D[1] + c[:, 1]) * D[0] + c[:, 0]
    return keys


def tree_sum(x):
    """M7: consecutive blocks of 256, each by four 64-entry trees (strides 32 .. 1) and (w0 + w1) + (w2 + w3); partials ascending"""
    x = np.asarray(x, np.float64)
    s = np.float64(0.0)
    for b in range(0, len(x), 256):
        v = np.zeros(256)
        v[:len(x[b:b + 256])] = x[b:b + 256]
        w = v.reshape(4, 64).copy()
        off = 32
        while off >= 1:
            w[:, :off] = w[:, :off] + w[:, off:2 * off]
            off //= 2
        s = s + ((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))
    return float(s)


def _cross(a, b, c):
    u, v = b - a, c - a
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def reference_finish(xyz, rgb, verts, tris, radius, min_support=1, min_component=0, keep_largest=0):
    """M1-M7 in numpy; a dict as stub_finish returns it"""
    x32, v32, t = _f(xyz), _f(verts), _t(tris)
    nv, nt = len(v32), len(t)
    summary = dict.fromkeys(COUNTS, 0)
    summary.update(n_vertices_in=nv, n_triangles_in=nt, area=0.0, volume=0.0)
    pfin, vfin = np.isfinite(x32).all(1), np.isfinite(v32).all(1)
    empty = {"vertices": np.zeros((0, 3), np.float32), "triangles": np.zeros((0, 3), np.int32), "normals": np.zeros((0, 3), np.float32),
             "rgb": None if rgb is None else np.zeros(0, np.uint32), "support": np.zeros(0, np.int32), "nearest": np.zeros(0, np.int32),
             "nearest_d2": np.zeros(0, np.float32), "vertex_src": np.zeros(0, np.int32), "triangle_src": np.zeros(0, np.int32), "summary": summary}
    if not pfin.any() or nv == 0:
        summary.update(n_unsupported_vertices=nv, n_trimmed_triangles=nt)
        return empty
    # M2
    keys = grid_keys(x32, radius)
    order = np.lexsort((np.arange(len(x32)), keys))
    order = order[pfin[order]]                                                   # the finite points ascending by (cell id, index)
    r2f = np.float32(float(radius) * float(radius))
    r2d = float(r2f)
    support, nearest = np.zeros(nv, np.int32), np.full(nv, -1, np.int32)
    nd2, colour = np.full(nv, np.inf, np.float32), np.zeros(nv, np.uint32)
    for v in range(nv):
        if not vfin[v]:
            continue
        d = v32[v][None, :] - x32[order]
        d2 = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]       # float32
        hit = d2 < r2f
        support[v] = hit.sum()
        if not hit.any():
            continue
        idx, hd2 = order[hit], d2[hit]
        best = np.lexsort((idx, hd2))[0]
        nearest[v], nd2[v] = idx[best], hd2[best]
        if rgb is not None:
            w = (1.0 - hd2.astype(np.float64) / r2d) ** 2
            col = np.asarray(rgb, np.uint32)[idx]
            sw = sr = sg = sb = np.float64(0.0)
            for k in range(len(idx)):                                            # one written order
                sw = sw + w[k]
                sr = sr + w[k] * float((col[k] >> 16) & 255)
                sg = sg + w[k] * float((col[k] >> 8) & 255)
                sb = sb + w[k] * float(col[k] & 255)
            ch = [min(max(int(s / sw + 0.5), 0), 255) for s in (sr, sg, sb)]
            colour[v] = (ch[0] << 16) | (ch[1] << 8) | ch[2]
    # M3
    sup = vfin & (support >= min_support)
    summary["n_unsupported_vertices"] = int((~sup).sum())
    distinct = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2]) if nt else np.zeros(0, bool)
    tkeep = distinct & sup[t].all(1) if nt else np.zeros(0, bool)
    summary["n_trimmed_triangles"] = int((~tkeep).sum())
    # M4
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b, c in t[tkeep]:
        for p, q in ((a, b), (b, c)):
            p, q = find(p), find(q)
            parent[max(p, q)] = min(p, q)                                        # a root is its set's least member
    comp = np.array([find(a) for a in range(nv)], np.int64)
    size = np.bincount(comp[t[tkeep][:, 0]], minlength=nv) if tkeep.any() else np.zeros(nv, np.int64)
    ids = np.flatnonzero(size > 0)
    summary["n_components"] = len(ids)
    kept = [i for i in ids if size[i] >= min_component]
    if keep_largest > 0:
        kept = sorted(kept, key=lambda i: (-size[i], i))[:keep_largest]
    summary["n_components_kept"] = len(kept)
    tkeep = tkeep & np.isin(comp[t[:, 0]], kept) if nt else tkeep
    # M5
    used = np.zeros(nv, bool)
    used[t[tkeep].reshape(-1)] = True
    vsrc, tsrc = np.flatnonzero(used).astype(np.int32), np.flatnonzero(tkeep).astype(np.int32)
    new = np.cumsum(used) - 1
    ov, ot = v32[vsrc], new[t[tkeep]].astype(np.int32).reshape(-1, 3)
    # M6
    p = ov.astype(np.float64)
    cr = _cross(p[ot[:, 0]], p[ot[:, 1]], p[ot[:, 2]]) if len(ot) else np.zeros((0, 3))
    acc = np.zeros((len(ov), 3))
    for k in range(len(ot)):                                                     # ascending by output triangle
        for q in ot[k]:
            acc[q] = acc[q] + cr[k]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ln = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        nrm = (acc / ln[:, None]).astype(np.float32)
    bad = ~((ln > 0) & np.isfinite(ln))
    nrm.view(np.uint32)[bad] = NAN_BITS
    # M7
    if len(ot):
        a, b, c = p[ot[:, 0]], p[ot[:, 1]], p[ot[:, 2]]
        summary["area"] = tree_sum(0.5 * np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2]))
        bc = np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]], 1)
        summary["volume"] = tree_sum(((a[:, 0] * bc[:, 0] + a[:, 1] * bc[:, 1]) + a[:, 2] * bc[:, 2]) / 6.0)
    summary.update(n_vertices=len(ov), n_triangles=len(ot))
    return {"vertices": ov, "triangles": ot, "normals": nrm, "rgb": None if rgb is None else colour[vsrc], "support": support[vsrc],
            "nearest": nearest[vsrc], "nearest_d2": nd2[vsrc], "vertex_src": vsrc, "triangle_src": tsrc, "summary": summary}
