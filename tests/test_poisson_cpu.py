"""CPU: the screened Poisson surface reconstruction of create_mesh's second half, through
tests/stub/poisson_capi.cpp: the g++ build of csrc/poisson.h, the header the HIP kernels are compiled from.

PCL 1.8.1 is absent and its solver is an adaptive octree, so parity is UNPINNED; the contract is the rule list.  It is
checked against (1) an independent scipy restatement of rules 2-6, (2) analytic surfaces, (3) topological invariants and
(4) edge cases.  The bounds are the issue's: V / W / rhs to 1e-12 relative, chi and the iso-value to kappa * cg_rtol
with kappa = (2 N / pi)^2, every vertex within 0.25 h of the analytic surface, closed oriented 2-manifolds with the
surface's Euler characteristic, the depth-6 sphere's volume within 2 %.

Measured with this header (worst vertex distance in h / CG iterations): sphere 20 k depth 5 0.182 / 152, sphere 50 k depth 6
0.155 / 265, with 0.005 noise 0.180 / 265, torus 50 k depth 6 0.185 / 349; scipy restatement: V / W / rhs 2.7e-16, chi 1.8e-8."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "poisson_capi.cpp")
THREADS = min(16, os.cpu_count() or 1)


class PsnOpts(C.Structure):
    _fields_ = [("depth", C.c_int), ("scale", C.c_double), ("point_weight", C.c_double), ("cg_rtol", C.c_double),
                ("cg_max_iter", C.c_int)]


def build_stub(so):
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, f64, ci = C.c_void_p, C.c_double, C.c_int
    lib.psn_bspline.argtypes = [f64]
    lib.psn_bspline.restype = f64
    lib.psn_default_opts.argtypes = [C.POINTER(PsnOpts)]
    lib.psn_default_opts.restype = None
    lib.psn_reconstruct.argtypes = [ci, vp, vp, ci, C.POINTER(PsnOpts), ci, C.POINTER(vp)]
    lib.psn_counts.argtypes = [vp, vp]
    lib.psn_counts.restype = None
    lib.psn_get.argtypes = [vp, vp, vp, vp, vp]
    lib.psn_get.restype = None
    lib.psn_free.argtypes = [vp]
    lib.psn_free.restype = None
    lib.psn_splat.argtypes = [ci, vp, vp, ci, C.POINTER(PsnOpts), ci, vp, vp, vp, vp]
    lib.psn_solve.argtypes = [ci, vp, vp, f64, f64, ci, ci, vp, vp]
    lib.psn_iso.argtypes = [ci, vp, vp, ci, C.POINTER(PsnOpts), ci, vp]
    lib.psn_iso.restype = f64
    lib.psn_extract.argtypes = [ci, vp, f64, vp, f64]
    lib.psn_extract.restype = vp
    lib.psn_sum.argtypes = [vp, ci]
    lib.psn_sum.restype = f64
    lib.psn_ord_keys.argtypes = [ci, vp, vp, vp]
    lib.psn_ord_keys.restype = None
    return lib


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("poisson") / "libpoissoncapi.so"))


# ---------------------------------------------------------------- numpy-facing wrappers (shared with tests/test_gpu_poisson.py)
def opts(ps, **kw):
    o = PsnOpts()
    ps.psn_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _arrays(xyz, nrm):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    nrm = np.asarray(nrm, np.float32)
    nrm = np.ascontiguousarray(nrm.reshape(len(xyz), -1) if len(xyz) else nrm.reshape(0, 3))
    assert nrm.shape[1] in (3, 4)
    return xyz, nrm


class Mesh:
    pass


def _take(ps, h, want_chi=True):
    info = np.zeros(5, np.int32)
    ps.psn_counts(h, info.ctypes.data)
    m = Mesh()
    nv, nt, m.iterations, m.samples, m.N = (int(v) for v in info)
    m.verts = np.zeros((nv, 3), np.float32)
    m.tris = np.zeros((nt, 3), np.int32)
    has_chi = want_chi and m.samples > 0
    m.chi = np.zeros(m.N ** 3 if has_chi else 0)
    d = np.zeros(7)
    ps.psn_get(h, m.verts.ctypes.data, m.tris.ctypes.data, m.chi.ctypes.data if has_chi else None, d.ctypes.data)
    m.iso, m.rr, m.bb, m.origin, m.h = d[0], d[1], d[2], d[3:6].copy(), d[6]
    ps.psn_free(h)
    return m


def stub_reconstruct(ps, xyz, nrm, want_chi=True, **kw):
    xyz, nrm = _arrays(xyz, nrm)
    o = opts(ps, **kw)
    h = C.c_void_p()
    rc = ps.psn_reconstruct(len(xyz), xyz.ctypes.data, nrm.ctypes.data, nrm.shape[1], C.byref(o), THREADS, C.byref(h))
    if rc:
        return rc
    return _take(ps, h, want_chi)


def stub_splat(ps, xyz, nrm, **kw):
    xyz, nrm = _arrays(xyz, nrm)
    o = opts(ps, **kw)
    n3 = (1 << o.depth) ** 3
    V, W, rhs, cube = np.zeros((3, n3)), np.zeros(n3), np.zeros(n3), np.zeros(4)
    m = ps.psn_splat(len(xyz), xyz.ctypes.data, nrm.ctypes.data, nrm.shape[1], C.byref(o), THREADS, V.ctypes.data, W.ctypes.data,
                     rhs.ctypes.data, cube.ctypes.data)
    return V, W, rhs, cube, m


def stub_solve(ps, depth, rhs, W, point_weight=4.0, rtol=1e-8, max_iter=0):
    chi, rb = np.zeros((1 << depth) ** 3), np.zeros(2)
    rhs, W = np.ascontiguousarray(rhs, np.float64), np.ascontiguousarray(W, np.float64)
    it = ps.psn_solve(depth, rhs.ctypes.data, W.ctypes.data, point_weight, rtol, max_iter or 4 << depth, THREADS, chi.ctypes.data,
                      rb.ctypes.data)
    return chi, it, rb


def stub_extract(ps, chi, iso, origin=(0.0, 0.0, 0.0), h=1.0):
    chi = np.ascontiguousarray(chi, np.float64)
    N = chi.shape[0]
    assert chi.shape == (N, N, N)  # [z, y, x]
    o = np.asarray(origin, np.float64)
    return _take(ps, ps.psn_extract(N, chi.ctypes.data, float(iso), o.ctypes.data, float(h)), want_chi=False)


# ---------------------------------------------------------------- clouds and mesh checks (shared with the GPU tests)
def sphere_cloud(n, seed, noise=0.0):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 3))
    nrm = a / np.linalg.norm(a, axis=1, keepdims=True)
    xyz = nrm + (rng.normal(size=(n, 3)) * noise if noise else 0.0)
    return xyz.astype(np.float32), nrm.astype(np.float32)


def torus_cloud(n, seed, R=1.0, r=0.4):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 2 * np.pi, 3 * n)
    v = rng.uniform(0, 2 * np.pi, 3 * n)
    keep = rng.uniform(0, R + r, 3 * n) < R + r * np.cos(v)  # (uniform in area)
    u, v = u[keep][:n], v[keep][:n]
    assert len(u) == n
    nrm = np.c_[np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)]
    xyz = np.c_[R * np.cos(u), R * np.sin(u), np.zeros(n)] + r * nrm
    return xyz.astype(np.float32), nrm.astype(np.float32)


def cg_cap(depth):
    """cg_max_iter of the test cases.  Conjugate gradients reach a relative error eps in about sqrt(kappa) / 2 * ln(2 / eps)
    steps; with kappa = (2 N / pi)^2 and eps = 1e-8 that is 6.1 N, above the default cap of 4 N (which a call may hit: it
    then returns what it has, with the residual in the summary).  The cases run with the next power of two, 8 N, and
    assert that the solve ends before it."""
    return 8 << depth


def sphere_distance(v):
    return np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0)


def torus_distance(v, R=1.0, r=0.4):
    v = v.astype(np.float64)
    return np.abs(np.hypot(np.hypot(v[:, 0], v[:, 1]) - R, v[:, 2]) - r)


def check_closed_oriented(verts, tris, euler):
    """every undirected edge in exactly two triangles, traversed once in each direction; no duplicate vertex; V - E + F"""
    assert len(tris) > 0
    assert tris.min() >= 0 and tris.max() < len(verts)
    assert len(np.unique(tris)) == len(verts), "a vertex no triangle uses"
    assert len(np.unique(verts.view(np.uint32).reshape(-1, 3), axis=0)) == len(verts), "duplicate vertices"
    d = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    assert (d[:, 0] != d[:, 1]).all()
    key = d[:, 0] * len(verts) + d[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge used twice"
    rev = d[:, 1] * len(verts) + d[:, 0]
    assert np.array_equal(np.sort(key), np.sort(rev)), "an edge without its opposite"
    E = len(key) // 2
    assert len(verts) - E + len(tris) == euler


def signed_volume(verts, tris):
    p = verts.astype(np.float64)[tris]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------- 1. the independent oracle
def scipy_oracle(xyz, nrm, depth, scale=1.1, point_weight=4.0):
    """rules 2-6 restated with np.add.at, a Kronecker Laplacian and a direct solve"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    p, nv = xyz.astype(np.float64), nrm.astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    side = scale * (hi - lo).max()
    N = 1 << depth
    h = side / N
    origin = (lo + hi) / 2 - side / 2
    u = (p - origin) / h - 0.5
    base = np.floor(u + 0.5).astype(int)

    def B(t):
        a = np.abs(t)
        return np.where(a < 0.5, 0.75 - a * a, np.where(a < 1.5, 0.5 * (1.5 - a) ** 2, 0.0))
    V, W = np.zeros((3, N, N, N)), np.zeros((N, N, N))  # [z, y, x]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                c = base + [dx, dy, dz]
                ok = ((c >= 0) & (c < N)).all(1)
                w = (B(u - c)).prod(1)[ok]
                ix = (c[ok, 2], c[ok, 1], c[ok, 0])
                np.add.at(W, ix, w)
                for a in range(3):
                    np.add.at(V[a], ix, w * nv[ok, a])
    div = np.zeros((N, N, N))
    for a, ax in ((0, 2), (1, 1), (2, 0)):  # (component a varies along array axis ax)
        pad = np.pad(V[a], 1)
        sl = [slice(1, -1)] * 3
        up, dn = list(sl), list(sl)
        up[ax], dn[ax] = slice(2, None), slice(0, -2)
        div += (pad[tuple(up)] - pad[tuple(dn)]) / 2
    rhs = -div
    T = sp.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
    I = sp.identity(N)
    L = sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)
    A = (L + point_weight * sp.diags(W.ravel())).tocsc()
    chi = spsolve(A, rhs.ravel()).reshape(N, N, N)
    # trilinear chi at the samples
    padc = np.pad(chi, 1)  # index + 1; one layer of zeros is enough (samples lie inside the cube)
    i0 = np.floor(u).astype(int)
    f = u - i0
    val = np.zeros(len(p))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                val += w * padc[i0[:, 2] + dz + 1, i0[:, 1] + dy + 1, i0[:, 0] + dx + 1]
    return V.reshape(3, -1), W.ravel(), rhs.ravel(), chi.ravel(), val.mean(), origin, h


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_bspline_is_the_quadratic_partition_of_unity(ps):
    t = np.linspace(-2, 2, 4001)
    b = np.array([ps.psn_bspline(float(x)) for x in t])
    assert (b[np.abs(t) >= 1.5] == 0).all() and b.max() == 0.75
    s = np.array([sum(ps.psn_bspline(float(x) - k) for k in (-2, -1, 0, 1, 2)) for x in np.linspace(-0.5, 0.5, 101)])
    assert np.abs(s - 1).max() < 1e-15


def test_ord_keys_match_the_rule_both_headers_spelled(ps):
    from tests.test_segment_cpu import check_ord_keys
    check_ord_keys(ps.psn_ord_keys)


def test_fixed_order_sum_is_a_sum(ps):
    rng = np.random.default_rng(0)
    for n in (1, 63, 256, 257, 70001):
        v = rng.normal(size=n)
        assert abs(ps.psn_sum(v.ctypes.data, n) - np.sum(v)) <= 1e-13 * np.abs(v).sum()


def test_against_the_scipy_restatement(ps):
    depth, N = 5, 32
    xyz, nrm = sphere_cloud(6000, 3)
    xyz = xyz * [1.0, 0.8, 0.6] + [0.3, -0.2, 0.1]  # (no symmetry for an axis mix-up to hide behind)
    xyz = xyz.astype(np.float32)
    Vo, Wo, ro, chio, isoo, origin, h = scipy_oracle(xyz, nrm, depth)
    V, W, rhs, cube, m = stub_splat(ps, xyz, nrm, depth=depth)
    assert m == len(xyz)
    assert np.abs(cube[:3] - origin).max() < 1e-14 and abs(cube[3] - h) < 1e-15
    print("V / W / rhs relative error:", _rel(V, Vo), _rel(W, Wo), _rel(rhs, ro))
    assert _rel(V, Vo) <= 1e-12 and _rel(W, Wo) <= 1e-12 and _rel(rhs, ro) <= 1e-12
    rtol = 1e-8
    kappa = (2 * N / np.pi) ** 2
    res = stub_reconstruct(ps, xyz, nrm, depth=depth, cg_rtol=rtol, cg_max_iter=cg_cap(depth))
    print("chi relative error:", _rel(res.chi, chio), "bound", kappa * rtol, "iterations", res.iterations,
          "iso", res.iso, isoo)
    assert res.iterations < cg_cap(depth)
    assert np.sqrt(res.rr / res.bb) <= rtol
    assert _rel(res.chi, chio) <= kappa * rtol
    assert abs(res.iso - isoo) <= kappa * rtol * abs(isoo)
    # the staged entries are the whole call's stages
    chi2, it2, rb = stub_solve(ps, depth, rhs, W, rtol=rtol, max_iter=cg_cap(depth))
    assert it2 == res.iterations and np.array_equal(chi2, res.chi)


# ---------------------------------------------------------------- 2 + 3. analytic surfaces and topology
CASES = {
    "sphere-d5": (lambda: sphere_cloud(20000, 1), 5, sphere_distance, 2),
    "sphere-d6": (lambda: sphere_cloud(50000, 2), 6, sphere_distance, 2),
    "sphere-d6-noise": (lambda: sphere_cloud(50000, 2, noise=0.005), 6, sphere_distance, 2),
    "torus-d6": (lambda: torus_cloud(50000, 4), 6, torus_distance, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_analytic_surface(ps, name):
    make, depth, dist, euler = CASES[name]
    xyz, nrm = make()
    res = stub_reconstruct(ps, xyz, nrm, want_chi=False, depth=depth, cg_max_iter=cg_cap(depth))
    d = dist(res.verts) / res.h
    vol = signed_volume(res.verts, res.tris)
    print(f"{name}: worst vertex distance {d.max():.4f} h, mean {d.mean():.4f} h, {res.iterations} iterations, "
          f"{len(res.verts)} vertices, {len(res.tris)} triangles, volume {vol:.5f}")
    assert res.iterations < cg_cap(depth)
    assert d.max() <= 0.25
    check_closed_oriented(res.verts, res.tris, euler)
    assert vol > 0
    if name == "sphere-d6":
        assert abs(vol / (4 * np.pi / 3) - 1) <= 0.02


def _sines(n, seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n) / n] * 3, indexing="ij"), -1)
    f = np.zeros((n, n, n))
    for _ in range(12):
        k = rng.integers(1, 4, 3) * rng.choice([-1, 1], 3)
        f += rng.normal() * np.sin(2 * np.pi * (g @ k) + rng.uniform(0, 2 * np.pi))
    return f


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_extraction_is_watertight_on_random_fields(ps, seed):
    """The extraction entry alone on a sum of random low-frequency sines on a 24^3 grid: every tetrahedron case and every
    orientation of the split occurs.  The field is pushed above the iso-value on the boundary layer, so the surface stays
    off the boundary and must close."""
    n = 24
    f = _sines(n, seed)
    iso = float(np.median(f))
    edge = np.ones((n, n, n), bool)
    edge[1:-1, 1:-1, 1:-1] = False
    f[edge] = iso + 1.0 + np.abs(f[edge])
    res = stub_extract(ps, f, iso, origin=(0.5, -1.0, 2.0), h=0.25)
    assert len(res.tris) > 1000
    d = np.concatenate([res.tris[:, [0, 1]], res.tris[:, [1, 2]], res.tris[:, [2, 0]]]).astype(np.int64)
    key, rev = d[:, 0] * len(res.verts) + d[:, 1], d[:, 1] * len(res.verts) + d[:, 0]
    assert len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))
    assert len(np.unique(res.tris)) == len(res.verts)
    assert len(np.unique(res.verts.view(np.uint32).reshape(-1, 3), axis=0)) == len(res.verts)
    # outward winding: the enclosed volume is the inside (f < iso) region's, counted in cells
    vol = signed_volume(res.verts, res.tris) / 0.25 ** 3
    cells = float((f < iso).sum())
    print(f"seed {seed}: {len(res.verts)} vertices, {len(res.tris)} triangles, volume {vol:.1f} cells, inside points {cells:.0f}")
    assert vol > 0 and abs(vol / cells - 1) < 0.1


def test_every_triangle_faces_the_outside(ps):
    """normals point towards chi > iso: on a linear field the triangles' normals are the gradient's direction"""
    n = 8
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    for grad in ([1, 0, 0], [0, -1, 0], [0.3, 0.5, -0.8], [-1, -1, -1], [0.2, -0.9, 0.4]):
        f = grad[0] * x + grad[1] * y + grad[2] * z
        res = stub_extract(ps, f, float(np.median(f)) + 0.013)
        p = res.verts.astype(np.float64)[res.tris]
        nn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert len(nn) > 0 and (nn @ np.asarray(grad, np.float64) > 0).all()


# ---------------------------------------------------------------- 4. edge cases
def test_edge_cases(ps):
    xyz, nrm = sphere_cloud(500, 5)
    res = stub_reconstruct(ps, xyz[:0], nrm[:0], depth=4)
    assert (res.samples, len(res.verts), len(res.tris)) == (0, 0, 0)
    res = stub_reconstruct(ps, xyz[:1], nrm[:1], depth=4)  # one sample: a valid (tiny, closed or empty) mesh
    assert res.samples == 1 and res.h == 1.0 / 16
    if len(res.tris):
        assert res.tris.max() < len(res.verts)
    res = stub_reconstruct(ps, xyz, np.full_like(nrm, np.nan), depth=4)
    assert (res.samples, len(res.verts), len(res.tris)) == (0, 0, 0)
    same = np.repeat(xyz[:1], 50, 0)
    res = stub_reconstruct(ps, same, nrm[:50], depth=4)
    assert res.samples == 50 and res.h == 1.0 / 16 and np.isfinite(res.chi).all() and np.isfinite(res.verts).all()
    for depth in (0, 9, -1):
        assert stub_reconstruct(ps, xyz, nrm, depth=depth) == -3
    for kw in (dict(scale=0.5), dict(point_weight=-1.0), dict(cg_rtol=1.0), dict(cg_max_iter=-1), dict(scale=float("nan"))):
        assert stub_reconstruct(ps, xyz, nrm, depth=4, **kw) == -3


def test_unusable_rows_are_skipped(ps):
    xyz, nrm = sphere_cloud(3000, 6)
    bad = nrm.copy()
    rows = np.arange(0, 3000, 7)
    bad[rows[0::3], 1] = np.nan
    bad[rows[1::3], 0] = np.inf
    bad[rows[2::3]] = 0.0
    xyz2 = xyz.copy()
    xyz2[5] = [np.nan, 0, 0]
    keep = np.ones(3000, bool)
    keep[rows] = False
    keep[5] = False
    a = stub_reconstruct(ps, xyz2, bad, depth=5)
    b = stub_reconstruct(ps, xyz[keep], nrm[keep], depth=5)
    assert a.samples == b.samples == keep.sum()
    assert np.array_equal(a.verts, b.verts) and np.array_equal(a.tris, b.tris) and a.iso == b.iso
    # the 4-float layout of the normals call gives the same bytes as the 3-float one
    c = stub_reconstruct(ps, xyz2, np.c_[bad, np.full(3000, 0.25, np.float32)], depth=5)
    assert np.array_equal(a.verts, c.verts) and np.array_equal(a.tris, c.tris)


def test_thread_count_does_not_change_a_bit(ps):
    xyz, nrm = sphere_cloud(4000, 7)
    o = opts(ps, depth=5)
    out = []
    for threads in (1, 3, 16):
        h = C.c_void_p()
        assert ps.psn_reconstruct(len(xyz), xyz.ctypes.data, nrm.ctypes.data, 3, C.byref(o), threads, C.byref(h)) == 0
        out.append(_take(ps, h))
    for r in out[1:]:
        assert np.array_equal(r.chi, out[0].chi) and r.iso == out[0].iso and r.iterations == out[0].iterations
        assert np.array_equal(r.verts, out[0].verts) and np.array_equal(r.tris, out[0].tris)
