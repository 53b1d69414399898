"""GPU: the Poisson surface reconstruction (sfmhip_cloud_poisson and its staged entries, csrc/poisson.hip) against the
g++ build of the same header (tests/stub/poisson_capi.cpp), bit for bit: V, W, the right-hand side, chi, the CG
iteration count, the iso-value, vertices and triangles; then the analytic and topological checks of
tests/test_poisson_cpu.py on the device's mesh, and the C++ host mirror's create_mesh.  No test provokes a fault."""
import subprocess
import time

import numpy as np
import pytest

from sfm_danpipeline_amd import build, cloud, poisson
from tests.test_cloud_cpu import surface_cloud
from tests.test_poisson_cpu import (build_stub, cg_cap, check_closed_oriented, signed_volume, sphere_cloud, sphere_distance,
                                    stub_extract, stub_reconstruct, stub_solve, stub_splat, torus_cloud, torus_distance, _sines)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("poisson") / "libpoissoncapi.so"))


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(ctx, ps, xyz, nrm, depth, staged=True):
    """the device against the header's host build on one cloud; returns (device mesh, summary, stub result, times)"""
    kw = dict(depth=depth, cg_max_iter=cg_cap(depth))
    with cloud.Cloud(xyz, ctx=ctx) as c:
        v, t, s = poisson.reconstruct(c, nrm, poisson.default_opts(**kw))
        t0 = time.perf_counter()
        v2, t2, s2 = poisson.reconstruct(c, nrm, poisson.default_opts(**kw))      # a repeat on the handle: the same bytes
        gpu_s = time.perf_counter() - t0                                          # (the timed call is the warm one)
        tm = poisson.last_timing(c)
        assert _same(v, v2) and _same(t, t2) and s.iso_value == s2.iso_value and s.cg_iterations == s2.cg_iterations
        if staged:
            V, W, rhs, ss = poisson.splat(c, nrm, poisson.default_opts(**kw))
    t0 = time.perf_counter()
    ref = stub_reconstruct(ps, xyz, nrm, **kw)
    cpu_s = time.perf_counter() - t0
    print(f"depth {depth}, {len(xyz)} points: {s.n_samples} samples, {s.cg_iterations} iterations, relres "
          f"{s.cg_relative_residual:.3e}, {s.n_vertices} vertices, {s.n_triangles} triangles; device {gpu_s:.3f} s {tm}, "
          f"host build on {min(16, __import__('os').cpu_count())} threads {cpu_s:.3f} s")
    assert (s.n_samples, s.cg_iterations, s.grid) == (ref.samples, ref.iterations, ref.N)
    assert s.iso_value == ref.iso and s.cell == ref.h and list(s.origin) == list(ref.origin)
    assert s.cg_relative_residual == np.sqrt(ref.rr / ref.bb)
    assert _same(v, ref.verts) and _same(t, ref.tris)
    if staged:
        Vr, Wr, rr, cube, m = stub_splat(ps, xyz, nrm, **kw)
        assert _same(V, Vr) and _same(W, Wr) and _same(rhs, rr) and ss.n_samples == m
        chi, it, rb = poisson.solve(depth, rhs, W, cg_max_iter=cg_cap(depth), ctx=ctx)
        assert it == ref.iterations and _same(chi, ref.chi) and rb[0] == ref.rr and rb[1] == ref.bb
    if depth == 7:  # (the size the pipeline runs at; below it a call is launch overhead)
        assert gpu_s < cpu_s, "the device call is slower than the header's host build on 16 threads"
    return v, t, s, ref


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("depth", [5, 6, 7])
@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_device_equals_the_header_build(ctx, ps, shape, depth):
    xyz, nrm = sphere_cloud(50000, 11) if shape == "sphere" else torus_cloud(50000, 12)
    _compare(ctx, ps, xyz, nrm, depth)


@pytest.mark.timeout(2400)
@pytest.mark.parametrize("n", [200_000, 1_000_000])
@pytest.mark.parametrize("depth", [5, 6, 7])
def test_device_equals_the_header_build_on_a_scanned_cloud(ctx, ps, n, depth):
    """surface_cloud (a sphere, a plane, a wavy sheet and 5 % outliers) with the normals of sfmhip_cloud_normals in
    their own 4-float layout, flipped as create_mesh flips them; some normals are NaN (fewer than 3 neighbours never
    happens here, so a few rows are spoilt by hand)."""
    xyz = surface_cloud(n, 21)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        nrm = c.normals()
    nrm[:, :3] *= -1.0
    nrm[::997, 0] = np.nan
    xyz[5] = [np.nan, 0, 0]
    _compare(ctx, ps, xyz, nrm, depth)


@pytest.mark.timeout(1500)
def test_depth7_sphere_geometry_and_topology(ctx, ps):
    xyz, nrm = sphere_cloud(200_000, 13)
    v, t, s, ref = _compare(ctx, ps, xyz, nrm, 7, staged=False)
    d = sphere_distance(v) / s.cell
    vol = signed_volume(v, t)
    print(f"depth 7 sphere: worst vertex distance {d.max():.4f} h, mean {d.mean():.4f} h, volume {vol:.5f}")
    assert s.cg_iterations < cg_cap(7)
    assert d.max() <= 0.25
    check_closed_oriented(v, t, 2)
    assert vol > 0 and abs(vol / (4 * np.pi / 3) - 1) <= 0.02


@pytest.mark.timeout(900)
def test_depth6_torus_geometry_and_topology(ctx):
    xyz, nrm = torus_cloud(50000, 4)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        v, t, s = poisson.reconstruct(c, nrm, poisson.default_opts(depth=6, cg_max_iter=cg_cap(6)))
    assert (torus_distance(v) / s.cell).max() <= 0.25
    check_closed_oriented(v, t, 0)
    assert signed_volume(v, t) > 0


@pytest.mark.timeout(600)
def test_extraction_entry_equals_the_header_build(ctx, ps):
    for seed in (0, 1):
        f = _sines(24, seed)
        iso = float(np.median(f))
        v, t = poisson.extract(f, iso, origin=(0.5, -1.0, 2.0), cell=0.25, ctx=ctx)
        ref = stub_extract(ps, f, iso, origin=(0.5, -1.0, 2.0), h=0.25)
        assert len(t) > 1000 and _same(v, ref.verts) and _same(t, ref.tris)


@pytest.mark.timeout(600)
def test_edge_cases_and_refusals(ctx, ps):
    xyz, nrm = sphere_cloud(500, 5)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        v, t, s = poisson.reconstruct(c, np.full_like(nrm, np.nan), poisson.default_opts(depth=4))
        assert (len(v), len(t), s.n_samples) == (0, 0, 0)
        for kw in (dict(depth=0), dict(depth=9), dict(scale=0.5), dict(point_weight=-1.0), dict(cg_rtol=1.0), dict(cg_max_iter=-1)):
            with pytest.raises(Exception, match="status -3"):
                poisson.reconstruct(c, nrm, poisson.default_opts(**kw))
        for depth in (1, 2, 3):  # bricks smaller than a workgroup
            v, t, s = poisson.reconstruct(c, nrm, poisson.default_opts(depth=depth))
            ref = stub_reconstruct(ps, xyz, nrm, depth=depth)
            assert _same(v, ref.verts) and _same(t, ref.tris) and s.iso_value == ref.iso and s.cg_iterations == ref.iterations
    for pts, nr in ((xyz[:0], nrm[:0]), (xyz[:1], nrm[:1]), (np.repeat(xyz[:1], 50, 0), nrm[:50])):
        with cloud.Cloud(pts, ctx=ctx) as c:
            v, t, s = poisson.reconstruct(c, nr, poisson.default_opts(depth=4))
        ref = stub_reconstruct(ps, pts, nr, depth=4)
        assert s.n_samples == len(pts) and _same(v, ref.verts) and _same(t, ref.tris)


def _write_pcd(path, xyz):
    head = (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
            f"WIDTH {len(xyz)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(xyz)}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes())


def read_ply_mesh(path):
    """a binary little-endian PLY with float x y z vertices and `list uchar int vertex_indices` faces"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    v = np.frombuffer(raw, "<f4", 3 * nv, end).reshape(nv, 3)
    rec = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nf, end + 12 * nv)
    assert len(raw) == end + 12 * nv + 13 * nf and (rec["n"] == 3).all()
    return v.copy(), rec["v"].copy()


@pytest.mark.timeout(900)
def test_cpp_driver_create_mesh(ctx, tmp_path):
    """sfm_mesh_selftest: loadPCDFile -> StructFromMotion::create_mesh (computeNormals, the -1 flip, Poisson at depth 7,
    point weight 4, scale 1.1) -> a binary PLY; the mesh is the Python path's, and a closed oriented sphere."""
    exe = build.build_mesh_demo()
    xyz, _ = sphere_cloud(60000, 17)
    xyz = (xyz * 0.5).astype(np.float32)  # (around the viewpoint at 0: the normals face it, the flipped ones point outwards)
    _write_pcd(tmp_path / "MAP3D.pcd", xyz)
    r = subprocess.run([exe, str(tmp_path / "MAP3D.pcd"), str(tmp_path / "mesh.ply")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    v, t = read_ply_mesh(tmp_path / "mesh.ply")
    pv, pt, s = poisson.create_mesh(xyz, ctx=ctx)
    assert s.grid == 128 and _same(v, pv) and _same(t, pt)
    check_closed_oriented(v, t, 2)
    assert signed_volume(v, t) > 0
