"""GPU: map3D's step 10 (reference src/Sfm.cpp:94-102, :1323-1383) -- sfmhip_cloud_* bit for bit against the CPU build
of the same header (tests/stub/cloud_capi.cpp over csrc/cloud.h, with a spatial search of its own) on 50 k, 200 k and
1 M point clouds, independent agreement with scipy's cKDTree, the grid's edge regimes, handle reuse, and the host
mirror's steps 8-10 end to end.  PARITY UNPINNED: PCL is not in the image."""
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from sfm_danpipeline_amd import _lib, build, cloud
from tests.test_cloud_cpu import (STUB, load_stub, stub_counts, stub_knn, stub_normals, stub_outlier, stub_passthrough,
                                  surface_cloud)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cloud") / "libcloudcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def bench_cloud(n, seed=0):
    """Surfaces plus 5 % uniform outliers, scaled so that r = 0.07 holds a few hundred neighbours at any n."""
    return surface_cloud(n, seed, outliers=0.05, scale=3.0 * np.sqrt(n / 1e6))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_all(ctx, cc, xyz, radius=0.07, min_pts=150, k=10, vp=(0, 0, 0), pass_args=(0, 0.003, 0.83)):
    with cloud.Cloud(xyz, ctx=ctx) as c:
        exact = c.radius_count(radius)
        assert np.array_equal(exact, stub_counts(cc, xyz, radius))
        assert np.array_equal(c.radius_count(radius, cap=min_pts + 1), np.minimum(exact, min_pts + 1))
        assert np.array_equal(c.radius_outlier(radius, min_pts), stub_outlier(cc, xyz, radius, min_pts))
        ax, lo, hi = pass_args
        assert np.array_equal(c.passthrough(ax, lo, hi), stub_passthrough(cc, xyz, ax, lo, hi))
        assert np.array_equal(c.passthrough(ax, lo, hi, negative=True), stub_passthrough(cc, xyz, ax, lo, hi, True))
        idx, d2 = c.knn(k)
        si, sd = stub_knn(cc, xyz, k)
        assert np.array_equal(idx, si)
        assert np.array_equal(bits(d2), bits(sd))
        nrm = c.normals(k, vp)
        assert np.array_equal(bits(nrm), bits(stub_normals(cc, xyz, k, vp)))
    return exact, idx, d2, nrm


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [50_000, 200_000, 1_000_000])
def test_device_equals_the_header_build_and_scipy(ctx, cc, n):
    xyz = bench_cloud(n, seed=n % 7)
    exact, idx, d2, nrm = check_all(ctx, cc, xyz)
    assert 150 <= np.median(exact) <= 600                          # (the regime the reference's constants are for)
    # independent: scipy's k-d tree in double, on the points clear of the radius / the k-th distance
    t = cKDTree(xyz.astype(np.float64))
    x64 = xyz.astype(np.float64)
    sel = np.random.default_rng(1).choice(n, 20_000, replace=False)
    lo = t.query_ball_point(x64[sel], 0.07 * (1 - 1e-5), return_length=True, workers=16)
    hi = t.query_ball_point(x64[sel], 0.07 * (1 + 1e-5), return_length=True, workers=16)
    clear = lo == hi
    assert clear.mean() > 0.95 and np.array_equal(exact[sel][clear], lo[clear])
    dd, ii = t.query(x64[sel], k=11, workers=16)
    gap = (dd[:, 10] - dd[:, 9]) > 1e-5 * np.maximum(dd[:, 9], 1e-12)     # the 10 nearest are a well-defined set
    assert gap.mean() > 0.9
    for r in np.nonzero(gap)[0][:5000]:
        assert set(idx[sel[r]]) == set(ii[r, :10])
    assert np.allclose(np.sqrt(d2[sel[gap]]), dd[gap, :10], rtol=1e-5, atol=1e-6)
    assert np.isfinite(nrm).all(1).mean() > 0.99


def test_grid_regimes(ctx, cc):
    rng = np.random.default_rng(3)
    base = surface_cloud(20_000, 4, scale=0.5)
    far = np.concatenate([base, [[1e6, 0.2, 0.2]]]).astype(np.float32)             # one far outlier: clamped, not a huge grid
    check_all(ctx, cc, far, k=10)
    check_all(ctx, cc, base[:3000], radius=5.0, min_pts=2000, k=32)               # everything in one cell
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (300, 1))                       # all points identical
    _, idx, d2, nrm = check_all(ctx, cc, same, min_pts=299, k=10)
    assert list(idx[7]) == list(range(10)) and (d2 == 0).all()
    assert (bits(nrm[:, :3]) == 0x7FC00000).all() and (nrm[:, 3] == 0).all()
    for n in (0, 1, 2):                                                              # tiny clouds
        xyz = rng.uniform(0, 0.01, (n, 3)).astype(np.float32)
        for k in (1, 10, 32):
            check_all(ctx, cc, xyz, min_pts=1, k=k)
    for k in (1, 10, 32):                                                            # k = 1, 10, 32 and k > n
        check_all(ctx, cc, base[:k + 7] if k > 10 else base[:5000], k=k)
        check_all(ctx, cc, base[:max(k - 3, 1)], k=k)
    bad = base[:5000].copy()                                                         # non-finite points
    bad[::50, 0] = np.nan
    bad[3::70, 1] = np.inf
    bad[5::90, 2] = -np.inf
    _, idx, d2, nrm = check_all(ctx, cc, bad, k=10)
    assert (idx[::50] == -1).all() and np.isinf(d2[::50]).all() and (bits(nrm[::50]) == 0x7FC00000).all()
    assert not np.isin(idx, np.nonzero(~np.isfinite(bad).all(1))[0]).any()


def test_pairs_straddling_cell_faces_are_counted(ctx, cc):
    r = 0.07
    c = r * (1 + 2.0 ** -10)             # the radius grid's cell (cloud.hip), from the smallest coordinate, which is 0 here
    d = r * (1 - 2.0 ** -20)
    pts = [[0.0, 0.0, 0.0]]
    dirs = [np.array(v, float) / np.linalg.norm(v) for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1], [1, -1, 1])]
    j = 0
    for a in range(2, 14, 2):
        for b in range(2, 14, 2):
            for e in (2, 6, 10):
                v = dirs[j % len(dirs)]
                j += 1
                ctr = np.array([a, b, e], float) * c                                    # a cell corner: faces on every axis
                p, q = np.float32(ctr - v * d / 2), np.float32(ctr + v * d / 2)
                ax = int(np.argmax(np.abs(v)))
                while cc.cloud_dist2(*map(float, p), *map(float, q)) >= np.float32(r * r):   # (float coordinates: an ulp in)
                    q[ax] = np.nextafter(q[ax], p[ax])
                pts += [p, q]
    xyz = np.array(pts, np.float32)
    d2 = np.array([cc.cloud_dist2(*map(float, xyz[i]), *map(float, xyz[i + 1])) for i in range(1, len(xyz), 2)], np.float32)
    assert (d2 < np.float32(r * r)).all() and (d2 > np.float32((r * (1 - 2.0 ** -17)) ** 2)).all()
    with cloud.Cloud(xyz, ctx=ctx) as cl:
        got = cl.radius_count(r)
    assert got[0] == 1 and (got[1:] == 2).all()
    assert np.array_equal(got, stub_counts(cc, xyz, r))


def test_compaction_at_block_boundaries(ctx, cc):
    """Flags, scan, total, scatter around the scan's and the launches' block sizes: the n - 1 reads and the last block."""
    rng = np.random.default_rng(12)
    for n in (1, 2, 63, 64, 65, 256, 257, 1025):
        xyz = rng.uniform(0, 0.01, (n, 3)).astype(np.float32)
        xyz[:, 2] = np.where(np.arange(n) % 2 == 0, 0.5, 2.0)                       # z alternates inside / outside [0, 1]
        bad = xyz.copy()
        bad[-1, 1] = np.inf                                                          # a non-finite last point: never kept
        with cloud.Cloud(xyz, ctx=ctx) as c, cloud.Cloud(bad, ctx=ctx) as cb:
            for lo, hi, want in ((-10.0, 10.0, np.arange(n)), (5.0, 6.0, np.arange(0)), (0.0, 1.0, np.arange(0, n, 2))):
                got = c.passthrough(2, lo, hi)
                assert np.array_equal(got, want) and np.array_equal(got, stub_passthrough(cc, xyz, 2, lo, hi))
                assert np.array_equal(cb.passthrough(2, lo, hi), stub_passthrough(cc, bad, 2, lo, hi))
            assert np.array_equal(cb.passthrough(2, -10.0, 10.0), np.arange(n - 1))
            kept = c.radius_outlier(5.0, 0)                                          # every point has itself within 5: all kept
            assert np.array_equal(kept, np.arange(n)) and np.array_equal(kept, stub_outlier(cc, xyz, 5.0, 0))
            assert np.array_equal(cb.radius_outlier(5.0, 0), stub_outlier(cc, bad, 5.0, 0))


def test_handle_reuse_and_two_handles(ctx, cc):
    a = bench_cloud(60_000, seed=2)
    b = bench_cloud(30_000, seed=5)
    ca, cb = cloud.Cloud(a, ctx=ctx), cloud.Cloud(b, ctx=ctx)
    try:
        for r, k in ((0.05, 5), (0.07, 10), (0.1, 32), (0.07, 10), (0.05, 1)):
            for c, x in ((ca, a), (cb, b)):
                with cloud.Cloud(x, ctx=ctx) as fresh:
                    assert np.array_equal(c.radius_count(r), fresh.radius_count(r))
                    assert np.array_equal(c.radius_outlier(r, 150), fresh.radius_outlier(r, 150))
                    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(c.knn(k), fresh.knn(k)))
                    assert np.array_equal(bits(c.normals(k)), bits(fresh.normals(k)))
        assert np.array_equal(ca.radius_count(0.07), stub_counts(cc, a, 0.07))
        assert np.array_equal(bits(cb.normals(10)), bits(stub_normals(cc, b, 10)))
    finally:
        ca.close()
        cb.close()


def test_argument_refusals(ctx):
    L = _lib.lib()
    with cloud.Cloud(np.zeros((4, 3), np.float32), ctx=ctx) as c:
        out, m = np.zeros(8, np.int32), np.zeros(1, np.int32)
        f = np.zeros(8 * 33, np.float32)
        vp = np.zeros(3, np.float32)
        assert L.sfmhip_cloud_passthrough(c.h, 3, 0.0, 1.0, 0, out.ctypes.data, m.ctypes.data) == -3
        assert L.sfmhip_cloud_radius_count(c.h, 0.0, 0, out.ctypes.data) == -3
        assert L.sfmhip_cloud_radius_count(c.h, float("nan"), 0, out.ctypes.data) == -3
        assert L.sfmhip_cloud_radius_outlier(c.h, 0.07, -1, out.ctypes.data, m.ctypes.data) == -3
        assert L.sfmhip_cloud_knn(c.h, 0, out.ctypes.data, f.ctypes.data) == -3
        assert L.sfmhip_cloud_knn(c.h, 33, out.ctypes.data, f.ctypes.data) == -3
        assert L.sfmhip_cloud_normals(c.h, 10, None, f.ctypes.data) == -3
        assert L.sfmhip_cloud_normals(c.h, 10, vp.ctypes.data, None) == -3
    assert L.sfmhip_cloud_create(ctx.h, -1, None, None) == -3
    with pytest.raises(ValueError):
        cloud.Cloud(np.zeros((1, 3)), ctx=ctx).knn(40)


def _write_ply(path, xyz):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar diffuse_red\nproperty uchar diffuse_green\n"
            "property uchar diffuse_blue\nend_header\n" % len(xyz))
    rec = np.zeros(len(xyz), np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    rec["p"] = xyz
    path.write_bytes(head.encode() + rec.tobytes())


def _read_driver(path):
    b = open(path, "rb").read()
    o, out = 0, []
    for w in (3, 3, 3, 4):
        n = struct.unpack_from("<i", b, o)[0]
        o += 4
        out.append(np.frombuffer(b, np.float32, n * w, o).reshape(n, w))
        o += 4 * n * w
    return out


@pytest.mark.timeout(600)
def test_cpp_driver_steps_8_to_10(ctx, cc, tmp_path):
    xyz = surface_cloud(40_000, 8, scale=0.9)                   # x straddles [0.003, 0.83]; dense enough for 150 neighbours
    _write_ply(tmp_path / "options.txt.ply", xyz)
    exe = build.build_cloud_demo()
    r = subprocess.run([exe, str(tmp_path / "options.txt.ply"), str(tmp_path), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    loaded, passed, kept, nrm = _read_driver(tmp_path / "out.bin")
    assert (tmp_path / "MAP3D.pcd").exists()
    p8 = np.array([np.float32("%.8g" % v) for v in xyz.ravel()], np.float32).reshape(xyz.shape)   # the PCD's 8 digits
    assert np.array_equal(loaded, p8)
    keep_pass, keep_radius, want = cloud.map3d_step10(loaded, ctx=ctx)
    assert 0 < len(keep_pass) < len(loaded) and 0 < len(keep_radius) < len(loaded)
    assert np.array_equal(passed, loaded[keep_pass]) and np.array_equal(kept, loaded[keep_radius])
    assert np.array_equal(keep_pass, stub_passthrough(cc, loaded)) and np.array_equal(keep_radius, stub_outlier(cc, loaded))
    assert np.array_equal(bits(nrm), bits(want))
    stub = stub_normals(cc, loaded, 10)
    stub[:, :3] = -stub[:, :3]
    assert np.array_equal(bits(nrm), bits(stub))
    # the reference's quirk: create_mesh reads the unfiltered cloud -- one normal per loaded point, not per kept point
    assert len(nrm) == len(loaded) != len(kept)
