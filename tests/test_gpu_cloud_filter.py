"""GPU: VoxelGrid and StatisticalOutlierRemoval on the device-resident cloud (sfmhip_cloud_voxel_grid,
sfmhip_cloud_statistical_outlier, sfmhip_cloud_select / _download) bit for bit against the CPU build of the
same header (tests/stub/cloud_filter_capi.cpp over csrc/cloud_filter.h, with a sort and a neighbour search of its own), at
the shapes each kernel can go wrong at; the chain voxel grid -> outlier removal -> selection -> normals without a trip
through the host against the same chain through host arrays; the refusals through the ABI; the host mirror's driver."""
import struct
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, cloud
from tests.test_cloud_filter_cpu import (ERR_ARG, ERR_UNSUPPORTED, OK, bits, build_stub, stub_sor, stub_voxel_grid, surface_cloud)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


@pytest.fixture(scope="module")
def cf(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("cloud_filter"))


def check_voxel_grid(ctx, cf, xyz, leaf, min_points=0, rgb=None, normals=None):
    rc, want = stub_voxel_grid(cf, xyz, leaf, min_points, rgb, normals)
    assert rc == OK
    with cloud.Cloud(xyz, ctx=ctx) as c:
        got = c.voxel_grid(leaf, min_points, rgb=rgb, normals=normals, return_cloud=True)
        assert len(got["xyz"]) == len(want["xyz"]) and got["cloud"].n == len(want["xyz"])
        assert np.array_equal(bits(got["xyz"]), bits(want["xyz"]))
        assert np.array_equal(got["voxel_of"], want["voxel_of"])
        if rgb is not None:
            assert np.array_equal(got["rgb"], want["rgb"])
        if normals is not None:
            assert np.array_equal(bits(got["normals"]), bits(want["normals"]))
        assert np.array_equal(bits(got["cloud"].download()), bits(want["xyz"]))         # the handle born on the device
        got["cloud"].close()
    return got


def check_sor(ctx, cf, xyz, mean_k, std_mul=1.0):
    """both signs against the stub; returns the device's (kept, mean_dist, threshold) of the positive call"""
    with cloud.Cloud(xyz, ctx=ctx) as c:
        for negative in (True, False):
            rc, kept, md, thr = stub_sor(cf, xyz, mean_k, std_mul, negative)
            assert rc == OK
            gk, gmd, gthr = c.statistical_outlier(mean_k, std_mul, negative, return_distances=True)
            assert np.array_equal(bits(gmd), bits(md))
            assert struct.pack("<d", gthr) == struct.pack("<d", thr)
            assert np.array_equal(gk, kept)
    return gk, gmd, gthr


def attributes(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm[::37] = np.nan
    return rng.integers(0, 1 << 32, n, dtype=np.uint32), nrm


@pytest.fixture(scope="module")
def cloud20k():
    xyz = surface_cloud(20_000, 21)
    xyz[np.random.default_rng(5).choice(20_000, 200, replace=False), 0] = np.nan       # 1 % NaN
    return xyz


def test_voxel_grid_tiny_and_long_runs(ctx, cf):
    rng = np.random.default_rng(1)
    for n in (0, 1, 2):
        xyz = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        rgb, nrm = attributes(n, n)
        for leaf in (0.01, 10.0):
            check_voxel_grid(ctx, cf, xyz, leaf, rgb=rgb, normals=nrm)
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (300, 1))                          # one run over five blocks
    rgb, nrm = attributes(300, 3)
    nrm[::37] = 1.0
    out = check_voxel_grid(ctx, cf, same, 0.1, rgb=rgb, normals=nrm)
    assert len(out["xyz"]) == 1 and (out["voxel_of"] == 0).all()
    # a voxel of exactly 64 points (a lane's sum) and one of exactly 65 (the wave's), interleaved in input order, among others
    a = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.4, 0.4, (64, 3)).astype(np.float32)
    b = np.float32([1.5, 0.5, 0.5]) + rng.uniform(-0.4, 0.4, (65, 3)).astype(np.float32)
    rest = rng.uniform(2.0, 9.0, (500, 3)).astype(np.float32)
    xyz = np.concatenate([a, b, rest])[rng.permutation(629)]
    rgb, nrm = attributes(629, 4)
    out = check_voxel_grid(ctx, cf, xyz, 1.0, rgb=rgb, normals=nrm)
    assert sorted(np.bincount(out["voxel_of"]))[-2:] == [64, 65]
    check_voxel_grid(ctx, cf, xyz, 1.0, min_points=65)
    check_voxel_grid(ctx, cf, np.concatenate([xyz, [[np.nan, 0, 0]]]).astype(np.float32), 20.0, rgb=np.r_[rgb, 7].astype(np.uint32))


@pytest.mark.parametrize("leaf", [0.02, 0.05])
def test_voxel_grid_on_surfaces(ctx, cf, cloud20k, leaf):
    rgb, nrm = attributes(len(cloud20k), 6)
    out = check_voxel_grid(ctx, cf, cloud20k, leaf, rgb=rgb, normals=nrm)
    assert 1.5 < np.isfinite(cloud20k).all(1).sum() / len(out["xyz"]) < 12            # about 2 and 8 points per voxel
    for mp in (2, 3):
        check_voxel_grid(ctx, cf, cloud20k, (leaf, 2 * leaf, leaf), min_points=mp)


def test_voxel_grid_keys_of_31_bits(ctx, cf):
    rng = np.random.default_rng(8)
    xyz = np.concatenate([[[0, 0, 0]], rng.uniform(0, 1289.5, (1000, 3)), [[1289.5] * 3]]).astype(np.float32)
    xyz[500:520] = xyz[480:500] + np.float32(0.001)                                    # some shared voxels
    out = check_voxel_grid(ctx, cf, xyz, 1.0)                                          # 1290^3 = 2 146 689 000 voxels
    assert out["voxel_of"][-1] == len(out["xyz"]) - 1 and out["voxel_of"][0] == 0


def test_voxel_grid_over_several_workgroups(ctx, cf):
    xyz = surface_cloud(200_000, 23)
    xyz[::1000, 1] = np.inf
    xyz[:3000] = xyz[3000] + np.float32(1e-4) * np.random.default_rng(2).uniform(0, 1, (3000, 3)).astype(np.float32)  # a long run too
    rgb, nrm = attributes(len(xyz), 9)
    check_voxel_grid(ctx, cf, xyz, 0.01, rgb=rgb, normals=nrm)


@pytest.mark.parametrize("mean_k", [1, 8, 31, 32, 63])
def test_outlier_removal_equals_the_header_build(ctx, cf, cloud20k, mean_k):
    check_sor(ctx, cf, cloud20k[:3000], mean_k)
    kept, md, thr = check_sor(ctx, cf, cloud20k, mean_k)
    assert 0.8 * len(cloud20k) < len(kept) < len(cloud20k) and thr > 0


def test_outlier_removal_edge_regimes(ctx, cf, cloud20k):
    base = cloud20k[np.isfinite(cloud20k).all(1)]
    for mean_k in (1, 16, 63):
        check_sor(ctx, cf, base[:mean_k + 1], mean_k)                                  # n = mean_k + 1
    check_sor(ctx, cf, base[:40] * np.float32(1e-3), 16)                               # everything in one cell
    far = np.concatenate([base[:5000], [[1e6, 0.2, 0.2]]]).astype(np.float32)           # a far outlier: the clamped border cell
    kept, md, _ = check_sor(ctx, cf, far, 16)
    assert 5000 not in kept and md[5000] > 1e5
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (300, 1))
    kept, md, thr = check_sor(ctx, cf, same, 16)
    assert np.array_equal(kept, np.arange(300)) and thr == 0.0 and (md == 0).all()
    check_sor(ctx, cf, cloud20k[:4000], 8, std_mul=0.0)
    with cloud.Cloud(np.full((3, 3), np.nan, np.float32), ctx=ctx) as c:               # nothing finite
        kept, md, thr = c.statistical_outlier(8, return_distances=True)
        assert len(kept) == 0 and (md == 0).all() and thr == 0.0
    with cloud.Cloud(np.zeros((0, 3), np.float32), ctx=ctx) as c:
        assert len(c.statistical_outlier(8)) == 0


def test_chain_stays_on_the_device(ctx, cf, cloud20k):
    with cloud.Cloud(cloud20k, ctx=ctx) as c:
        before = c.radius_count(0.05)
        vg = c.voxel_grid(0.02, return_cloud=True)
        thin = vg["cloud"]
        assert thin.xyz is None and thin.n == len(vg["xyz"])
        kept = thin.statistical_outlier(16, 1.0)
        sel = thin.select(kept)
        nrm = sel.normals(10)
        assert sel.xyz is None and sel.n == len(kept)
        # the same chain through host arrays
        with cloud.Cloud(vg["xyz"], ctx=ctx) as h1:
            kept_h = h1.statistical_outlier(16, 1.0)
            with cloud.Cloud(vg["xyz"][kept_h], ctx=ctx) as h2:
                nrm_h = h2.normals(10)
                assert np.array_equal(h2.radius_count(0.05), sel.radius_count(0.05))
        assert np.array_equal(kept, kept_h) and 0 < len(kept) < thin.n
        assert np.array_equal(bits(nrm), bits(nrm_h))
        assert np.array_equal(bits(sel.download()), bits(vg["xyz"][kept]))
        dup = thin.select([5, 5, 0, thin.n - 1])                                        # duplicates allowed, order kept
        assert np.array_equal(bits(dup.download()), bits(vg["xyz"][[5, 5, 0, thin.n - 1]]))
        assert thin.select([]).n == 0
        assert np.array_equal(c.radius_count(0.05), before)                            # the original handle still answers
        assert np.array_equal(bits(c.select(np.arange(c.n)).download()), bits(cloud20k))
        assert c.filter_last_timing() == [0.0] * 4                                     # timing is off


def test_refusals_through_the_abi(ctx):
    L = _lib.lib()
    f32, i32 = np.float32, np.int32
    leaf = np.ones(3, f32)
    for pts, lf, status in ((f32([[0, 0, 0], [1290.5] * 3]), leaf, ERR_UNSUPPORTED), (f32([[3e9, 0, 0], [3e9, 1, 1]]), leaf, ERR_UNSUPPORTED),
                            (f32([[0, 0, 0], [2e7, 0, 0]]), leaf, ERR_UNSUPPORTED), (f32([[0, 0, 0], [1, 1, 1]]), f32([1, 0, 1]), ERR_ARG),
                            (f32([[0, 0, 0], [1, 1, 1]]), f32([1, np.nan, 1]), ERR_ARG)):
        with cloud.Cloud(pts, ctx=ctx) as c:
            oxyz, vox, m = np.full((2, 3), 7.5, f32), np.full(2, 77, i32), np.full(1, -9, i32)
            h = _lib.C.c_void_p()
            rc = L.sfmhip_cloud_voxel_grid(c.h, lf.ctypes.data, 0, None, None, oxyz.ctypes.data, None, None, vox.ctypes.data, m.ctypes.data,
                                           _lib.C.byref(h))
            assert rc == status and (oxyz == 7.5).all() and (vox == 77).all() and m[0] == -9 and not h.value
    with cloud.Cloud(surface_cloud(16, 1), ctx=ctx) as c:
        idx, m, md, thr = np.full(16, -7, i32), np.full(1, -9, i32), np.full(16, 7.5, f32), np.full(1, 7.5)
        args = (idx.ctypes.data, m.ctypes.data, md.ctypes.data, thr.ctypes.data)
        assert L.sfmhip_cloud_statistical_outlier(c.h, 16, 1.0, 0, *args) == ERR_ARG    # n = mean_k
        assert L.sfmhip_cloud_statistical_outlier(c.h, 0, 1.0, 0, *args) == ERR_ARG
        assert L.sfmhip_cloud_statistical_outlier(c.h, 64, 1.0, 0, *args) == ERR_ARG
        assert L.sfmhip_cloud_statistical_outlier(c.h, 8, float("nan"), 0, *args) == ERR_ARG
        assert (idx == -7).all() and m[0] == -9 and (md == 7.5).all() and thr[0] == 7.5
        assert L.sfmhip_cloud_voxel_grid(c.h, leaf.ctypes.data, -1, None, None, None, None, None, None, m.ctypes.data, None) == ERR_ARG
        h = _lib.C.c_void_p()
        for bad in ([16], [-1], [0, 3, 99]):
            b = i32(bad)
            assert L.sfmhip_cloud_select(c.h, b.ctypes.data, len(b), _lib.C.byref(h)) == ERR_ARG and not h.value
        assert L.sfmhip_cloud_download(c.h, None) == ERR_ARG and L.sfmhip_cloud_size(None, None, None) == ERR_ARG
        n, nv = _lib.C.c_int32(0), _lib.C.c_int32(0)
        assert L.sfmhip_cloud_size(c.h, _lib.C.byref(n), _lib.C.byref(nv)) == OK and (n.value, nv.value) == (16, 16)
        with pytest.raises(ValueError):
            c.statistical_outlier(64)


def test_timing_is_reported_when_on(ctx, cloud20k):
    with cloud.Cloud(cloud20k, ctx=ctx) as c:
        ctx.set_timing(True)
        try:
            c.voxel_grid(0.02)
            c.statistical_outlier(16)
            ms = c.filter_last_timing()
        finally:
            ctx.set_timing(False)
        assert all(0 < t < 5000 for t in ms)
        c.voxel_grid(0.02)
        assert c.filter_last_timing()[:2] == [0.0, 0.0]


def _write_pcd(path, xyz):
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
            "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (len(xyz), len(xyz)))
    path.write_bytes(head.encode() + np.ascontiguousarray(xyz, np.float32).tobytes())


def _read_pcd(path, width):
    b = open(path, "rb").read()
    o = b.index(b"DATA binary\n") + len(b"DATA binary\n")
    return np.frombuffer(b, np.float32, offset=o).reshape(-1, width)


def test_mirror_driver_equals_the_python_chain(ctx, cloud20k, tmp_path):
    xyz = cloud20k[:8000]
    _write_pcd(tmp_path / "in.pcd", xyz)
    exe = build.build_cloud_filter_demo()
    r = subprocess.run([exe, str(tmp_path / "in.pcd"), "0.03", "16", "1.0", str(tmp_path / "out.pcd")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _read_pcd(tmp_path / "out.pcd", 7)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        thin = c.voxel_grid(0.03, return_cloud=True)["cloud"]
        sel = thin.select(thin.statistical_outlier(16, 1.0))
        want = np.c_[sel.download(), sel.normals(10)]
        want[:, 3:6] = -want[:, 3:6]                                                    # computeNormals is create_mesh's: negated
    assert r.stdout.split() == ["points", "8000", "voxels", str(thin.n), "kept", str(sel.n)]
    assert np.array_equal(bits(got), bits(want))
