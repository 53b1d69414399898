"""GPU: the colour region growing after map3D and Dendrometry's bounds (reference src/Segmentation.cpp:3-66,
src/DendrometryE.cpp:3-29) -- sfmhip_cloud_segment_* / sfmhip_cloud_minmax bit for bit against the CPU build of the same
header (tests/stub/segment_capi.cpp over csrc/segment.h: a search of its own, the literal queue growth) on 50 k, 200 k
and 1 M point scenes, the subset k-NN against scipy's cKDTree, handle reuse, and the host mirror's Segmentation /
Dendrometry classes end to end.  PARITY UNPINNED: PCL is not in the image."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from sfm_danpipeline_amd import _lib, build, cloud, segment
from tests.test_segment_cpu import (STUB, load_stub, passthrough_z, patch_scene, ref_opts, stub_grow, stub_minmax, stub_segment,
                                    stub_subset_knn)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("segment") / "libsegmentcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene(n, seed):
    """The patch scene with points outside the z limits and a few non-finite ones, so the index list is a proper subset."""
    xyz, rgb, patch, is_salt = patch_scene(n, seed, salt=0.03, close=True)
    xyz[::53, 2] += 14.0
    xyz[5::977, 0] = np.nan
    return xyz, rgb


def check_all(ctx, sc, xyz, rgb, ind, **kw):
    o = ref_opts(**kw)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        assert np.isin(ind, c.passthrough("z", 0.0, 14.0)).all()                  # (the PassThrough's list, or a part of it)
        k = o["region_neighbour_number"]
        idx, d2 = segment.subset_knn(c, ind, k)
        si, sd = stub_subset_knn(sc, xyz, ind, k)
        assert np.array_equal(idx, si)
        assert np.array_equal(bits(d2), bits(sd))
        seg, ns, rounds = segment.grow(c, rgb, ind, segment.default_opts(**kw))
        sseg, sns = stub_grow(sc, xyz, rgb, ind, o)
        assert ns == sns and np.array_equal(seg, sseg)
        labels, nc, st = segment.segment_rgb(c, rgb, ind, segment.default_opts(**kw))
        slabels, snc, sstats, _ = stub_segment(sc, xyz, rgb, ind, o)
        assert nc == snc and np.array_equal(labels, slabels)                      # the clusters and their order
        assert [st.n_idx, st.n_segments, st.n_regions] == list(sstats[:3]) and st.rounds >= 1 and rounds >= 1   # (rounds vary: atomics)
        mn, mx, h = segment.minmax(c)
        smn, smx, sh = stub_minmax(sc, xyz)
        assert np.array_equal(bits(mn), bits(smn)) and np.array_equal(bits(mx), bits(smx)) and h == sh
    return idx, d2, labels, nc, st


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("n", [50_000, 200_000, 1_000_000])
def test_device_equals_the_header_build_and_scipy(ctx, sc, n):
    xyz, rgb = scene(n, seed=n % 7)
    ind = passthrough_z(xyz)
    assert 0.97 * n < len(ind) < n
    with cloud.Cloud(xyz, ctx=ctx) as c:
        assert np.array_equal(c.passthrough("z", 0.0, 14.0), ind)
    idx, d2, labels, nc, st = check_all(ctx, sc, xyz, rgb, ind)
    assert nc >= 5 and st.n_segments > 0.02 * n                                    # the patches; the salt's own segments
    # independent: scipy's k-d tree in double over the indexed points, on the rows whose 100 nearest are a well-defined set
    pts = xyz[ind].astype(np.float64)
    sel = np.random.default_rng(1).choice(len(ind), 20_000, replace=False)
    dd, ii = cKDTree(pts).query(pts[sel], k=101, workers=16)
    gap = (dd[:, 100] - dd[:, 99]) > 1e-5 * np.maximum(dd[:, 99], 1e-12)
    assert gap.mean() >= 0.9
    rows = np.nonzero(gap)[0]
    assert np.array_equal(np.sort(idx[sel[rows]], 1), np.sort(ind[ii[rows, :100]], 1))
    assert np.allclose(np.sqrt(d2[sel[rows]]), dd[rows, :100], rtol=1e-5, atol=1e-6)
    assert np.array_equal(idx[:, 0], ind) and (np.diff(d2, axis=1) >= 0).all()


def test_small_and_odd_lists(ctx, sc):
    xyz, rgb = scene(3000, 3)
    ind = passthrough_z(xyz)
    check_all(ctx, sc, xyz, rgb, ind, min_cluster_size=100)
    st = check_all(ctx, sc, xyz, rgb, ind, min_cluster_size=100, point_color_threshold=1.5)[4]   # fragments that rule 8 joins again
    assert st.n_regions < 0.8 * st.n_segments
    check_all(ctx, sc, xyz, rgb, ind[::3], min_cluster_size=30, region_neighbour_number=128, neighbour_number=128)
    check_all(ctx, sc, xyz[:80], rgb[:80], passthrough_z(xyz[:80]), min_cluster_size=5)     # n_idx < 100
    check_all(ctx, sc, xyz[:300], rgb[:300], passthrough_z(xyz[:300]), min_cluster_size=5, region_neighbour_number=1, neighbour_number=1)
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (300, 1))                                # all points identical: ties by index
    check_all(ctx, sc, same, rgb[:300], np.arange(300, dtype=np.int32), min_cluster_size=1)
    far = np.concatenate([xyz, [[1e6, 0.2, 0.2]]]).astype(np.float32)                        # one far point: clamped cells
    check_all(ctx, sc, far, np.append(rgb, 0), passthrough_z(far), min_cluster_size=100)


def test_handle_reuse(ctx, sc):
    xyz, rgb = scene(40_000, 4)
    ind = passthrough_z(xyz)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        nrm = c.normals(10)
        a = segment.segment_rgb(c, rgb, ind)                                                 # after normals, on one handle
        b = segment.segment_rgb(c, rgb, ind[ind % 3 != 0])                                   # another index list
        a2 = segment.segment_rgb(c, rgb, ind)
        assert np.array_equal(bits(c.normals(10)), bits(nrm))
        t = segment.last_timing(c)
    assert np.array_equal(a[0], a2[0]) and a[1] == a2[1]
    assert np.array_equal(a[0], stub_segment(sc, xyz, rgb, ind, ref_opts())[0])
    assert np.array_equal(b[0], stub_segment(sc, xyz, rgb, ind[ind % 3 != 0], ref_opts())[0])
    assert (b[0][::3] == -1).all() and b[2].n_idx == len(ind[ind % 3 != 0])
    assert t["total"] > 0 and abs(t["knn"] + t["growth"] + t["statistics"] + t["regions"] - t["total"]) < 1e-6 * max(t["total"], 1)


def test_argument_refusals(ctx):
    L = _lib.lib()
    xyz, rgb = scene(50, 1)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        o = segment.default_opts()
        lab, m = np.zeros(64, np.int32), np.zeros(4, np.int32)
        good = np.array([1, 2, 3], np.int32)

        def call(ind, n, opts):
            return L.sfmhip_cloud_segment_rgb(c.h, rgb.ctypes.data, ind.ctypes.data, n, C.byref(opts), lab.ctypes.data, m.ctypes.data, None)

        assert call(good, 3, o) == 0
        assert call(good, 0, o) == -3                                                        # an empty list
        assert call(np.array([3, 2, 1], np.int32), 3, o) == -3                               # not ascending
        assert call(np.array([1, 2, 50], np.int32), 3, o) == -3                              # out of range
        assert call(good, 3, segment.default_opts(region_neighbour_number=129)) == -3
        assert call(good, 3, segment.default_opts(min_cluster_size=0)) == -3
        f = np.zeros(3 * 130, np.float32)
        assert L.sfmhip_cloud_subset_knn(c.h, good.ctypes.data, 3, 129, lab.ctypes.data, f.ctypes.data) == -3
        assert L.sfmhip_cloud_minmax(c.h, None, f.ctypes.data, None) == -3
    with pytest.raises(ValueError):
        segment.subset_knn(cloud.Cloud(xyz, ctx=ctx), good, 200)


def _write_pcd(path, xyz, rgb):
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
            "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (len(xyz), len(xyz)))
    rec = np.zeros(len(xyz), np.dtype([("p", "<f4", 3), ("c", "<u4")]))
    rec["p"], rec["c"] = xyz, rgb
    path.write_bytes(head.encode() + rec.tobytes())


@pytest.mark.timeout(600)
def test_cpp_driver_segmentation_and_dendrometry(ctx, sc, tmp_path):
    xyz, rgb = scene(30_000, 6)
    xyz[np.isnan(xyz[:, 0]), 0] = 0.5                                                        # (a binary PCD of finite points)
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, rgb)
    exe = build.build_segment_demo()
    r = subprocess.run([exe, str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    b = (tmp_path / "out.bin").read_bytes()
    n, nc = struct.unpack_from("<ii", b, 0)
    labels = np.frombuffer(b, np.int32, n, 8)
    mn, mx = np.frombuffer(b, np.float32, 3, 8 + 4 * n), np.frombuffer(b, np.float32, 3, 20 + 4 * n)
    h = struct.unpack_from("<d", b, 32 + 4 * n)[0]
    want, wnc, st = segment.color_based_growing_segmentation(xyz, rgb, ctx=ctx)
    assert n == len(xyz) and nc == wnc >= 5 and np.array_equal(labels, want)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        wmn, wmx, wh = segment.minmax(c)
    assert np.array_equal(bits(mn), bits(wmn)) and np.array_equal(bits(mx), bits(wmx)) and h == wh
    assert np.array_equal(wmn, xyz.min(0)) and np.array_equal(wmx, xyz.max(0))
    out = r.stdout
    assert "COLOR BASE GROWING SEGMENTATION" in out and "Input cloud:%d\n" % n in out and "Extract:%d clusters\n" % nc in out
    assert "Distance threshold:10\nPoint color threshold:6\nRegion color threshold:5\nClusters size:600\n" in out
    assert "DENDROMETRY ESTIMATION" in out and "Total Height =" in out and "Altura DAP=1.3\n" in out
    # an empty cloud is reported, not exited on
    (tmp_path / "e").mkdir()
    _write_pcd(tmp_path / "e" / "MAP3D.pcd", np.zeros((0, 3), np.float32), np.zeros(0, np.uint32))
    r = subprocess.run([exe, str(tmp_path / "e" / "MAP3D.pcd"), str(tmp_path / "e.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "Cloud reading failed. no data points found" in r.stdout
