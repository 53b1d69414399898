"""GPU: the moving-least-squares smoothing of the device-resident cloud (sfmhip_cloud_mls, csrc/mls.hip; include/sfmhip.h rules
M1-M7) bit for bit against the CPU build of the same header (tests/stub/mls_capi.cpp over csrc/mls.h, with a
neighbour search of its own): out_xyz, out_normals4, src_index, n_out and every field of the stats, at orders 0, 1 and 2 and at
the shapes the kernel can go wrong at; the handle born on the device and the chain behind it; the grid shared with the other
calls on the handle; the refusals through the ABI; the host mirror's driver.  No test provokes a fault."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, cloud, poisson
from tests.mls_scenes import ERR_ARG, NAN_BITS, OK, bits, build_stub, radius_for, stub_grid, stub_mls, surface_cloud
from tests.test_gpu_poisson import _write_pcd, read_ply_mesh
from tests.test_poisson_cpu import sphere_cloud

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
ORDERS = (0, 1, 2)


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("mls"))


def same(got, want):
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    assert np.array_equal(got["src_index"], want["src_index"])
    assert np.array_equal(bits(got["xyz"]), bits(want["xyz"]))
    if want["normals"] is not None:
        assert np.array_equal(bits(got["normals"]), bits(want["normals"]))


def check(ctx, ms, xyz, radius, orders=ORDERS, sqr_gauss=0.0, handle=None):
    """the device against the stub at every order, on a fresh handle (or on `handle`); returns {order: the device's result}"""
    out = {}
    c = handle or cloud.Cloud(xyz, ctx=ctx)
    try:
        for order in orders:
            rc, want = stub_mls(ms, xyz, radius, order, sqr_gauss=sqr_gauss)
            assert rc == OK
            got = c.mls(radius, order, sqr_gauss=sqr_gauss, return_cloud=True)
            same(got, want)
            assert got["cloud"].n == len(want["xyz"]) and np.array_equal(bits(got["cloud"].download()), bits(want["xyz"]))
            got["cloud"].close()
            out[order] = got
    finally:
        if handle is None:
            c.close()
    return out


def cluster(rng, k, centre=(0.0, 0.0, 0.0), spread=0.01):
    return (np.float32(centre) + rng.uniform(0, spread, (k, 3))).astype(np.float32)


def test_tiny_clouds_and_minimum_counts(ctx, ms):
    rng = np.random.default_rng(1)
    for n in (0, 1, 2):
        got = check(ctx, ms, cluster(rng, n), 1.0)
        assert all(g["stats"]["n_out"] == 0 and g["stats"]["n_dropped"] == n for g in got.values())
    # a cluster of exactly 3 points (kept) and, far from it, one of 2 (dropped)
    xyz = np.concatenate([cluster(rng, 3), cluster(rng, 2, (5.0, 0.0, 0.0))])
    got = check(ctx, ms, xyz, 0.5)
    assert all(g["stats"]["n_out"] == 3 and g["stats"]["n_dropped"] == 2 and g["src_index"].tolist() == [0, 1, 2] for g in got.values())


def test_coefficient_edges(ctx, ms):
    """5 and 6 neighbours at order 2, 2 and 3 at order 1: below the coefficient count the plane stands"""
    rng = np.random.default_rng(2)
    xyz = np.concatenate([cluster(rng, 5), cluster(rng, 6, (5.0, 0.0, 0.0)), cluster(rng, 2, (0.0, 5.0, 0.0)), cluster(rng, 3, (0.0, 0.0, 5.0))])
    got = check(ctx, ms, xyz, 0.5)
    assert got[2]["stats"]["n_plane_only"] == 5 + 3 and got[1]["stats"]["n_plane_only"] == 0 and got[0]["stats"]["n_plane_only"] == 0
    assert all(g["stats"]["n_dropped"] == 2 and g["stats"]["n_out"] == 14 for g in got.values())
    assert np.array_equal(bits(got[2]["xyz"][:5]), bits(got[0]["xyz"][:5])) and not np.array_equal(bits(got[2]["xyz"][5:11]), bits(got[0]["xyz"][5:11]))


@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_one_cell_at_the_chunk_edges(ctx, ms, k):
    got = check(ctx, ms, cluster(np.random.default_rng(k), k), 1.0)
    assert all(g["stats"]["n_out"] == k and g["stats"]["max_neighbours"] == k for g in got.values())


@pytest.mark.parametrize("k", [63, 64, 65, 128, 129])
def test_row_span_at_the_tile_edges_beside_a_cell_of_one(ctx, ms, k):
    """a cluster of k points in cell 0 of its x row and a single point in cell 1: the single point's row span holds k + 1
    points (64, 65, 66, 129, 130: one tile, one tile and one point, two tiles and one point)"""
    rng = np.random.default_rng(100 + k)
    xyz = np.concatenate([(rng.uniform(0, 1, (k, 3)) * [0.3, 0.3, 0.3]).astype(np.float32), np.float32([[1.1, 0.1, 0.1]])])
    _, D, keys = stub_grid(ms, xyz, 1.0)
    assert D.tolist() == [2, 1, 1] and (keys[:k] == 0).all() and keys[k] == 1
    got = check(ctx, ms, xyz, 1.0)
    assert all(g["stats"]["n_out"] == k + 1 for g in got.values())
    with cloud.Cloud(xyz, ctx=ctx) as c:
        assert 3 <= c.radius_count(1.0)[k] <= k + 1


def test_radius_edge(ctx, ms):
    """a neighbour at d2 == (float)(r * r) exactly is excluded, one float below it is included"""
    r = 0.5
    near = np.float32([[0.1, 0.1, 0.0], [-0.1, 0.05, 0.02], [0.05, -0.1, 0.01]])
    xyz = np.concatenate([np.float32([[0, 0, 0]]), near, np.float32([[0.5, 0, 0], [0, np.nextafter(np.float32(0.5), np.float32(0)), 0]])])
    d2 = (xyz.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    assert d2[4] == np.float32(r * r) and d2[5] < np.float32(r * r)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        assert c.radius_count(r)[0] == 5
        got = check(ctx, ms, xyz, r, handle=c)
    assert all(g["stats"]["n_out"] == 6 for g in got.values())


def test_grid_edges(ctx, ms):
    rng = np.random.default_rng(4)
    xyz = surface_cloud(300, 5)
    got = check(ctx, ms, xyz, 10.0)                                       # the whole cloud in one cell
    assert stub_grid(ms, xyz, 10.0)[1].tolist() == [1, 1, 1] and got[2]["stats"]["max_neighbours"] == 300
    far = np.concatenate([surface_cloud(3000, 6), np.float32([[1000.0, 0.5, 0.05]])])
    cell, D, keys = stub_grid(ms, far, 0.05)
    assert D[0] == 4096 and keys[-1] % 4096 == 4095 and cell == 0.05 * (1 + 1 / 1024)       # clamped into a border cell, no doubling
    got = check(ctx, ms, far, 0.05)
    assert got[2]["stats"]["n_dropped"] >= 1 and 3000 not in got[2]["src_index"]
    # a tiny radius on a wide box: grid_build doubles the cell; 300 clusters of 10 points keep the neighbourhoods alive
    centres = rng.uniform(0, 1, (300, 1, 3))
    tiny = (centres + rng.uniform(0, 0.001, (300, 10, 3))).reshape(-1, 3).astype(np.float32)[rng.permutation(3000)]
    cell, D, _ = stub_grid(ms, tiny, 0.002)
    assert cell == 4 * 0.002 * (1 + 1 / 1024) and int(D.astype(np.int64).prod()) <= 1 << 22
    got = check(ctx, ms, tiny, 0.002)
    assert got[2]["stats"]["n_out"] > 2000 and got[2]["stats"]["max_neighbours"] >= 10


def test_degenerate_sets(ctx, ms):
    same_pt = np.tile(np.float32([[0.25, -0.5, 2.0]]), (70, 1))
    got = check(ctx, ms, same_pt, 0.1)
    for g in got.values():                                                 # M4
        assert g["stats"]["n_degenerate"] == 70 and np.array_equal(bits(g["xyz"]), bits(same_pt)) and (bits(g["normals"]) == NAN_BITS).all()
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = 0.01 * np.arange(40)
    got = check(ctx, ms, line, 0.1)
    assert all(g["stats"]["n_degenerate"] == 40 and np.array_equal(bits(g["xyz"]), bits(line)) for g in got.values())
    # M5's failed pivot: a cross in the plane z = 0, so u v = 0 at every neighbour of its centre and A is singular at order 2
    k = np.arange(-4, 5, dtype=np.float32)
    cross = np.concatenate([np.stack([0 * k, 0.01 * k, 0 * k], 1), np.stack([0.01 * k[k != 0], 0 * k[k != 0], 0 * k[k != 0]], 1)])
    got = check(ctx, ms, cross, 1.0)
    assert got[2]["stats"]["n_fit_failed"] >= 1 and got[1]["stats"]["n_fit_failed"] == 0 and got[2]["stats"]["n_out"] == 17


@pytest.fixture(scope="module")
def cloud20k():
    xyz = surface_cloud(20_000, 21)
    bad = np.random.default_rng(5).choice(20_000, 200, replace=False)      # 1 % NaN and +-inf rows
    xyz[bad[:100], 0] = np.nan
    xyz[bad[100:150], 1] = np.inf
    xyz[bad[150:], 2] = -np.inf
    return xyz, bad


def test_non_finite_input(ctx, ms, cloud20k):
    xyz, bad = cloud20k
    got = check(ctx, ms, xyz, radius_for(30, 20_000, 1.0))
    for g in got.values():
        assert not np.isin(bad, g["src_index"]).any() and g["stats"]["n_out"] + g["stats"]["n_dropped"] == 19_800
        assert np.isfinite(g["xyz"]).all() and 30 <= g["stats"]["max_neighbours"] <= 90


def test_gauss_parameter_underflow(ctx, ms, cloud20k):
    """r = 0.1 and g = 1e-5: (e.e) / g passes 745 inside the radius, so the far weights are exactly 0"""
    got = check(ctx, ms, cloud20k[0][:6000], 0.1, orders=(1, 2), sqr_gauss=1e-5)
    assert got[2]["stats"]["n_out"] > 5000
    got = check(ctx, ms, cloud20k[0][:2000], 0.1, orders=(2,), sqr_gauss=1e-9)           # every weight but the point's own: the fit fails
    assert got[2]["stats"]["n_fit_failed"] > 1000


def test_shared_grid_and_repeatability(ctx, ms, cloud20k):
    xyz = cloud20k[0]
    r = radius_for(30, 20_000, 1.0)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        first = c.mls(r, 2)
        again = c.mls(r, 2)                                                # a second call: the same bytes
        same(again, first)
        counts = c.radius_count(r)                                         # the grid radius_count shares
        c.knn(10)
        same(c.mls(r, 2), first)
        assert counts.max() == first["stats"]["max_neighbours"]
        c.radius_count(2 * r)                                              # another radius takes the grid away: rebuilt
        same(c.mls(r, 2), first)
        same(c.mls(r, 0), stub_mls(ms, xyz, r, 0)[1])
        no_normals = c.mls(r, 2, normals=False)
        assert no_normals["normals"] is None and np.array_equal(bits(no_normals["xyz"]), bits(first["xyz"]))


def test_the_handle_born_on_the_device(ctx, cloud20k):
    """mls -> normals -> poisson on the device handle equals the same chain through host arrays"""
    xyz = cloud20k[0]
    r = radius_for(30, 20_000, 1.0)
    opts = dict(depth=5)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        got = c.mls(r, 2, return_cloud=True)
    dev = got["cloud"]
    assert dev.xyz is None and dev.n == len(got["xyz"])
    nd = dev.normals(10)
    vd, td, sd = poisson.reconstruct(dev, nd, poisson.default_opts(**opts))
    assert np.array_equal(bits(dev.download()), bits(got["xyz"]))
    dev.close()
    with cloud.Cloud(got["xyz"], ctx=ctx) as h:
        nh = h.normals(10)
        vh, th, sh = poisson.reconstruct(h, nh, poisson.default_opts(**opts))
    assert np.array_equal(bits(nd), bits(nh)) and vd.tobytes() == vh.tobytes() and td.tobytes() == th.tobytes() and len(td) > 100
    assert sd.iso_value == sh.iso_value


def test_abi_refusals(ctx):
    L = _lib.lib()
    xyz = surface_cloud(50, 3)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        o = cloud.MlsOpts()
        assert L.sfmhip_mls_default_opts(C.addressof(o)) == OK and L.sfmhip_mls_default_opts(None) == ERR_ARG
        assert (o.search_radius, o.polynomial_order, o.compute_normals, o.sqr_gauss_param) == (0.0, 2, 1, 0.0)
        oxyz, on4, src = np.full((50, 3), 7.5, np.float32), np.full((50, 4), 7.5, np.float32), np.full(50, 77, np.int32)
        m, st = C.c_int32(-9), cloud.MlsStats(*([-9] * 6))

        def call(h=c.h, opts=o, n_out=m):
            return L.sfmhip_cloud_mls(h, C.addressof(opts) if opts is not None else None, oxyz.ctypes.data, on4.ctypes.data, src.ctypes.data,
                                      C.addressof(n_out) if n_out is not None else None, C.addressof(st), None)

        assert call() == ERR_ARG                                            # the default radius 0 must be replaced
        bad = []
        for kw in (dict(search_radius=-1.0), dict(search_radius=float("inf")), dict(search_radius=float("nan")),
                   dict(search_radius=0.2, polynomial_order=3), dict(search_radius=0.2, polynomial_order=-1),
                   dict(search_radius=0.2, sqr_gauss_param=float("nan")), dict(search_radius=0.2, sqr_gauss_param=float("inf"))):
            b = cloud.MlsOpts(0.0, 2, 1, 0.0)
            for k, v in kw.items():
                setattr(b, k, v)
            bad.append(call(opts=b))
        assert bad == [ERR_ARG] * 7
        good = cloud.MlsOpts(2.0, 2, 1, 0.0)                                # (every point within reach of every other)
        assert call(h=None, opts=good) == ERR_ARG and call(opts=None) == ERR_ARG and call(opts=good, n_out=None) == ERR_ARG
        assert m.value == -9 and st.n_out == -9 and (oxyz == 7.5).all() and (on4 == 7.5).all() and (src == 77).all()      # nothing written
        assert L.sfmhip_cloud_mls_last_timing(c.h, None) == ERR_ARG and L.sfmhip_cloud_mls_last_timing(None, None) == ERR_ARG
        assert call(opts=good) == OK and m.value == 50 and st.n_out == 50
        assert L.sfmhip_cloud_mls(c.h, C.addressof(good), None, None, None, C.addressof(m), None, None) == OK and m.value == 50
    nan = np.full((5, 3), np.nan, np.float32)                               # no finite point: OK, nothing out, an empty handle
    with cloud.Cloud(nan, ctx=ctx) as c:
        got = c.mls(0.2, return_cloud=True)
        assert got["stats"] == dict.fromkeys(got["stats"], 0) and got["cloud"].n == 0 and len(got["xyz"]) == 0
        got["cloud"].close()
    with pytest.raises(_lib.SfmHipError):
        with cloud.Cloud(xyz, ctx=ctx) as c:
            c.mls(0.0)


def read_smoothed_pcd(path):
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    assert b"FIELDS x y z normal_x normal_y normal_z curvature index" in raw[:end]
    rec = np.frombuffer(raw, np.dtype([("f", "<f4", 7), ("i", "<i4")]), offset=end)
    return rec["f"][:, :3].copy(), rec["f"][:, 3:].copy(), rec["i"].copy()


def test_host_mirror(ctx, ms, tmp_path):
    """sfm_smooth_selftest: smoothCloud through pcl::MovingLeastSquares as pcllite.h mirrors it equals the library call; the
    three-argument create_mesh gives the mesh of the Python chain on the smoothed handle, the two-argument one the mesh it gave
    before (the Python path's, as tests/test_gpu_poisson.py pins it)"""
    exe = build.build_smooth_demo()
    xyz, _ = sphere_cloud(20_000, 17)
    xyz = (xyz * 0.5 * (1 + np.random.default_rng(2).normal(0, 0.002, (20_000, 1)))).astype(np.float32)
    xyz[11] = np.nan
    r = 0.04
    _write_pcd(tmp_path / "in.pcd", xyz)
    for order in (0, 2):
        res = subprocess.run([exe, str(tmp_path / "in.pcd"), str(r), str(order), str(tmp_path / "out.pcd")] +
                             ([str(tmp_path / "mesh.ply"), str(tmp_path / "plain.ply")] if order == 2 else []),
                             capture_output=True, text=True, timeout=280)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        pxyz, pn4, pidx = read_smoothed_pcd(tmp_path / "out.pcd")
        rc, want = stub_mls(ms, xyz, r, order)
        assert rc == OK and res.stdout.startswith(f"points 20000 smoothed {len(want['xyz'])}\n")
        assert np.array_equal(bits(pxyz), bits(want["xyz"])) and np.array_equal(bits(pn4), bits(want["normals"]))
        assert np.array_equal(pidx, want["src_index"]) and 11 not in pidx
    v, t = read_ply_mesh(tmp_path / "mesh.ply")
    with cloud.Cloud(xyz, ctx=ctx) as c:
        sm = c.mls(r, 2, normals=False, return_cloud=True)["cloud"]
    nrm = sm.normals(10)
    nrm[:, :3] = -nrm[:, :3]
    pv, pt, s = poisson.reconstruct(sm, nrm, poisson.default_opts(cg_max_iter=8 << 7))
    sm.close()
    assert len(t) > 1000 and v.tobytes() == pv.tobytes() and t.tobytes() == pt.tobytes()
    v0, t0 = read_ply_mesh(tmp_path / "plain.ply")
    qv, qt, _ = poisson.create_mesh(xyz, ctx=ctx)
    assert v0.tobytes() == qv.tobytes() and t0.tobytes() == qt.tobytes() and v0.tobytes() != v.tobytes()
