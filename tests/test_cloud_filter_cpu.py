"""PCL 1.8.1's VoxelGrid and StatisticalOutlierRemoval (csrc/cloud_filter.h) on the CPU, through a g++ build
of the header the device kernels compile: the voxel keys against a numpy float32 restatement, the centroids against
np.unique and float64 means, the summation order bit for bit on single voxels, min_points and voxel_of, the colour and
normal attributes, the refusals, the edge cases; the mean distances and the kept set against scipy's cKDTree in double,
the documented edge cases, what the filter does to known outliers, and both filters under ASan / UBSan in a stand-alone
driver.  No GPU.  PARITY UNPINNED: PCL is not in the image."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "cloud_filter_capi.cpp")
NAN_BITS = 0x7FC00000
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -3, -5


def build_stub(directory):
    so = str(directory / "libcloudfiltercapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.cf_voxel_keys.argtypes = [ci, vp, vp, vp, vp]
    lib.cf_voxel_grid.argtypes = [ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.cf_statistical_outlier.argtypes = [ci, vp, ci, C.c_double, ci, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def cf(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("cloud_filter"))


def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def _leaf(leaf):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, np.float32), (3,)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# thin numpy-facing wrappers (shared with tests/test_gpu_cloud_filter.py)
def stub_keys(cf, xyz, leaf):
    xyz, lf = _f(xyz), _leaf(leaf)
    keys, div = np.zeros(max(len(xyz), 1), np.int32), np.zeros(3, np.int32)
    rc = cf.cf_voxel_keys(len(xyz), xyz.ctypes.data, lf.ctypes.data, keys.ctypes.data, div.ctypes.data)
    return rc, keys[:len(xyz)], div


def stub_voxel_grid(cf, xyz, leaf, min_points=0, rgb=None, normals=None):
    """(status, dict as cloud.Cloud.voxel_grid returns it); the outputs start as a pattern, so a refusal shows them untouched"""
    xyz, lf = _f(xyz), _leaf(leaf)
    n, n1 = len(xyz), max(len(xyz), 1)
    col = None if rgb is None else np.ascontiguousarray(rgb, np.uint32)
    nrm = None if normals is None else _f(normals)
    oxyz, vox, m = np.full((n1, 3), 7.5, np.float32), np.full(n1, 77, np.int32), np.full(1, -9, np.int32)
    ocol = None if col is None else np.full(n1, 0xABCDEF, np.uint32)
    onrm = None if nrm is None else np.full((n1, 3), 7.5, np.float32)
    opt = lambda a: None if a is None else a.ctypes.data
    rc = cf.cf_voxel_grid(n, xyz.ctypes.data, lf.ctypes.data, min_points, opt(col), opt(nrm), oxyz.ctypes.data, opt(ocol), opt(onrm),
                          vox.ctypes.data, m.ctypes.data)
    if rc != OK:
        return rc, {"xyz": oxyz, "voxel_of": vox, "n_out": int(m[0])}
    out = {"xyz": oxyz[:m[0]], "voxel_of": vox[:n]}
    if ocol is not None:
        out["rgb"] = ocol[:m[0]]
    if onrm is not None:
        out["normals"] = onrm[:m[0]]
    return rc, out


def stub_sor(cf, xyz, mean_k, std_mul=1.0, negative=False):
    """(status, kept indices, mean_dist, threshold)"""
    xyz = _f(xyz)
    n1 = max(len(xyz), 1)
    idx, m, md, thr = np.full(n1, -7, np.int32), np.full(1, -9, np.int32), np.full(n1, 7.5, np.float32), np.full(1, 7.5, np.float64)
    rc = cf.cf_statistical_outlier(len(xyz), xyz.ctypes.data, mean_k, std_mul, int(negative), idx.ctypes.data, m.ctypes.data,
                                   md.ctypes.data, thr.ctypes.data)
    if rc != OK:
        return rc, idx, md, float(thr[0])
    return rc, idx[:m[0]], md[:len(xyz)], float(thr[0])


def surfaces_and_outliers(n, seed, outliers=0.05):
    """tests/test_cloud_cpu.py's surface_cloud without its final permutation: a sphere, a plane and a wavy sheet, then the
    uniform outliers -- (xyz float32, is_outlier)"""
    rng = np.random.default_rng(seed)
    m = n - int(n * outliers)
    a = rng.normal(size=(m // 3, 3))
    sph = 0.4 * a / np.linalg.norm(a, axis=1, keepdims=True) + [0.5, 0.5, 0.5]
    pl = np.c_[rng.uniform(0, 1, m // 3), rng.uniform(0, 1, m // 3), np.full(m // 3, 0.1)]
    k = m - 2 * (m // 3)
    u, v = rng.uniform(0, 1, k), rng.uniform(0, 1, k)
    wav = np.c_[u, 0.8 + 0.05 * np.sin(6 * u) * np.cos(5 * v), v]
    out = rng.uniform(0, 1, (n - m, 3))
    return np.concatenate([sph, pl, wav, out]).astype(np.float32), np.arange(n) >= m


def surface_cloud(n, seed):
    xyz, _ = surfaces_and_outliers(n, seed)
    return xyz[np.random.default_rng(seed + 100).permutation(n)]


# ---- the numpy restatements

def np_keys(xyz, leaf):
    """V1-V3 in float32: (keys with -1 for non-finite points, div)"""
    xyz, lf = _f(xyz), _leaf(leaf)
    inv = np.float32(1.0) / lf
    fin = np.isfinite(xyz).all(1)
    mn, mx = xyz[fin].min(0), xyz[fin].max(0)
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    div = max_b - min_b + 1
    ijk = (np.floor(xyz[fin] * inv) - min_b.astype(np.float32)).astype(np.float32).astype(np.int64)
    keys = np.full(len(xyz), -1, np.int64)
    keys[fin] = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    return keys, div


def np_run_sum(v):
    """V5 in float32: blocks of 64 summed sequentially from 0, the block sums added in order from 0"""
    v = np.asarray(v, np.float32)
    total = np.float32(0.0)
    for b in range(0, len(v), 64):
        s = np.float32(0.0)
        for x in v[b:b + 64]:
            s = np.float32(s + x)
        total = np.float32(total + s)
    return total


# ---- voxel grid

@pytest.mark.parametrize("leaf", [0.25, (0.25, 0.125, 0.5), 0.013])
def test_keys_equal_the_float32_restatement(cf, leaf):
    rng = np.random.default_rng(1)
    grid = rng.integers(-9, 9, (400, 3)).astype(np.float32) * np.float32(0.25)       # exactly on faces: k * 0.25
    xyz = np.concatenate([rng.uniform(-2.0, 1.5, (3000, 3)), grid, [[37.0, -2.0, 1.5]], [[np.nan, 0, 0]], [[0, np.inf, 0]]])
    xyz = xyz.astype(np.float32)
    rc, keys, div = stub_keys(cf, xyz, leaf)
    want, wdiv = np_keys(xyz, leaf)
    assert rc == OK and np.array_equal(div, wdiv) and np.array_equal(keys, want)
    assert keys[-1] == -1 and keys[-2] == -1 and keys[:-2].min() >= 0 and (keys < np.prod(wdiv)).all()
    # a point on a face belongs to the upper voxel
    assert list(stub_keys(cf, [[0, 0, 0], [0.25, 0, 0], [0.24999, 0, 0], [-0.25, 0, 0]], 0.25)[1]) == [1, 2, 1, 0]


@pytest.mark.parametrize("leaf", [0.02, 0.05, (0.3, 0.04, 0.11)])
def test_centroids_against_unique_and_float64_means(cf, leaf):
    xyz = surface_cloud(20_000, 3)
    xyz[::100, 1] = np.nan
    rc, out = stub_voxel_grid(cf, xyz, leaf)
    assert rc == OK
    fin = np.isfinite(xyz).all(1)
    keys, _ = np_keys(xyz, leaf)
    uk, inv, cnt = np.unique(keys[fin], return_inverse=True, return_counts=True)
    assert len(out["xyz"]) == len(uk)                                                  # the count; ascending order below
    mean = np.zeros((len(uk), 3))
    np.add.at(mean, inv, xyz[fin].astype(np.float64))
    mean /= cnt[:, None]
    assert np.array_equal(out["voxel_of"][fin], inv) and (out["voxel_of"][~fin] == -1).all()
    # a sequential float sum of `count` terms and one division: count * 2^-23 * max|coordinate| (factor 2 for the division)
    bound = cnt[:, None] * 2.0 ** -23 * np.abs(xyz[fin]).max()
    assert (np.abs(out["xyz"].astype(np.float64) - mean) <= bound).all()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 129, 300])
def test_summation_order_bit_for_bit(cf, count):
    rng = np.random.default_rng(count)
    xyz = (rng.uniform(0.01, 0.99, (count, 3)) * [1, 1e-3, 100]).astype(np.float32) + np.float32([5, 0, 100])
    nrm = rng.normal(size=(count, 3)).astype(np.float32)
    rc, out = stub_voxel_grid(cf, xyz, (8.0, 8.0, 500.0), normals=nrm)
    assert rc == OK and len(out["xyz"]) == 1 and (out["voxel_of"] == 0).all()
    want = np.array([np_run_sum(xyz[:, a]) / np.float32(count) for a in range(3)], np.float32)
    assert np.array_equal(bits(out["xyz"][0]), bits(want))
    s = np.array([np_run_sum(nrm[:, a]) for a in range(3)], np.float32)
    l = np.sqrt(np.float32(np.float32(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
    assert np.array_equal(bits(out["normals"][0]), bits(s / l))


def test_min_points_and_voxel_of(cf):
    xyz = surface_cloud(5000, 5)
    full = stub_voxel_grid(cf, xyz, 0.03)[1]
    cnt = np.bincount(full["voxel_of"])
    assert cnt.min() == 1 and cnt.max() >= 3
    for mp in (0, 2, 3):
        rc, out = stub_voxel_grid(cf, xyz, 0.03, min_points=mp)
        keep = cnt >= mp
        assert rc == OK and len(out["xyz"]) == keep.sum()
        assert np.array_equal(bits(out["xyz"]), bits(full["xyz"][keep]))              # the same centroids, the dropped ones gone
        row = np.where(keep, np.cumsum(keep) - 1, -1)
        assert np.array_equal(out["voxel_of"], row[full["voxel_of"]])
        for r in (0, len(out["xyz"]) // 2, len(out["xyz"]) - 1):                       # voxel_of is consistent with the outputs
            members = xyz[out["voxel_of"] == r]
            assert len(members) >= max(mp, 1) and np.allclose(members.mean(0), out["xyz"][r], atol=1e-6)


def test_attributes(cf):
    # hand-made voxels (leaf 1): voxel 0 holds three points, voxel 1 two, voxel 2 one
    xyz = np.float32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.5, 0.5, 0.5], [0.3, 0.3, 0.3], [1.6, 0.1, 0.2], [2.5, 0.5, 0.5]])
    rgb = np.uint32([0x010203, 0x020304, 0xFF0000, 0x040507, 0x00FF01, 0xFFFFFFFF])
    nrm = np.float32([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 3, 2], [-1, 0, 0], [0, np.nan, 1]])
    rc, out = stub_voxel_grid(cf, xyz, 1.0, rgb=rgb, normals=nrm)
    assert rc == OK and list(out["voxel_of"]) == [0, 0, 1, 0, 1, 2]
    # (1 + 2 + 4) / 3 = 2, (2 + 3 + 5) / 3 = 3, (3 + 4 + 7) / 3 = 4 truncated; 255 / 2 = 127; the top byte is dropped
    assert list(out["rgb"]) == [0x020304, 0x7F7F00, 0x00FFFFFF]
    assert np.array_equal(bits(out["normals"][0]), bits(np.float32([0, 3, 4]) / np.sqrt(np.float32(25))))
    assert (bits(out["normals"][1]) == NAN_BITS).all()                                 # a zero sum
    assert (bits(out["normals"][2]) == NAN_BITS).all()                                 # a NaN normal propagates
    assert "rgb" not in stub_voxel_grid(cf, xyz, 1.0, normals=nrm)[1]


def test_refusals_leave_the_outputs_untouched(cf):
    ok = np.float32([[0, 0, 0], [1289.5] * 3])
    rc, out = stub_voxel_grid(cf, ok, 1.0)                                             # d = 1290, 1290^3 = 2 146 689 000
    assert rc == OK and len(out["xyz"]) == 2 and np.array_equal(stub_keys(cf, ok, 1.0)[2], [1290] * 3)
    assert stub_keys(cf, ok, 1.0)[1][1] == 1290 ** 3 - 1
    for xyz, leaf, status in ((np.float32([[0, 0, 0], [1290.5] * 3]), 1.0, ERR_UNSUPPORTED),   # 1291^3 = 2 151 685 171
                              (np.float32([[3e9, 0, 0], [3e9, 1, 1]]), 1.0, ERR_UNSUPPORTED),   # a ratio beyond int32
                              (np.float32([[0, 0, 0], [1, 1, 1]]), 1e-10, ERR_UNSUPPORTED),
                              (np.float32([[0, 0, 0], [2e7, 0, 0]]), 1.0, ERR_UNSUPPORTED),     # one extent beyond 2^24
                              (ok, (1.0, 0.0, 1.0), ERR_ARG), (ok, (1.0, -1.0, 1.0), ERR_ARG),
                              (ok, (1.0, np.inf, 1.0), ERR_ARG), (ok, (np.nan, 1.0, 1.0), ERR_ARG)):
        rc, out = stub_voxel_grid(cf, xyz, leaf)
        assert rc == status, (leaf, rc)
        assert (out["xyz"] == 7.5).all() and (out["voxel_of"] == 77).all() and out["n_out"] == -9
    assert cf.cf_voxel_grid(2, ok.ctypes.data, _leaf(1.0).ctypes.data, -1, None, None, None, None, None, None, np.zeros(1, np.int32).ctypes.data) == ERR_ARG


def test_voxel_edge_cases(cf):
    rc, out = stub_voxel_grid(cf, np.zeros((0, 3)), 0.1)
    assert rc == OK and len(out["xyz"]) == 0 and len(out["voxel_of"]) == 0
    rc, out = stub_voxel_grid(cf, [[1.5, -2.5, 3.25]], 0.1)
    assert rc == OK and np.array_equal(out["xyz"], np.float32([[1.5, -2.5, 3.25]])) and list(out["voxel_of"]) == [0]
    rc, out = stub_voxel_grid(cf, [[np.nan, 0, 0], [0, np.inf, 0]], 0.1)               # nothing finite
    assert rc == OK and len(out["xyz"]) == 0 and list(out["voxel_of"]) == [-1, -1]
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (300, 1))
    rc, out = stub_voxel_grid(cf, same, 0.1)
    assert rc == OK and len(out["xyz"]) == 1 and (out["voxel_of"] == 0).all()
    assert np.allclose(out["xyz"][0], same[0], rtol=300 * 2.0 ** -23)
    xyz = surface_cloud(2000, 9)
    xyz[::7] = np.nan
    rc, out = stub_voxel_grid(cf, xyz, 0.05)
    assert rc == OK and (out["voxel_of"][::7] == -1).all() and (np.delete(out["voxel_of"], np.s_[::7]) >= 0).all()
    assert np.isfinite(out["xyz"]).all()


# ---- statistical outlier removal

def scipy_sor(xyz, mean_k, std_mul):
    """the filter in double over scipy's k-d tree: (mean_dist with 0 for non-finite points, threshold)"""
    x = np.asarray(xyz, np.float64)
    fin = np.isfinite(x).all(1)
    d, _ = cKDTree(x[fin]).query(x[fin], k=mean_k + 1, workers=16)
    md = np.zeros(len(x))
    md[fin] = d[:, 1:].mean(1)
    m = md[fin]
    return md, m.mean() + std_mul * m.std(ddof=1)


@pytest.fixture(scope="module")
def sor_cloud():
    xyz = surface_cloud(20_000, 11)
    xyz[::100, 2] = np.nan
    return xyz


@pytest.mark.parametrize("mean_k", [1, 8, 31, 32, 63])
def test_mean_distances_and_kept_set_against_scipy(cf, sor_cloud, mean_k):
    xyz = sor_cloud
    fin = np.isfinite(xyz).all(1)
    rc, kept, md, thr = stub_sor(cf, xyz, mean_k, 1.0)
    want_md, want_thr = scipy_sor(xyz, mean_k, 1.0)
    assert rc == OK and (md[~fin] == 0).all()
    assert np.allclose(md, want_md, rtol=1e-5, atol=1e-6)                              # tests/test_gpu_cloud.py's tolerance for this d2
    assert abs(thr - want_thr) <= 1e-5 * want_thr
    window = fin & (np.abs(want_md - want_thr) <= 1e-5 * want_thr)                     # too close to the threshold to call
    assert window.sum() <= 0.001 * len(xyz)
    want = fin & (want_md <= want_thr)
    got = np.zeros(len(xyz), bool)
    got[kept] = True
    assert np.array_equal(got[~window], want[~window]) and (np.diff(kept) > 0).all()
    rc, out, md2, thr2 = stub_sor(cf, xyz, mean_k, 1.0, negative=True)                 # the complement within the finite points
    assert rc == OK and thr2 == thr and np.array_equal(bits(md2), bits(md))
    assert np.array_equal(np.sort(np.concatenate([kept, out])), np.flatnonzero(fin))   # NaN points are in neither set


def test_sor_edge_cases(cf):
    xyz = surface_cloud(200, 2)
    for mean_k in (1, 16, 63):
        rc, kept, md, thr = stub_sor(cf, xyz[:mean_k + 1], mean_k)                     # n = mean_k + 1: every other point is a neighbour
        want_md, want_thr = scipy_sor(xyz[:mean_k + 1], mean_k, 1.0)
        # S3 squares md in float: each term of sq is off by up to 2^-24 of itself, so var by up to 2^-24 N mean(md^2) / (N - 1)
        # and, where the true variance is (nearly) 0 as for two points, the deviation by up to the root of that
        n = mean_k + 1
        slack = np.sqrt(2.0 ** -24 * n * (want_md ** 2).mean() / (n - 1))
        assert rc == OK and np.allclose(md, want_md, rtol=1e-5, atol=1e-6) and abs(thr - want_thr) <= 1e-5 * want_thr + slack
        rc, kept, md, thr = stub_sor(cf, xyz[:mean_k], mean_k)                         # n = mean_k: refused, nothing written
        assert rc == ERR_ARG and (kept == -7).all() and (md == 7.5).all() and thr == 7.5
        bad = np.concatenate([xyz[:mean_k], [[np.nan, 0, 0]]]).astype(np.float32)      # ... counted over the finite points
        assert stub_sor(cf, bad, mean_k)[0] == ERR_ARG
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (300, 1))
    rc, kept, md, thr = stub_sor(cf, same, 16)
    assert rc == OK and np.array_equal(kept, np.arange(300)) and thr == 0.0 and (md == 0).all()
    rc, kept, md, thr = stub_sor(cf, xyz, 8, std_mul=0.0)                              # the threshold is the mean
    fsum = md.astype(np.float64).sum() / len(xyz)
    assert rc == OK and abs(thr - fsum) <= 1e-12 and np.array_equal(kept, np.flatnonzero(md.astype(np.float64) <= thr))
    assert 0 < len(kept) < len(xyz)
    rc, kept, md, thr = stub_sor(cf, np.zeros((0, 3)), 8)
    assert rc == OK and len(kept) == 0 and thr == 0.0
    rc, kept, md, thr = stub_sor(cf, [[np.nan, 0, 0]] * 3, 8)                          # nothing finite: nothing kept, no error
    assert rc == OK and len(kept) == 0 and (md == 0).all()
    for mean_k, std_mul in ((0, 1.0), (64, 1.0), (8, np.nan), (8, np.inf)):
        assert stub_sor(cf, xyz, mean_k, std_mul)[0] == ERR_ARG


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_known_outliers_are_removed(cf, seed):
    xyz, is_out = surfaces_and_outliers(20_000, seed)
    rc, kept, _, _ = stub_sor(cf, xyz, 16, 1.0)
    gone = np.ones(len(xyz), bool)
    gone[kept] = False
    assert rc == OK
    assert gone[is_out].mean() >= 0.70                                                # (75.7 - 78.1 % with the scipy restatement)
    assert gone[~is_out].mean() <= 0.005                                              # (0.03 - 0.07 %)


def test_filters_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cloud_filter_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DCLOUD_FILTER_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.endswith("done\n")
    assert "refusals -5 -5 -3\n" in r.stdout and "edge 0 -3 0\n" in r.stdout and "leaf 5.00 min_points 3 voxels 2 " in r.stdout
    assert "mean_k 63 negative 1 kept " in r.stdout
