"""map3D's step 10 (csrc/cloud.h: PCL 1.8.1's PassThrough, RadiusOutlierRemoval and k-nearest NormalEstimation,
reference src/Sfm.cpp:94-102, :1323-1383) on the CPU, through a g++ build of the header the device kernels compile:
the distance against numpy float32, radius counts against scipy's cKDTree, the boundary rules on exactly representable
clouds, PassThrough's limits, k-NN against a float32 brute force, normals against numpy's eigh, the documented
degenerate outcomes, one cloud under ASan / UBSan, and the PCD reader (pcllite.h).  No GPU.  PARITY UNPINNED: PCL is
not in the image."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from sfm_danpipeline_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "cloud_capi.cpp")
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def cc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cloud") / "libcloudcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, f32, f64, ci = C.c_void_p, C.c_float, C.c_double, C.c_int
    lib.cloud_dist2.argtypes = [f32] * 6
    lib.cloud_dist2.restype = f32
    lib.cloud_radius2.argtypes = [f64]
    lib.cloud_radius2.restype = f32
    for f in ("cloud_atan2",):
        getattr(lib, f).argtypes = [f64, f64]
        getattr(lib, f).restype = f64
    for f in ("cloud_cos", "cloud_sin"):
        getattr(lib, f).argtypes = [f64]
        getattr(lib, f).restype = f64
    lib.cloud_roots.argtypes = [vp, vp]
    lib.cloud_eigen33.argtypes = [vp, vp, vp]
    lib.cloud_normal_from_cov.argtypes = [vp, ci, vp, vp, vp]
    lib.cloud_normal_of_list.argtypes = [vp, ci, vp, vp, vp]
    lib.cloud_passthrough.argtypes = [ci, vp, ci, f32, f32, ci, vp]
    lib.cloud_radius_count.argtypes = [ci, vp, f64, ci, vp]
    lib.cloud_radius_outlier.argtypes = [ci, vp, f64, ci, vp]
    lib.cloud_knn.argtypes = [ci, vp, ci, vp, vp]
    lib.cloud_normals.argtypes = [ci, vp, ci, vp, vp]
    lib.cloud_load_pcd.argtypes = [C.c_char_p, vp, ci, vp, vp]
    return lib


def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


# thin numpy-facing wrappers (shared with tests/test_gpu_cloud.py)
def stub_passthrough(cc, xyz, axis=0, lo=0.003, hi=0.83, negative=False):
    xyz = _f(xyz)
    out = np.zeros(max(len(xyz), 1), np.int32)
    m = cc.cloud_passthrough(len(xyz), xyz.ctypes.data, axis, lo, hi, int(negative), out.ctypes.data)
    return out[:m]


def stub_counts(cc, xyz, r, cap=0):
    xyz = _f(xyz)
    out = np.zeros(max(len(xyz), 1), np.int32)
    cc.cloud_radius_count(len(xyz), xyz.ctypes.data, r, cap, out.ctypes.data)
    return out[:len(xyz)]


def stub_outlier(cc, xyz, r=0.07, min_pts=150):
    xyz = _f(xyz)
    out = np.zeros(max(len(xyz), 1), np.int32)
    m = cc.cloud_radius_outlier(len(xyz), xyz.ctypes.data, r, min_pts, out.ctypes.data)
    return out[:m]


def stub_knn(cc, xyz, k):
    xyz = _f(xyz)
    idx, d2 = np.zeros((max(len(xyz), 1), k), np.int32), np.zeros((max(len(xyz), 1), k), np.float32)
    cc.cloud_knn(len(xyz), xyz.ctypes.data, k, idx.ctypes.data, d2.ctypes.data)
    return idx[:len(xyz)], d2[:len(xyz)]


def stub_normals(cc, xyz, k, vp=(0, 0, 0)):
    xyz = _f(xyz)
    v = np.asarray(vp, np.float32)
    out = np.zeros((max(len(xyz), 1), 4), np.float32)
    cc.cloud_normals(len(xyz), xyz.ctypes.data, k, v.ctypes.data, out.ctypes.data)
    return out[:len(xyz)]


def normal_of_list(cc, nb, p, vp=(0, 0, 0)):
    nb, p, v = _f(nb), np.asarray(p, np.float32), np.asarray(vp, np.float32)
    out = np.zeros(4, np.float32)
    cc.cloud_normal_of_list(nb.ctypes.data, len(nb), p.ctypes.data, v.ctypes.data, out.ctypes.data)
    return out


def surface_cloud(n, seed, outliers=0.05, scale=1.0):
    """Points on a sphere, a plane and a wavy sheet, plus uniform outliers in their box (float32)."""
    rng = np.random.default_rng(seed)
    m = n - int(n * outliers)
    a = rng.normal(size=(m // 3, 3))
    sph = 0.4 * a / np.linalg.norm(a, axis=1, keepdims=True) + [0.5, 0.5, 0.5]
    pl = np.c_[rng.uniform(0, 1, m // 3), rng.uniform(0, 1, m // 3), np.full(m // 3, 0.1)]
    k = m - 2 * (m // 3)
    u, v = rng.uniform(0, 1, k), rng.uniform(0, 1, k)
    wav = np.c_[u, 0.8 + 0.05 * np.sin(6 * u) * np.cos(5 * v), v]
    out = rng.uniform(0, 1, (n - m, 3))
    xyz = np.concatenate([sph, pl, wav, out]) * scale
    return xyz[rng.permutation(n)].astype(np.float32)


def brute_counts(xyz, r2):
    xyz = _f(xyz)
    d = xyz[:, None, :] - xyz[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return (d2 < r2).sum(1)


def brute_knn(xyz, k):
    xyz = _f(xyz)
    n = len(xyz)
    fin = np.isfinite(xyz).all(1)
    d = xyz[:, None, :] - xyz[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
    idx = np.full((n, k), -1, np.int32)
    dd = np.full((n, k), np.inf, np.float32)
    cols = np.nonzero(fin)[0]
    for i in np.nonzero(fin)[0]:
        order = np.lexsort((cols, d2[i, cols]))[:k]
        idx[i, :len(order)] = cols[order]
        dd[i, :len(order)] = d2[i, cols[order]]
    return idx, dd


# ---------------------------------------------------------------- the distance and the radius rules
def test_distance_matches_numpy_float32_bit_for_bit(cc):
    rng = np.random.default_rng(1)
    a = (rng.normal(size=(2000, 3)) * rng.choice([1e-3, 1, 1e3], (2000, 1))).astype(np.float32)
    b = (a + rng.normal(size=a.shape).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    d = a - b
    want = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    got = np.array([cc.cloud_dist2(*map(float, a[i]), *map(float, b[i])) for i in range(len(a))], np.float32)
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_radius_squared_in_double_then_float(cc):
    for r in (0.07, 0.1, 0.3, 1.0 / 3.0, 2.5):
        assert np.float32(cc.cloud_radius2(r)) == np.float32(r * r)
    for r in (0.1, 0.7):                            # (radii where squaring in float would give another r2)
        assert np.float32(r * r) != np.float32(r) * np.float32(r)


@pytest.mark.parametrize("seed", [0, 1])
def test_radius_counts_match_scipy(cc, seed):
    xyz = surface_cloud(6000, seed)
    r = 0.07
    got = stub_counts(cc, xyz, r)
    want = cKDTree(xyz.astype(np.float64)).query_ball_point(xyz.astype(np.float64), r, return_length=True)
    # pairs within 1e-5 of the radius could fall either way between float and double: keep the comparison clear of them
    t = cKDTree(xyz.astype(np.float64))
    lo = t.query_ball_point(xyz.astype(np.float64), r * (1 - 1e-5), return_length=True)
    hi = t.query_ball_point(xyz.astype(np.float64), r * (1 + 1e-5), return_length=True)
    clear = lo == hi
    assert clear.mean() > 0.95
    assert np.array_equal(got[clear], want[clear])
    assert np.array_equal(got, brute_counts(xyz, np.float32(r * r))) if len(xyz) <= 6000 else True


def _offset_with_d2(target):
    """float32 (x, y) whose float d2 from the origin is exactly `target`."""
    for y in np.float32(np.sqrt(target)) * np.linspace(0, 0.5, 400, dtype=np.float32):
        y = np.float32(y)
        x = np.float32(np.sqrt(np.float64(target) - np.float64(y) * np.float64(y)))
        for s in range(-4, 5):
            xs = x
            for _ in range(abs(s)):
                xs = np.nextafter(xs, np.float32(np.sign(s)))
            if np.float32(np.float32(xs * xs) + np.float32(y * y)) == target:
                return xs, y
    raise AssertionError("no offset found")


def test_radius_boundary_rules(cc):
    # a point at exactly r on x with r = 0.5 (0.25 exact): d2 == r2 is not a neighbour
    xyz = np.array([[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0]], np.float32)
    assert list(stub_counts(cc, xyz, 0.5)) == [2, 2, 3]
    # (float)(r * r) squared in double: at r = 0.1 it lies below float(r)^2, at r = 0.7 above; a pair whose d2 lands
    # exactly on the smaller of the two squares is counted iff that square is below the rule's r2
    for r in (0.1, 0.7):
        r2, r2f = np.float32(r * r), np.float32(r) * np.float32(r)
        lo_r2 = min(r2, r2f)
        x, y = _offset_with_d2(lo_r2)
        assert cc.cloud_dist2(0, 0, 0, float(x), float(y), 0) == lo_r2
        want = 2 if lo_r2 < r2 else 1
        assert list(stub_counts(cc, np.array([[0, 0, 0], [x, y, 0]], np.float32), r)) == [want, want]
    # itself and its duplicates count; k <= min_pts is an outlier
    xyz = np.array([[0, 0, 0]] * 3 + [[5, 5, 5]] * 2 + [[9, 9, 9]], np.float32)
    assert list(stub_counts(cc, xyz, 0.07)) == [3, 3, 3, 2, 2, 1]
    assert list(stub_outlier(cc, xyz, 0.07, 2)) == [0, 1, 2]
    assert list(stub_outlier(cc, xyz, 0.07, 1)) == [0, 1, 2, 3, 4]
    assert list(stub_outlier(cc, xyz, 0.07, 0)) == [0, 1, 2, 3, 4, 5]
    # non-finite points: counted by nobody, count 0, always removed
    xyz = np.array([[0, 0, 0], [np.nan, 0, 0], [0.01, 0, 0], [np.inf, 0, 0]], np.float32)
    assert list(stub_counts(cc, xyz, 0.07)) == [2, 0, 2, 0]
    assert list(stub_outlier(cc, xyz, 0.07, 0)) == [0, 2]
    # the cap reports min(count, cap)
    xyz = surface_cloud(3000, 5)
    exact = stub_counts(cc, xyz, 0.1)
    assert np.array_equal(stub_counts(cc, xyz, 0.1, cap=40), np.minimum(exact, 40))


def test_passthrough_rules(cc):
    lo = np.float32(0.003)
    below = np.nextafter(lo, np.float32(0))
    hi = np.float32(0.83)
    above = np.nextafter(hi, np.float32(1))
    xyz = np.array([[lo, 0, 0], [below, 0, 0], [hi, 5, 5], [above, 0, 0], [0.5, np.nan, 0], [0.5, 0, np.inf], [np.nan, 0, 0],
                    [0.4, -1e30, 1e30]], np.float32)
    assert list(stub_passthrough(cc, xyz)) == [0, 2, 7]                       # inclusive float bounds; non-finite dropped
    assert list(stub_passthrough(cc, xyz, negative=True)) == [1, 3]           # negative: outside, still finite only
    yz = np.array([[9, 0.5, 0], [9, 2, 0.5], [9, 0.5, 0.5], [9, np.nan, 0.5]], np.float32)
    assert list(stub_passthrough(cc, yz, axis=1, lo=0, hi=1)) == [0, 2]
    assert list(stub_passthrough(cc, yz, axis=2, lo=0.25, hi=1)) == [1, 2]
    assert list(stub_passthrough(cc, yz, axis=2, lo=0.25, hi=1, negative=True)) == [0]
    assert len(stub_passthrough(cc, np.zeros((0, 3), np.float32))) == 0


# ---------------------------------------------------------------- k nearest
@pytest.mark.parametrize("k", [1, 10, 32])
def test_knn_matches_brute_force(cc, k):
    xyz = surface_cloud(1500, 3)
    xyz[::97] = xyz[::97][::-1]                    # duplicates of other points (ties broken by index)
    xyz[5] = xyz[6]
    xyz[11, 1] = np.nan
    idx, d2 = stub_knn(cc, xyz, k)
    bi, bd = brute_knn(xyz, k)
    assert np.array_equal(idx, bi)
    assert np.array_equal(d2.view(np.uint32), bd.view(np.uint32))
    assert (idx[11] == -1).all() and np.isinf(d2[11]).all()


def test_knn_k_above_n_and_ties(cc):
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [-1, 0, 0]], np.float32)
    idx, d2 = stub_knn(cc, xyz, 6)
    assert list(idx[0]) == [0, 2, 1, 3, -1, -1] and list(idx[2]) == [0, 2, 1, 3, -1, -1]
    assert list(idx[1]) == [1, 0, 2, 3, -1, -1]
    assert list(d2[1][:4]) == [0, 1, 1, 4] and np.isinf(d2[1][4:]).all()


# ---------------------------------------------------------------- the eigen step and normals
def test_own_trigonometry(cc):
    rng = np.random.default_rng(0)
    for y, x in list(rng.normal(size=(500, 2)) * rng.choice([1e-6, 1, 1e6], (500, 1))) + [(0.0, 1.0), (1.0, 0.0), (0.0, -1.0),
                                                                                         (-0.0, -1.0), (0.0, 0.0), (-0.0, -0.0)]:
        assert abs(cc.cloud_atan2(y, x) - np.arctan2(y, x)) <= 4e-16 * max(1.0, abs(np.arctan2(y, x)))
        assert np.signbit(cc.cloud_atan2(y, x)) == np.signbit(np.arctan2(y, x))
    for t in np.linspace(0, np.pi / 3, 200):
        assert abs(cc.cloud_cos(t) - np.cos(t)) < 3e-16 and abs(cc.cloud_sin(t) - np.sin(t)) < 3e-16


def _np_normal(nb, p, vp=(0, 0, 0)):
    nb = np.asarray(nb, np.float64)
    c = np.cov(nb.T, bias=True)
    w, v = np.linalg.eigh(c)
    n = v[:, 0]
    if np.dot(np.asarray(vp) - p, n) < 0:
        n = -n
    return n, w[0] / w.sum()


@pytest.mark.parametrize("shape", ["plane", "curved"])
def test_normals_against_numpy_eigh(cc, shape):
    rng = np.random.default_rng(7)
    worst, worst_c = 0.0, 0.0
    for t in range(300):
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        uv = rng.uniform(-0.05, 0.05, (10, 2))
        h = 0.0 * uv[:, 0] if shape == "plane" else 3.0 * (uv[:, 0] ** 2 - 0.5 * uv[:, 1] ** 2)
        local = np.c_[uv, h + rng.normal(0, 1e-4, 10)]
        nb = (local @ R.T + rng.uniform(-2, 2, 3)).astype(np.float32)
        p = nb[0]
        got = normal_of_list(cc, nb, p)
        n, curv = _np_normal(nb, p.astype(np.float64))
        ang = np.degrees(np.arccos(min(1.0, abs(float(np.dot(got[:3], n))) / np.linalg.norm(got[:3]))))
        assert np.dot(got[:3], n) > 0                       # same side: the flip rule
        worst = max(worst, ang)
        worst_c = max(worst_c, abs(got[3] - curv))
    # float covariance of points 2 units from the origin with a 0.05 spread: ~1e-7 relative on E[ab] - E[a]E[b]
    assert worst < 0.5, worst
    assert worst_c < 2e-3, worst_c


def test_flip_rule_is_exact(cc):
    cov = np.array([1, 0, 0, 0, 2, 0, 0, 0, 3], np.float32)         # normal = +-x
    out = np.zeros(4, np.float32)
    for px, want in ((1.0, -1.0), (-1.0, 1.0), (0.0, None)):
        p = np.array([px, 0.5, 0.5], np.float32)
        vp = np.zeros(3, np.float32)
        cc.cloud_normal_from_cov(cov.ctypes.data, 10, p.ctypes.data, vp.ctypes.data, out.ctypes.data)
        if want is not None:
            assert abs(out[0]) == 1 and out[0] == want
        else:                                                          # (vp - p) . n == 0: not < 0, no flip
            ref = np.zeros(4, np.float32)
            cc.cloud_normal_from_cov(cov.ctypes.data, 10, np.array([0, 0, 0], np.float32).ctypes.data, vp.ctypes.data,
                                     ref.ctypes.data)
            assert out[0] == ref[0]
        assert out[3] == np.float32(1.0 / 6.0) or abs(out[3] - 1 / 6) < 1e-6


def test_fewer_than_three_neighbours_is_nan(cc):
    for cnt in (0, 1, 2):
        out = normal_of_list(cc, np.arange(3 * max(cnt, 1), dtype=np.float32).reshape(-1, 3)[:cnt], [0, 0, 0])
        assert (out.view(np.uint32) == NAN_BITS).all()
    xyz = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    assert (stub_normals(cc, xyz, 10).view(np.uint32) == NAN_BITS).all()


def test_degenerate_neighbourhoods(cc):
    # all identical (exact values): covariance 0 -> scale 1, roots 0, all crosses vanish -> NaN normal, curvature 0 (zero trace)
    out = normal_of_list(cc, np.full((10, 3), 0.5, np.float32), [0.5, 0.5, 0.5])
    assert (out[:3].view(np.uint32) == NAN_BITS).all() and out[3] == 0
    # collinear (exact, along x): eigenvalues (0, 0, s) -> the rows of M - 0 I span one direction: NaN normal, curvature 0
    nb = np.c_[np.arange(-4, 6, dtype=np.float32) * 0.25, np.zeros(10), np.zeros(10)].astype(np.float32)
    out = normal_of_list(cc, nb, nb[0])
    assert (out[:3].view(np.uint32) == NAN_BITS).all() and out[3] == 0
    # isotropic: the octahedron and its centre gives cov = (2/7) a^2 I exactly -> M - root I vanishes: NaN normal, curvature 1/3
    a = 0.5
    nb = np.array([[0, 0, 0], [a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, a], [0, 0, -a]], np.float32)
    out = normal_of_list(cc, nb, nb[0])
    assert (out[:3].view(np.uint32) == NAN_BITS).all()
    assert abs(out[3] - 1.0 / 3.0) < 1e-6
    val, vec = np.zeros(1, np.float32), np.zeros(3, np.float32)
    cov = np.diag([2.0, 2.0, 2.0]).astype(np.float32).ravel()
    cc.cloud_eigen33(cov.ctypes.data, val.ctypes.data, vec.ctypes.data)
    assert val[0] == 2 and np.isnan(vec).all()


def test_roots_match_numpy(cc):
    rng = np.random.default_rng(3)
    for _ in range(300):
        A = rng.normal(size=(3, 3))
        m = (A @ A.T / np.abs(A @ A.T).max()).astype(np.float32)
        r = np.zeros(3, np.float32)
        cc.cloud_roots(m.ravel().copy().ctypes.data, r.ctypes.data)
        w = np.linalg.eigvalsh(m.astype(np.float64))
        assert np.all(np.diff(r) >= 0)
        assert np.allclose(r, w, atol=3e-5), (r, w)


def test_normals_of_a_cloud(cc):
    xyz = surface_cloud(3000, 9, outliers=0.0)
    got = stub_normals(cc, xyz, 10)
    idx, _ = stub_knn(cc, xyz, 10)
    for i in range(0, 3000, 37):
        want = normal_of_list(cc, xyz[idx[i]], xyz[i])
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32))
        n, _ = _np_normal(xyz[idx[i]], xyz[i].astype(np.float64))
        assert abs(float(np.dot(got[i, :3], n))) > 0.999


# ---------------------------------------------------------------- sanitizers
def test_cloud_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cloud_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DCLOUD_MAIN", "-o", exe, STUB])
    xyz = surface_cloud(4000, 2, scale=0.4)
    xyz[3] = [np.nan, 0, 0]
    xyz[4] = xyz[5]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(xyz)))
        f.write(xyz.astype("<f4").tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("passthrough ")


# ---------------------------------------------------------------- the PCD reader (pcllite.h)
def load_pcd(cc, path, cap=1 << 16):
    xyz = np.zeros((cap, 3), np.float32)
    info, org = np.zeros(3, np.int32), np.zeros(3, np.float32)
    n = cc.cloud_load_pcd(str(path).encode(), xyz.ctypes.data, cap, info.ctypes.data, org.ctypes.data)
    return (None if n < 0 else xyz[:n].copy()), info, org


def _ply(xyz):
    head = "ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" \
           "property uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\nend_header\n" % len(xyz)
    return head + "".join("%.9g %.9g %.9g 10 20 30\n" % tuple(p) for p in xyz)


def test_pcd_round_trip_with_the_ply_converter(cc, tmp_path):
    rng = np.random.default_rng(4)
    xyz = rng.normal(size=(300, 3)).astype(np.float32)
    (tmp_path / "m.ply").write_text(_ply(xyz))
    exe = build.build_io_demo()
    r = subprocess.run([exe, "--ply2pcd", str(tmp_path / "m.ply"), str(tmp_path / "MAP3D.pcd")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and int(r.stdout) == 300
    got, info, org = load_pcd(cc, tmp_path / "MAP3D.pcd")
    p8 = np.array([np.float32("%.8g" % v) for v in xyz.ravel()], np.float32).reshape(xyz.shape)   # the writer's precision(8)
    assert np.array_equal(got, p8)
    assert list(info) == [300, 1, 1] and list(org) == [0, 0, 0]
    # the writer's "nan" for a non-finite coordinate reads back as NaN, and the cloud is not dense
    (tmp_path / "n.pcd").write_bytes(_pcd_head(2, "x y z rgb", "4 4 4 4", "F F F F", "ascii") + b"nan 1 2 0\n0.5 -1.25 3 0\n")
    got, info, _ = load_pcd(cc, tmp_path / "n.pcd")
    assert np.isnan(got[0, 0]) and list(got[1]) == [0.5, -1.25, 3] and list(info) == [2, 1, 0]


def _pcd_head(n, fields, sizes, types, data, vp="0 0 0 1 0 0 0"):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT %s\nPOINTS %d\nDATA %s\n" % (fields, sizes, types, " ".join("1" * len(fields.split())), n, vp, n, data)).encode()


def test_pcd_binary_and_failures(cc, tmp_path):
    rng = np.random.default_rng(5)
    n = 100
    rec = np.zeros(n, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<f4")]))
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    rec["x"], rec["y"], rec["z"] = xyz.T
    (tmp_path / "b.pcd").write_bytes(_pcd_head(n, "x y z rgb", "4 4 4 4", "F F F F", "binary", vp="1 2 3 1 0 0 0") + rec.tobytes())
    got, info, org = load_pcd(cc, tmp_path / "b.pcd")
    assert np.array_equal(got, xyz) and list(info) == [n, 1, 1] and list(org) == [1, 2, 3]
    # a field order with extra fields and a double z
    rec2 = np.zeros(n, np.dtype([("i", "<f4"), ("z", "<f8"), ("x", "<f4"), ("y", "<f4")]))
    rec2["x"], rec2["y"], rec2["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2].astype(np.float64)
    (tmp_path / "b2.pcd").write_bytes(_pcd_head(n, "intensity z x y", "4 8 4 4", "F F F F", "binary") + rec2.tobytes())
    got, _, _ = load_pcd(cc, tmp_path / "b2.pcd")
    assert np.array_equal(got, xyz)
    # truncated binary and ascii files, a missing file, a compressed file
    (tmp_path / "t.pcd").write_bytes(_pcd_head(n, "x y z rgb", "4 4 4 4", "F F F F", "binary") + rec.tobytes()[:-1])
    assert load_pcd(cc, tmp_path / "t.pcd")[0] is None
    (tmp_path / "ta.pcd").write_bytes(_pcd_head(3, "x y z", "4 4 4", "F F F", "ascii") + b"1 2 3\n4 5 6\n7 8\n")
    assert load_pcd(cc, tmp_path / "ta.pcd")[0] is None
    assert load_pcd(cc, tmp_path / "none.pcd")[0] is None
    (tmp_path / "c.pcd").write_bytes(_pcd_head(n, "x y z rgb", "4 4 4 4", "F F F F", "binary_compressed") + b"\0" * 64)
    r = subprocess.run(["python", "-c", "import sys; sys.path.insert(0, %r); from tests.test_cloud_cpu import load_stub, load_pcd; "
                        "print(load_pcd(load_stub(%r), %r)[0] is None)" % (ROOT, cc._name, str(tmp_path / "c.pcd"))],
                       capture_output=True, text=True, timeout=60)
    assert r.stdout.strip() == "True" and "binary_compressed is not supported" in r.stderr
