"""Shared by tests/test_pnp_cpu.py and tests/test_gpu_pnp.py: the g++ build of tests/stub/pnp_capi.cpp (csrc/pnp.h on one
CPU thread), numpy geometry that owes nothing to that header, and the synthetic scenes (a non-planar cloud in front of a
camera with the temple's K)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "pnp_capi.cpp")
K = np.array([[1520.4, 0.0, 302.32], [0.0, 1525.9, 246.87], [0.0, 0.0, 1.0]])   # tests/golden/temple calibration
DIST0 = np.zeros(5)
DIST1 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])   # a small non-zero k1 k2 p1 p2 k3


def build_stub(dirpath):
    so = os.path.join(str(dirpath), "libpnpcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.pnp_sincos.argtypes = [C.c_double, vp]
    L.pnp_sincos.restype = None
    L.pnp_acos.argtypes = [C.c_double]
    L.pnp_acos.restype = C.c_double
    L.pnp_rodrigues_to_matrix.argtypes = [vp, vp]
    L.pnp_rodrigues_to_matrix.restype = None
    L.pnp_rodrigues_to_vector.argtypes = [vp, vp]
    L.pnp_samples.argtypes = [C.c_int, C.c_int, vp]
    L.pnp_samples.restype = None
    L.pnp_sample.argtypes = [vp] * 5
    L.pnp_count.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_double, vp]
    L.pnp_epnp.argtypes = [C.c_int] + [vp] * 6
    L.pnp_ransac.argtypes = [C.c_int] + [vp] * 6 + [C.c_double, C.c_int] + [vp] * 11
    return L


def _pack(xyz_list, xy_list):
    off = np.concatenate([[0], np.cumsum([len(a) for a in xyz_list])]).astype(np.int32)
    if off[-1]:
        xyz = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in xyz_list]))
        xy = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float64).reshape(-1, 2) for b in xy_list]))
    else:
        xyz, xy = np.zeros((1, 3)), np.zeros((1, 2))
    return off, xyz, xy


def stub_epnp(L, xyz_list, xyn_list):
    n = len(xyz_list)
    off, xyz, xy = _pack(xyz_list, xyn_list)
    R, t, fl = np.zeros((n, 9)), np.zeros((n, 3)), C.c_int32(0)
    assert L.pnp_epnp(n, off.ctypes.data, xyz.ctypes.data, xy.ctypes.data, R.ctypes.data, t.ctypes.data, C.addressof(fl)) == 0
    return R.reshape(-1, 3, 3), t, fl.value


def stub_ransac(L, xyz_list, xy_list, Kmat, dist, thresholds=None, confidence=0.99, max_iters=1000):
    """the stub's twin of sfm_danpipeline_amd.pnp.pnp_ransac (same result dict)"""
    n = len(xyz_list)
    off, xyz, xy = _pack(xyz_list, xy_list)
    if thresholds is None:
        thresholds = [0.006 * float(np.max(b)) if len(b) else 0.0 for b in xy_list]
    thr = np.ascontiguousarray(np.asarray(thresholds, np.float64))
    Kc, dc = np.ascontiguousarray(np.asarray(Kmat, np.float64).reshape(9)), np.ascontiguousarray(np.asarray(dist, np.float64))
    m = max(n, 1)
    status, inl, its = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    vec = [np.zeros((m, 3)) for _ in range(6)]
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    fl = C.c_int32(0)
    assert L.pnp_ransac(n, off.ctypes.data, xyz.ctypes.data, xy.ctypes.data, Kc.ctypes.data, dc.ctypes.data, thr.ctypes.data,
                        float(confidence), int(max_iters), status.ctypes.data, *[v.ctypes.data for v in vec], inl.ctypes.data,
                        mask.ctypes.data, its.ctypes.data, C.addressof(fl)) == 0
    return dict(status=status[:n], rvec=vec[0][:n], tvec=vec[1][:n], rvec_ransac=vec[2][:n], tvec_ransac=vec[3][:n],
                rvec_refit=vec[4][:n], tvec_refit=vec[5][:n], inliers=inl[:n], iterations=its[:n],
                masks=[mask[off[i]:off[i + 1]].copy() for i in range(n)], flags=fl.value)


# ---------------------------------------------------------------- numpy geometry (independent of csrc/pnp.h)
def rot(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rot_angle(Ra, Rb):
    """the angle of Ra Rb^T, accurate for small angles (from the skew part) and for large ones (from the trace)"""
    E = Ra @ Rb.T
    s = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    c = 0.5 * (np.trace(E) - 1)
    return float(np.arctan2(s, c))


def project(X, R, t, Kmat, dist):
    Xc = np.asarray(X) @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * Kmat[0, 0] + Kmat[0, 2], yd * Kmat[1, 1] + Kmat[1, 2]], 1)


def normalise(xy, Kmat, dist, iters=40):
    """pixels -> undistorted normalised coordinates, iterated to convergence"""
    x0 = (xy[:, 0] - Kmat[0, 2]) / Kmat[0, 0]
    y0 = (xy[:, 1] - Kmat[1, 2]) / Kmat[1, 1]
    k1, k2, p1, p2, k3 = dist
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        ic = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return np.stack([x, y], 1)


def scene(seed, n, dist=DIST0, noise=0.0, outliers=0.0, outlier_shift=0.0):
    """n points of a non-planar cloud about 6 units in front of a rotated, shifted camera.  Returns dict(R, t, X, xy, truth
    (1 = inlier)); outliers: the fraction of points whose pixel is displaced by at least outlier_shift pixels."""
    g = np.random.default_rng(seed)
    R = rot(g.normal(0, 0.4, 3))
    t = np.array([0.0, 0.0, 6.0]) + g.normal(0, 0.5, 3)
    X = g.uniform(-0.6, 0.6, (n, 3))
    xy = project(X, R, t, K, dist)
    if noise:
        xy = xy + g.normal(0, noise, xy.shape)
    truth = np.ones(n, np.uint8)
    n_out = int(round(outliers * n))
    if n_out:
        idx = g.choice(n, n_out, replace=False)
        ang = g.uniform(0, 2 * np.pi, n_out)
        rad = outlier_shift * g.uniform(1.0, 2.0, n_out)
        xy[idx] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        truth[idx] = 0
    return dict(R=R, t=t, X=X, xy=xy, truth=truth)


def posed_scene(seed, n, R=None, tz=6.0, scale=(0.6, 0.6, 0.6), dist=DIST0, noise=0.0):
    """scene with the rotation (None: scene's own draw), the depth and the per-axis half extent of the cloud as arguments;
    the camera's shift grows with the depth (tz / 6 of scene's), so a near camera keeps the cloud in front of it.  With the
    defaults it is scene(seed, n, dist, noise) bit for bit (test_pnp_cpu.py asserts it)."""
    g = np.random.default_rng(seed)
    own = rot(g.normal(0, 0.4, 3))
    R = own if R is None else np.asarray(R, np.float64)
    t = np.array([0.0, 0.0, tz]) + (tz / 6.0) * g.normal(0, 0.5, 3)
    half = np.asarray(scale, np.float64)
    X = g.uniform(-half, half, (n, 3))
    xy = project(X, R, t, K, dist)
    if noise:
        xy = xy + g.normal(0, noise, xy.shape)
    return dict(R=R, t=t, X=X, xy=xy, truth=np.ones(n, np.uint8))


def axis_rotation(axis, angle):
    """the rotation by angle about axis (any length), from rot"""
    a = np.asarray(axis, np.float64)
    return rot(a / np.linalg.norm(a) * angle)


def _random_axis(seed):
    a = np.random.default_rng(90000 + seed).normal(0, 1, 3)
    return a / np.linalg.norm(a)


def slab(ratio):
    """the family of clouds whose z extent is `ratio` of the other two"""
    return lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, scale=(0.6, 0.6, 0.6 * ratio), dist=dist, noise=noise)


# geometry off scene's default: name -> f(seed, n, dist, noise)
FAMILIES = {
    "half_turn": lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, R=axis_rotation(_random_axis(seed), np.pi), dist=dist, noise=noise),
    "half_turn_1e-7": lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, R=axis_rotation(_random_axis(seed), np.pi - 1e-7), dist=dist,
                                                                         noise=noise),
    "identity": lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, R=np.eye(3), dist=dist, noise=noise),
    "near": lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, tz=1.5, scale=(0.3, 0.3, 0.3), dist=dist, noise=noise),
    "far60": lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, tz=60.0, dist=dist, noise=noise),
    "far150": lambda seed, n, dist=DIST0, noise=0.0: posed_scene(seed, n, tz=150.0, scale=(15.0, 15.0, 15.0), dist=dist, noise=noise),
    "slab_1e-1": slab(1e-1), "slab_1e-2": slab(1e-2), "slab_1e-3": slab(1e-3), "slab_1e-4": slab(1e-4), "slab_1e-5": slab(1e-5),
}


def outlier_scene(seed, n, frac, dist=DIST0):
    """ransac_scene with the outlier share as an argument: frac of the points displaced by >= 20 thresholds, 0.5 px
    inlier noise, the reference's threshold"""
    base = scene(seed, n, dist, noise=0.5)
    thr = 0.006 * float(base["xy"].max())
    sc = scene(seed, n, dist, noise=0.5, outliers=frac, outlier_shift=30 * thr)
    sc["thr"] = 0.006 * float(sc["xy"].max())
    return sc


def nonfinite_scene(L, bad):
    """ransac_scene(3, 300, DIST1) with `bad` in one coordinate of the 3-D point that the first sample draws first and in
    one of the 2-D point that the second sample draws first, so that solves meet them.  Returns (scene, the two rows)."""
    sc = ransac_scene(3, 300, DIST1)
    samp = np.zeros(10, np.int32)
    L.pnp_samples(300, 2, samp.ctypes.data)
    i, j = int(samp[0]), int(samp[5])
    assert i != j
    X, xy = sc["X"].copy(), sc["xy"].copy()
    X[i, 1] = bad
    xy[j, 0] = bad
    return dict(sc, X=X, xy=xy), (i, j)


def ransac_scene(seed, n, dist=DIST0):
    """30 % outliers displaced by >= 20 thresholds, 0.5 px inlier noise, the reference's threshold"""
    base = scene(seed, n, dist, noise=0.5)
    thr = 0.006 * float(base["xy"].max())
    sc = scene(seed, n, dist, noise=0.5, outliers=0.3, outlier_shift=30 * thr)   # (>= 20 of the final thresholds: the test asserts it)
    sc["thr"] = 0.006 * float(sc["xy"].max())
    return sc
