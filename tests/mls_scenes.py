"""What the moving-least-squares tests share (tests/test_mls_cpu.py, tests/test_mls_sanitizers_cpu.py, tests/test_gpu_mls.py):
the build of the CPU stub (tests/stub/mls_capi.cpp over csrc/mls.h) with numpy-facing wrappers, the scenes, and a numpy float64
restatement of the rules M1-M7 of include/sfmhip.h that shares nothing with the header: a brute-force float32 radius search,
libm's exp, numpy's sums in its own order and numpy's Cholesky."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "mls_capi.cpp")
NAN_BITS = 0x7FC00000
OK, ERR_ARG = 0, -3
STATS = ("n_out", "n_dropped", "n_plane_only", "n_degenerate", "n_fit_failed", "max_neighbours")


def build_stub(directory):
    so = str(directory / "libmlscapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp, ci, f64 = C.c_void_p, C.c_int, C.c_double
    lib.mls_exp.argtypes = [ci, vp, vp]
    lib.mls_exp.restype = None
    lib.mls_grid.argtypes = [ci, vp, f64, vp, vp, vp]
    lib.mls_run.argtypes = [ci, vp, f64, ci, ci, f64, ci, vp, vp, vp, vp, vp]
    return lib


def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stub_exp(lib, x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.empty_like(x)
    lib.mls_exp(len(x), x.ctypes.data, y.ctypes.data)
    return y


def stub_grid(lib, xyz, radius):
    """(cell, D[3], keys[n]) of M2's grid"""
    xyz = _f(xyz)
    cell, D, keys = np.zeros(1), np.zeros(3, np.int32), np.zeros(max(len(xyz), 1), np.int32)
    assert lib.mls_grid(len(xyz), xyz.ctypes.data, float(radius), cell.ctypes.data, D.ctypes.data, keys.ctypes.data) == OK
    return float(cell[0]), D, keys[:len(xyz)]


def stub_mls(lib, xyz, radius, order=2, normals=True, sqr_gauss=0.0, search=0):
    """(status, dict as cloud.Cloud.mls returns it, without `cloud`); the outputs start as a pattern, so a refusal shows
    them untouched"""
    xyz = _f(xyz)
    n1 = max(len(xyz), 1)
    oxyz, on4, src = np.full((n1, 3), 7.5, np.float32), np.full((n1, 4), 7.5, np.float32), np.full(n1, 77, np.int32)
    m, st = np.full(1, -9, np.int32), np.full(6, -9, np.int32)
    rc = lib.mls_run(len(xyz), xyz.ctypes.data, float(radius), int(order), int(bool(normals)), float(sqr_gauss), int(search),
                     oxyz.ctypes.data, on4.ctypes.data, src.ctypes.data, m.ctypes.data, st.ctypes.data)
    if rc != OK:
        return rc, {"xyz": oxyz, "normals": on4, "src_index": src, "n_out": int(m[0])}
    k = int(m[0])
    return rc, {"xyz": oxyz[:k].copy(), "normals": on4[:k].copy() if normals else None, "src_index": src[:k].copy(),
                "stats": dict(zip(STATS, (int(v) for v in st)))}


# ---- scenes

def noisy_plane(n, seed, sigma=0.005):
    """(points, unit normal, offset) of a tilted unit square with Gaussian noise along the normal: n.x = offset on the plane"""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    a = np.cross(nrm, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    uv = rng.uniform(0, 1, (n, 2))
    xyz = uv[:, :1] * a + uv[:, 1:] * b + 0.4 * nrm + rng.normal(0, sigma, (n, 1)) * nrm
    return xyz.astype(np.float32), nrm, 0.4


def sphere_cap(n, seed, sigma=0.0005, half_angle=0.5):
    """(points, centre, radius) of a cap of the unit sphere around +z, uniform in area, with radial Gaussian noise"""
    rng = np.random.default_rng(seed)
    cz = 1.0 - rng.uniform(0, 1, n) * (1.0 - math.cos(half_angle))
    ph = rng.uniform(0, 2 * math.pi, n)
    s = np.sqrt(1.0 - cz * cz)
    d = np.stack([s * np.cos(ph), s * np.sin(ph), cz], 1)
    centre = np.array([0.2, -0.1, 0.3])
    return (centre + d * (1.0 + rng.normal(0, sigma, (n, 1)))).astype(np.float32), centre, 1.0


def surface_cloud(n, seed, sigma=0.002):
    """a smooth height field over the unit square with noise: a scanned surface"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    z = 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y) + 0.1 * x * y + rng.normal(0, sigma, n)
    return np.stack([x, y, z], 1).astype(np.float32)


def radius_for(k, n, area):
    """the radius whose disc holds about k of n points spread over `area`"""
    return math.sqrt(k * area / (n * math.pi))


# ---- the rules in numpy float64

def neighbours(xyz, radius):
    """M1: a boolean [n, n] matrix by the float32 d2 and (float)(r * r); rows and columns of non-finite points are False"""
    x = _f(xyz)
    fin = np.isfinite(x).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, None, :] - x[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        nb = d2 < np.float32(float(radius) * float(radius))
    return nb & fin[:, None] & fin[None, :]


def _eigen33(cov):
    """pcl::eigen33 in double with libm's trigonometry: (smallest eigenvalue, its vector with eigen33's sign)"""
    scale = np.abs(cov).max()
    if scale <= np.finfo(np.float64).tiny:
        scale = 1.0
    m = cov / scale

    def roots2(b, c):
        d = max(b * b - 4.0 * c, 0.0)
        return [0.0, 0.5 * (b - math.sqrt(d)), 0.5 * (b + math.sqrt(d))]

    c0 = (m[0, 0] * m[1, 1] * m[2, 2] + 2.0 * m[0, 1] * m[0, 2] * m[1, 2] - m[0, 0] * m[1, 2] ** 2 - m[1, 1] * m[0, 2] ** 2 -
          m[2, 2] * m[0, 1] ** 2)
    c1 = m[0, 0] * m[1, 1] - m[0, 1] ** 2 + m[0, 0] * m[2, 2] - m[0, 2] ** 2 + m[1, 1] * m[2, 2] - m[1, 2] ** 2
    c2 = m[0, 0] + m[1, 1] + m[2, 2]
    if abs(c0) < np.finfo(np.float64).eps:
        r = roots2(c2, c1)
    else:
        c2_3 = c2 / 3.0
        a_3 = min((c1 - c2 * c2_3) / 3.0, 0.0)
        half_b = 0.5 * (c0 + c2_3 * (2.0 * c2_3 * c2_3 - c1))
        q = min(half_b * half_b + a_3 ** 3, 0.0)
        rho, theta = math.sqrt(-a_3), math.atan2(math.sqrt(-q), half_b) / 3.0
        ct, st = math.cos(theta), math.sin(theta)
        r = sorted([c2_3 + 2.0 * rho * ct, c2_3 - rho * (ct + math.sqrt(3.0) * st), c2_3 - rho * (ct - math.sqrt(3.0) * st)])
        if r[0] <= 0.0:
            r = roots2(c2, c1)
    m = m - r[0] * np.eye(3)
    v = [np.cross(m[0], m[1]), np.cross(m[0], m[2]), np.cross(m[1], m[2])]
    l = [float(w @ w) for w in v]
    k = 0 if l[0] >= l[1] and l[0] >= l[2] else 1 if l[1] >= l[0] and l[1] >= l[2] else 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return r[0] * scale, v[k] / math.sqrt(l[k])


def reference_mls(xyz, radius, order=2, sqr_gauss=0.0):
    """M1-M7 point by point in float64; a dict as stub_mls returns it (normals always), the outputs float64"""
    x32 = _f(xyz)
    x = x32.astype(np.float64)
    nb = neighbours(x32, radius)
    g = float(sqr_gauss) if sqr_gauss > 0 else float(radius) * float(radius)
    nc = (order + 1) * (order + 2) // 2
    st = dict.fromkeys(STATS, 0)
    oxyz, on4, src = [], [], []
    for i in range(len(x)):
        if not np.isfinite(x[i]).all():
            continue
        P = x[nb[i]]
        k = len(P)
        st["max_neighbours"] = max(st["max_neighbours"], k)
        if k < 3:
            st["n_dropped"] += 1
            continue
        mean = P.mean(0)
        cov = (P[:, :, None] * P[:, None, :]).mean(0) - np.outer(mean, mean)
        lam, n = _eigen33(cov)
        src.append(i)
        if not np.isfinite(n).all():
            st["n_degenerate"] += 1
            oxyz.append(x[i])
            on4.append([np.nan] * 4)
            continue
        q = x[i] - (x[i] @ n - n @ mean) * n
        tr = np.trace(cov)
        curv = abs(lam / tr) if tr != 0 else 0.0
        normal = n
        if order > 0 and k < nc:
            st["n_plane_only"] += 1
        elif order > 0:
            if not abs(n[0]) <= 1e-12 * abs(n[2]) or not abs(n[1]) <= 1e-12 * abs(n[2]):
                va = np.array([-n[1], n[0], 0.0]) / math.hypot(n[0], n[1])
            else:
                va = np.array([0.0, -n[2], n[1]]) / math.hypot(n[1], n[2])
            ua = np.cross(n, va)
            e = P - q
            w = np.exp(-(e * e).sum(1) / g)
            u, v, f = e @ ua, e @ va, e @ n
            T = np.stack([u ** a * v ** b for a in range(order + 1) for b in range(order + 1 - a)], 1)
            A, rhs = (T * w[:, None]).T @ T, (T * w[:, None]).T @ f
            try:
                L = np.linalg.cholesky(A)
                c = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
                ok = bool(np.isfinite(c).all())
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                q = q + c[0] * n
                normal = n - c[order + 1] * ua - c[1] * va
                normal = normal / np.linalg.norm(normal)
            else:
                st["n_fit_failed"] += 1
        oxyz.append(q)
        on4.append([normal[0], normal[1], normal[2], curv])
    st["n_out"] = len(src)
    return {"xyz": np.array(oxyz, np.float64).reshape(-1, 3), "normals": np.array(on4, np.float64).reshape(-1, 4),
            "src_index": np.array(src, np.int32), "stats": st}
