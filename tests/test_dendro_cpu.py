"""Dendrometry (csrc/dendro.h, DESIGN.md f-11: height, DBH, stem profile, crown base, crown spread) on the CPU, through a
g++ build of the header the device code compiles (tests/stub/dendro_capi.cpp): a literal Python transcription of rules
3-10 (hash included) against the stub's slice tables, planted trees against their truth and against scipy's geometric
circle fit, the scene variants (a 200-degree arc, clutter, a rotated frame, a scale, labels), and the rule cases built by
hand.  No GPU.  The reference has no implementation to compare with (src/DendrometryE.cpp:3-29 prints blanks)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.optimize import least_squares

from sfm_danpipeline_amd.dendro import SLICE_DTYPE, DendroOpts, DendroResult, set_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "dendro_capi.cpp")
MAX_SLICES, BINS, GN_STEPS = 4096, 1024, 10
EMPTY, DBH_ONE, DBH_NONE, NO_CROWN = 1, 2, 4, 8
RESULT_FIELDS = [f for f, _ in DendroResult._fields_]
# the worst |dbh / yardstick - 1| over the planted scenes below (full ring, 200-degree arc, clutter, taper, rotated, scaled):
# 8.8e-4, on the 200-degree arc with clutter (DESIGN.md f-11 records it); the test asserts at twice it
DBH_WORST = 8.8e-4


@pytest.fixture(scope="module")
def dn(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dendro") / "libdendrocapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci, u32, f64 = C.c_void_p, C.c_int, C.c_uint32, C.c_double
    lib.dnd_default_opts.argtypes = [vp]
    lib.dnd_default_opts.restype = None
    lib.dnd_sizes.argtypes = [vp, vp, vp]
    lib.dnd_run.argtypes = [ci, vp, vp, C.c_int32, vp, ci, vp, ci, vp, vp, vp]
    lib.dnd_fit_slice.argtypes = [vp, ci, ci, vp, vp]
    lib.dnd_winner.argtypes = [vp, ci, ci, vp]
    lib.dnd_hash.argtypes = [u32, u32, u32, u32]
    lib.dnd_hash.restype = u32
    lib.dnd_sector.argtypes = [f64, f64]
    lib.dnd_key.argtypes = [ci, ci, C.c_uint]
    lib.dnd_key.restype = C.c_uint64
    lib.dnd_circle.argtypes = [vp, f64, f64, vp]
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_dendro.py)
def stub_opts(dn, **kw):
    o = DendroOpts()
    dn.dnd_default_opts(C.byref(o))
    return set_opts(o, **kw)


def result_tuple(r):
    return tuple(getattr(r, f) for f in RESULT_FIELDS)


def result_bytes(r):
    return bytes(memoryview(r))


def stub_run(dn, xyz, labels=None, label=0, opts=None, threads=16, want_frame=False):
    """(DendroResult, rows, frame or None); None when the options are refused."""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32))
    opts = opts or stub_opts(dn)
    res, rows, m = DendroResult(), np.zeros(MAX_SLICES, SLICE_DTYPE), C.c_int32(0)
    frame = np.zeros((max(len(xyz), 1), 3), np.float32) if want_frame else None
    rc = dn.dnd_run(len(xyz), xyz.ctypes.data, None if lab is None else lab.ctypes.data, label, C.byref(opts), threads, C.byref(res),
                    MAX_SLICES, rows.ctypes.data, C.byref(m), None if frame is None else frame.ctypes.data)
    if rc != 0:
        return None
    return res, rows[:m.value].copy(), (frame[:len(xyz)] if want_frame else None)


def stub_winner(dn, en, k=0, opts=None):
    """The iteration that wins rule 5 on the slice (-1: none)."""
    en = np.ascontiguousarray(np.asarray(en, np.float32).reshape(-1, 2))
    pad = np.concatenate([en, np.zeros((1, 2), np.float32)])
    return dn.dnd_winner(pad.ctypes.data, len(en), k, C.byref(opts or stub_opts(dn)))


def stub_fit_slice(dn, en, k=0, opts=None):
    en = np.ascontiguousarray(np.asarray(en, np.float32).reshape(-1, 2))
    row = np.zeros(1, SLICE_DTYPE)
    pad = np.concatenate([en, np.zeros((1, 2), np.float32)])
    assert dn.dnd_fit_slice(pad.ctypes.data, len(en), k, C.byref(opts or stub_opts(dn)), row.ctypes.data) == 0
    return row[0]


# ---------------------------------------------------------------- planted trees
def trunk(rng, n, r0=0.15, r1=0.15, arc=360.0, height=4.0, sigma=0.005):
    z = rng.uniform(0, height, n)
    a = np.deg2rad(rng.uniform(-arc / 2, arc / 2, n))
    r = r0 + (r1 - r0) * z / height + rng.normal(0, sigma, n)
    return np.stack([r * np.cos(a), r * np.sin(a), z], 1)


def crown(rng, n, sigma=0.005):
    a, c = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1, 1, n)
    s = np.sqrt(1 - c * c)
    d = 1 + rng.normal(0, sigma, n) / 2.0
    return np.stack([2.0 * s * np.cos(a) * d, 1.5 * s * np.sin(a) * d, 6.5 + 2.5 * c * d], 1)


def clutter(rng, n, height=4.0):
    return np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0, height, n)], 1)


TOP = 9.05      # the planted top: above the crown's noisy apex (9 + 5 sigma of the shell's noise is 9.03)


def planted(seed=0, n=60000, r0=0.15, r1=0.15, arc=360.0, clutter_frac=0.0):
    """(xyz float32 [n, 3], the trunk's points): trunk 0 .. 4 with a point at height 0, crown shell around 6.5, one point at TOP."""
    rng = np.random.default_rng(seed)
    nt = n // 3
    t = trunk(rng, nt, r0, r1, arc)
    t[0] = (r0, 0, 0)                                  # the ground and the top are planted exactly
    cr = crown(rng, n - nt - int(clutter_frac * nt))
    cr[0] = (0, 0, TOP)
    parts = [t, cr]
    if clutter_frac:
        parts.append(clutter(rng, int(clutter_frac * nt)))
    xyz = np.concatenate(parts)
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(np.float32), t.astype(np.float32)


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def scipy_circle(xy, x0):
    """The geometric least-squares circle through xy (float64 [m, 2]) from the start x0 = (a, b, r)."""
    f = lambda p: np.hypot(xy[:, 0] - p[0], xy[:, 1] - p[1]) - p[2]
    return least_squares(f, x0, xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0).x


# ---------------------------------------------------------------- the transcription of rules 3-10
M32 = 0xFFFFFFFF


def py_mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def py_hash(seed, k, j, d):
    x = py_mix((seed + 0x9E3779B9) & M32)
    x = py_mix(x ^ k)
    x = py_mix(((x + 0x85EBCA6B) & M32) ^ j)
    x = py_mix(((x + 0xC2B2AE35) & M32) ^ d)
    return x


def py_frame(o):
    up, north = np.array(o.up[:]), np.array(o.north[:])
    d = (north[0] * up[0] + north[1] * up[1]) + north[2] * up[2]
    n = north - d * up
    n = n / math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    e = np.array([n[1] * up[2] - n[2] * up[1], n[2] * up[0] - n[0] * up[2], n[0] * up[1] - n[1] * up[0]])
    return e, n, up


def py_sectors(dx, dy):
    ax, ay = np.abs(dx), np.abs(dy)
    steep = ay > ax
    lo, hi = np.where(steep, ax, ay), np.where(steep, ay, ax)
    half = lo > hi * 0.41421356237309503
    s = np.where(steep, np.where(half, 2, 3), np.where(half, 1, 0))
    return np.where(dx >= 0, np.where(dy >= 0, s, 15 - s), np.where(dy >= 0, 7 - s, 8 + s))


def py_circle(p1, p2, p3, r_min, r_max):
    x1, y1 = float(p1[0]), float(p1[1])
    bx, by, cx, cy = float(p2[0]) - x1, float(p2[1]) - y1, float(p3[0]) - x1, float(p3[1]) - y1
    det = 2.0 * (bx * cy - by * cx)
    if det == 0.0 or det != det:
        return None
    b2, c2 = bx * bx + by * by, cx * cx + cy * cy
    ux, uy = (cy * b2 - by * c2) / det, (bx * c2 - cx * b2) / det
    r = math.sqrt(ux * ux + uy * uy)
    if not (r_min <= r <= r_max):
        return None
    c = (x1 + ux, y1 + uy, r)
    return c if math.isfinite(c[0]) and math.isfinite(c[1]) else None


def py_sum(terms, pos, nk):
    full = np.zeros(((nk + 255) // 256) * 256)
    full[pos] = terms
    acc = np.zeros(256)
    for row in full.reshape(-1, 256):
        acc = acc + row
    v = acc
    for w in range(4):
        off = 32
        while off >= 1:
            v[64 * w:64 * w + off] = v[64 * w:64 * w + off] + v[64 * w + off:64 * w + 2 * off]
            off >>= 1
    return (v[0] + v[64]) + (v[128] + v[192])


def py_solve2(s, N):
    mpp, mpq, mqq = s[0] - s[3] * s[3] / N, s[1] - s[3] * s[4] / N, s[2] - s[4] * s[4] / N
    gp, gq = s[5] - s[3] * s[7] / N, s[6] - s[4] * s[7] / N
    return mpp, mpq, mqq, gp, gq, mpp * mqq - mpq * mpq


def py_hypothesis(en, o, k, j, r_min, r_max):
    nk = len(en)
    ids = [(py_hash(o.seed, k, j, d) * nk) >> 32 for d in range(3)]
    if len(set(ids)) < 3:
        return None
    return py_circle(en[ids[0]], en[ids[1]], en[ids[2]], r_min, r_max)


def py_fit_slice(en, k, o, lengths):
    """One SLICE_DTYPE row (extent NaN) and the winner's inlier positions, by rules 5 and 6."""
    t, tol, r_min, r_max = lengths
    nan = float("nan")
    row = np.zeros(1, SLICE_DTYPE)[0]
    row["count"] = nk = len(en)
    for f in ("ce", "cn", "radius", "rms", "extent"):
        row[f] = nan
    if nk < o.min_slice_pts:
        return row, None
    x, y = en[:, 0].astype(np.float64), en[:, 1].astype(np.float64)
    best, best_c = 0, None
    for j in range(o.ransac_iters):
        c = py_hypothesis(en, o, k, j, r_min, r_max)
        if c is None:
            continue
        dx, dy = x - c[0], y - c[1]
        inl = np.abs(np.sqrt(dx * dx + dy * dy) - c[2]) <= tol
        cnt = int(inl.sum())
        if cnt == 0:
            continue
        mask = 0
        for s in np.unique(py_sectors(dx[inl], dy[inl])):
            mask |= 1 << int(s)
        key = (cnt << 32) | ((4095 - j) << 16) | mask
        if key > best:
            best, best_c = key, (c, inl, mask, cnt)
    if best == 0:
        return row, None
    c, inl, mask, cnt = best_c
    row["inliers"], row["mask"] = cnt, mask
    if cnt < o.min_inliers or bin(mask).count("1") < o.min_sectors:
        return row, None
    row["stem"] = 1
    pos = np.nonzero(inl)[0]
    u, v = x[pos] - c[0], y[pos] - c[1]
    N = float(cnt)
    z = u * u + v * v
    s = [py_sum(q, pos, nk) for q in (u * u, u * v, v * v, u, v, u * z, v * z, z)]
    a, b, r = 0.0, 0.0, c[2]
    cuu, cuv, cvv, cuz, cvz, det = py_solve2(s, N)
    if det > 0.0:
        ka, kb = (cuz * cvv - cvz * cuv) / (2.0 * det), (cvz * cuu - cuz * cuv) / (2.0 * det)
        cc = -((s[7] - 2.0 * ka * s[3]) - 2.0 * kb * s[4]) / N
        r2 = (ka * ka + kb * kb) - cc
        if r2 > 0.0 and math.isfinite(r2) and math.isfinite(ka) and math.isfinite(kb):
            a, b, r = ka, kb, math.sqrt(r2)
    for _ in range(GN_STEPS):
        du, dv = u - a, v - b
        d = np.sqrt(du * du + dv * dv)
        with np.errstate(invalid="ignore", divide="ignore"):
            p, q = np.where(d > 0.0, du / d, 0.0), np.where(d > 0.0, dv / d, 0.0)
        res = d - r
        s = [py_sum(w, pos, nk) for w in (p * p, p * q, q * q, p, q, p * res, q * res, res)]
        mpp, mpq, mqq, gp, gq, det = py_solve2(s, N)
        if not det > 0.0:
            continue
        da, db = (gp * mqq - gq * mpq) / det, (gq * mpp - gp * mpq) / det
        dr = ((s[7] - s[3] * da) - s[4] * db) / N
        na, nb, nr = a + da, b + db, r + dr
        if math.isfinite(na) and math.isfinite(nb) and math.isfinite(nr) and nr > 0.0:
            a, b, r = na, nb, nr
    du, dv = u - a, v - b
    res = np.sqrt(du * du + dv * dv) - r
    row["rms"] = math.sqrt(py_sum(res * res, pos, nk) / N)
    row["ce"], row["cn"], row["radius"] = c[0] + a, c[1] + b, r
    return row, pos


def py_run(xyz, labels, label, o):
    """(dict of the result's fields, rows, frame) by rules 1-10, written from DESIGN.md f-11 with numpy and plain loops."""
    nan = float("nan")
    out = dict(total_height=nan, dbh=nan, dbh_e=nan, dbh_n=nan, crown_base_height=nan, live_crown=nan, spread_ns=nan, spread_ew=nan,
               ground=nan, n_selected=0, n_slices=0, crown_base_slice=-1, flags=EMPTY)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    E, Nn, U = py_frame(o)
    t, tol, r_min, r_max = o.slice / o.scale, o.inlier_tol / o.scale, o.r_min / o.scale, o.r_max / o.scale
    binw, dbh_h = o.extent_bin / o.scale, o.dbh_height / o.scale
    p = xyz.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fr = np.stack([((A[0] * p[:, 0] + A[1] * p[:, 1]) + A[2] * p[:, 2]).astype(np.float32) for A in (E, Nn, U)], 1)
    sel = np.isfinite(xyz).all(1) & np.isfinite(fr).all(1)
    if labels is not None:
        sel &= np.asarray(labels) == label
    fr[~sel] = np.nan
    rows = np.zeros(0, SLICE_DTYPE)
    if not sel.any():
        return out, rows, fr
    h = fr[:, 2].astype(np.float64)
    hmax = float(h[sel].max())
    h0 = float(h[sel].min()) if math.isnan(o.ground) else o.ground / o.scale
    if not hmax - h0 >= 0.0:
        return out, rows, fr
    S = int(min(math.floor((hmax - h0) / t), MAX_SLICES - 1)) + 1
    with np.errstate(invalid="ignore"):
        kk = np.where(sel & (h - h0 >= 0.0), np.minimum(np.floor((h - h0) / t), S - 1), -1).astype(np.int64)
    members = [np.nonzero(kk == k)[0] for k in range(S)]            # ascending input index
    rows = np.zeros(S, SLICE_DTYPE)
    for k in range(S):
        rows[k], _ = py_fit_slice(fr[members[k], :2], k, o, (t, tol, r_min, r_max))
    # rule 7
    x = dbh_h / t - 0.5
    kf = math.floor(x)
    lo, hi = int(kf), int(kf) + 1
    slo, shi = 0 <= lo < S and rows[lo]["stem"] == 1, 0 <= hi < S and rows[hi]["stem"] == 1
    flags, r_dbh, ce, cn = 0, nan, nan, nan
    if slo and shi:
        w = x - kf
        r_dbh = rows[lo]["radius"] + w * (rows[hi]["radius"] - rows[lo]["radius"])
        ce = rows[lo]["ce"] + w * (rows[hi]["ce"] - rows[lo]["ce"])
        cn = rows[lo]["cn"] + w * (rows[hi]["cn"] - rows[lo]["cn"])
    elif slo or shi:
        one = rows[lo] if slo else rows[hi]
        r_dbh, ce, cn, flags = one["radius"], one["ce"], one["cn"], DBH_ONE
    else:
        flags = DBH_NONE
    # rule 8
    if not flags & DBH_NONE:
        for k in range(S):
            nk = len(members[k])
            if nk == 0:
                continue
            de, dn_ = fr[members[k], 0].astype(np.float64) - ce, fr[members[k], 1].astype(np.float64) - cn
            b = np.minimum(np.floor(np.sqrt(de * de + dn_ * dn_) / binw), BINS - 1).astype(np.int64)
            need = int(min(max(math.ceil(o.extent_q * nk), 1), nk))
            cum = np.cumsum(np.bincount(b, minlength=BINS))
            rows[k]["extent"] = float(np.nonzero(cum >= need)[0][0] + 1) * binw
    # rule 9
    cb = -1
    if not math.isnan(r_dbh):
        lim = o.crown_factor * r_dbh
        for k in range(0, S - o.crown_run + 1):
            if (k + 0.5) * t > dbh_h and all(rows[m]["count"] >= o.min_slice_pts and rows[m]["extent"] > lim for m in range(k, k + o.crown_run)):
                cb = k
                break
    out.update(n_selected=int(sel.sum()), n_slices=S, flags=flags, ground=h0 * o.scale, total_height=(hmax - h0) * o.scale,
               dbh=2.0 * r_dbh * o.scale, dbh_e=ce * o.scale, dbh_n=cn * o.scale, crown_base_slice=cb)
    if cb >= 0:
        with np.errstate(invalid="ignore"):
            top = h >= h0 + cb * t
        out["crown_base_height"] = cb * t * o.scale
        out["live_crown"] = out["total_height"] - out["crown_base_height"]
        out["spread_ew"] = (float(fr[top, 0].max()) - float(fr[top, 0].min())) * o.scale
        out["spread_ns"] = (float(fr[top, 1].max()) - float(fr[top, 1].min())) * o.scale
    else:
        out["flags"] |= NO_CROWN
    return out, rows, fr


def same(a, b):
    return a == b or (a != a and b != b)


def assert_same_result(res, want):
    for f in RESULT_FIELDS:
        assert same(getattr(res, f), want[f]), (f, getattr(res, f), want[f])


# ---------------------------------------------------------------- scenes (shared with the GPU test)
def scenes(dn_opts, n=60000):
    """name -> (xyz, labels, label, opts, trunk points in the scene's coordinates, metres per unit)."""
    out = {}
    xyz, t = planted(1, n)
    out["ring"] = (xyz, None, 0, dn_opts(), t, 1.0)
    xyz, t = planted(2, n, arc=200.0)
    out["arc200"] = (xyz, None, 0, dn_opts(), t, 1.0)
    xyz, t = planted(3, n, arc=200.0, clutter_frac=0.3)
    out["arc200_clutter"] = (xyz, None, 0, dn_opts(), t, 1.0)
    xyz, t = planted(4, n, r0=0.18, r1=0.12)
    out["taper"] = (xyz, None, 0, dn_opts(seed=7), t, 1.0)
    xyz, t = planted(5, n)
    R = rotation(5)                                                  # columns: east, north, up of the tilted scene
    out["rotated"] = ((xyz.astype(np.float64) @ R.T).astype(np.float32), None, 0,
                      dn_opts(up=R[:, 2], north=R[:, 1] + 0.3 * R[:, 2]), t, 1.0)
    xyz, t = planted(6, n)
    out["scaled"] = ((xyz / np.float32(0.37)).astype(np.float32), None, 0, dn_opts(scale=0.37), t, 1.0)
    xyz, t = planted(7, n)
    rng = np.random.default_rng(70)
    other = (clutter(rng, n // 10) + (6.0, 1.0, -0.5)).astype(np.float32)
    lab = np.concatenate([np.full(len(xyz), 2, np.int32), np.full(len(other), 5, np.int32)])
    perm = rng.permutation(len(lab))
    out["labels"] = (np.concatenate([xyz, other])[perm], lab[perm], 2, dn_opts(), t, 1.0)
    return out


@pytest.fixture(scope="module")
def runs(dn):
    """Every scene through the stub, once."""
    sc = scenes(lambda **kw: stub_opts(dn, **kw))
    return {name: (s, stub_run(dn, s[0], s[1], s[2], s[3], want_frame=True)) for name, s in sc.items()}


# ---------------------------------------------------------------- tests
def test_struct_sizes_match_the_header(dn):
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    dn.dnd_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(DendroOpts), SLICE_DTYPE.itemsize, C.sizeof(DendroResult))
    o = stub_opts(dn)
    assert (tuple(o.up), tuple(o.north), o.scale, o.dbh_height, o.slice, o.ransac_iters) == ((0, 0, 1), (0, 1, 0), 1.0, 1.3, 0.1, 256)
    assert math.isnan(o.ground) and (o.inlier_tol, o.r_min, o.r_max, o.min_inliers, o.min_sectors) == (0.02, 0.02, 1.5, 20, 6)
    assert (o.extent_q, o.extent_bin, o.crown_factor, o.crown_run, o.min_slice_pts, o.seed) == (0.95, 0.05, 3.0, 3, 10, 1)


def test_hash_sector_and_key_follow_the_rules(dn):
    for a in [(1, 0, 0, 0), (1, 5, 200, 2), (0xDEADBEEF, 4095, 4095, 1), (0, 0, 0, 0)]:
        assert dn.dnd_hash(*a) == py_hash(*a)
    ang = np.deg2rad(np.arange(16) * 22.5 + 11.25)
    assert [dn.dnd_sector(math.cos(a), math.sin(a)) for a in ang] == list(range(16))
    assert [int(s) for s in py_sectors(np.cos(ang), np.sin(ang))] == list(range(16))
    assert dn.dnd_key(30, 7, 0x00FF) > dn.dnd_key(30, 8, 0xFFFF) > dn.dnd_key(29, 0, 0xFFFF)   # count first, then the lower j


@pytest.mark.parametrize("name", ["ring", "arc200_clutter", "rotated", "scaled", "labels"])
def test_transcription_gives_the_same_tables(runs, name):
    (xyz, lab, label, o, _, _), (res, rows, frame) = runs[name]
    want, wrows, wframe = py_run(xyz, lab, label, o)
    assert np.array_equal(frame.view(np.uint32), wframe.view(np.uint32))
    assert rows.tobytes() == wrows.tobytes()
    assert_same_result(res, want)


def test_refit_equals_scipys_geometric_fit_on_the_same_inliers(dn):
    """360 / 200 / 120 degree arcs with 30 % clutter: the refit against least_squares on the winner's inlier set."""
    rng = np.random.default_rng(11)
    o = stub_opts(dn)
    worst = 0.0
    for case in range(30):
        arc = (360.0, 200.0, 120.0)[case % 3]
        m = 400 + 37 * case
        a = np.deg2rad(rng.uniform(-arc / 2, arc / 2, m))
        r = 0.15 + rng.normal(0, 0.005, m)
        en = np.concatenate([np.stack([r * np.cos(a) + 0.3, r * np.sin(a) - 0.2], 1), rng.uniform(-1, 1, (int(0.3 * m), 2))])
        en = en[rng.permutation(len(en))].astype(np.float32)
        row = stub_fit_slice(dn, en, k=case, opts=o)
        prow, pos = py_fit_slice(en, case, o, (0.1, 0.02, 0.02, 1.5))
        assert row.tobytes() == prow.tobytes()
        if not row["stem"]:
            continue
        ref = scipy_circle(en[pos].astype(np.float64), (row["ce"], row["cn"], row["radius"]))
        got = np.array([row["ce"], row["cn"], row["radius"]])
        worst = max(worst, float(np.abs(got - ref).max() / ref[2]))
    print("refit vs scipy, worst relative:", worst)
    assert worst <= 1e-8


def test_dbh_against_the_planted_trunk(runs):
    worst = {}
    for name, ((xyz, lab, label, o, t, _), (res, rows, frame)) in runs.items():
        near = t[(t[:, 2] >= 1.2) & (t[:, 2] < 1.4)].astype(np.float64)
        ref = scipy_circle(near[:, :2], (0.0, 0.0, 0.15))
        assert res.flags == 0, name
        worst[name] = abs(res.dbh / (2 * ref[2]) - 1)
    print("dbh vs scipy on the planted trunk:", worst)
    assert max(worst.values()) <= 2 * DBH_WORST, worst


def test_height_crown_base_and_spread(runs):
    # the analytic crown: a dense sample of the shell, its 0.95-quantile radius per slice against 3 r
    rng = np.random.default_rng(99)
    cr = crown(rng, 2000000, sigma=0.0)
    k = np.floor(cr[:, 2] / 0.1).astype(int)
    rad = np.hypot(cr[:, 0], cr[:, 1])
    q95 = np.array([np.quantile(rad[k == s], 0.95) if (k == s).any() else 0.0 for s in range(92)])
    for name, ((xyz, lab, label, o, t, _), (res, rows, frame)) in runs.items():
        assert res.n_slices == 91 and abs(res.ground) < 1e-6, name
        # the planted ground point is at 0 and the top at TOP: three float32 inputs and one float32 frame coordinate, half an
        # ulp of TOP each (the rotated scene), plus the same for the ground
        assert abs(res.total_height - TOP) <= 4 * 2.0 ** -23 * TOP + 1e-6, (name, res.total_height)
        if name == "arc200_clutter":
            # 30 % clutter out to 1.4 from the trunk IS the 0.95-quantile of rule 8 in every trunk slice: the rule finds a
            # "crown" at the first slice above the DBH height, as written; the crown assertions need an uncluttered stem
            assert res.crown_base_slice == 13
            continue
        r_dbh = res.dbh / 2
        over = q95 > 3 * r_dbh
        want = next(s for s in range(14, 88) if over[s] and over[s + 1] and over[s + 2])
        assert abs(res.crown_base_slice - want) <= 1, (name, res.crown_base_slice, want)
        assert res.crown_base_height == res.crown_base_slice * (o.slice / o.scale) * o.scale
        assert res.live_crown == res.total_height - res.crown_base_height
        top = frame[:, 2].astype(np.float64) >= res.ground / o.scale + res.crown_base_slice * (o.slice / o.scale)
        assert res.spread_ew == (float(frame[top, 0].max()) - float(frame[top, 0].min())) * o.scale, name
        assert res.spread_ns == (float(frame[top, 1].max()) - float(frame[top, 1].min())) * o.scale, name
        assert abs(res.spread_ew - 4.0) < 0.05 and abs(res.spread_ns - 3.0) < 0.05, name


def test_taper_profile_follows_the_planted_radii(runs):
    (_, _, _, o, _, _), (res, rows, _) = runs["taper"]
    stem = rows[:38]
    assert stem["stem"].all()
    want = 0.18 - 0.06 * (np.arange(38) + 0.5) * 0.1 / 4.0
    assert np.abs(stem["radius"] / want - 1).max() < 0.01


# ---------------------------------------------------------------- rule cases by hand
def ring(m, r=0.2, arc=360.0, c=(0.0, 0.0)):
    a = np.deg2rad(np.arange(m) * arc / m)
    return np.stack([r * np.cos(a) + c[0], r * np.sin(a) + c[1]], 1).astype(np.float32)


RULE_SLICES = {
    "n0": ring(0), "n1": ring(1), "n2": ring(2), "n3": ring(3), "n9": ring(9), "n64": ring(64), "n65": ring(65), "n256": ring(256),
    "n257": ring(257), "collinear": np.stack([np.arange(40) * 0.01, np.arange(40) * 0.02], 1).astype(np.float32),
    "identical": np.full((40, 2), 0.25, np.float32), "quarter": ring(200, arc=90.0),
    "three_collinear": np.array([[0, 0], [0.1, 0.1], [0.2, 0.2]], np.float32),
}


def test_rule_case_slices(dn):
    o = stub_opts(dn)
    rows = {name: stub_fit_slice(dn, en, k=3, opts=o) for name, en in RULE_SLICES.items()}
    for name in ("n0", "n1", "n2", "n3", "n9", "three_collinear"):               # below min_slice_pts: no RANSAC at all
        assert (rows[name]["stem"], rows[name]["inliers"], rows[name]["count"]) == (0, 0, len(RULE_SLICES[name])), name
    for name in ("n64", "n65", "n256", "n257"):
        m = len(RULE_SLICES[name])
        assert rows[name]["stem"] == 1 and rows[name]["inliers"] == m and rows[name]["mask"] == 0xFFFF, name
        assert abs(rows[name]["radius"] - 0.2) < 1e-6 and rows[name]["rms"] < 1e-6, name
    assert rows["collinear"]["stem"] == 0 and rows["identical"]["stem"] == 0
    assert rows["identical"]["inliers"] == 0                                     # every draw is degenerate: determinant 0
    q = rows["quarter"]                                                          # a full count, but 4 or 5 sectors of 16
    assert q["stem"] == 0 and q["inliers"] == 200 and bin(q["mask"]).count("1") < 6
    assert stub_fit_slice(dn, RULE_SLICES["quarter"], k=3, opts=stub_opts(dn, min_sectors=4))["stem"] == 1
    for name, en in RULE_SLICES.items():
        prow, _ = py_fit_slice(en, 3, o, (0.1, 0.02, 0.02, 1.5))
        assert rows[name].tobytes() == prow.tobytes(), name


def test_count_tie_goes_to_the_lower_iteration(dn):
    """An exact ring: every valid hypothesis counts all 64 points, so all valid iterations tie and the first must win."""
    en = RULE_SLICES["n64"]
    o = stub_opts(dn, ransac_iters=64)
    valid = [j for j in range(64) if py_hypothesis(en, o, 5, j, 0.02, 1.5) is not None]
    first = valid[0]
    assert len(valid) >= 2 and first + 1 < 64                    # a later hypothesis that ties really exists
    for j in valid[:4]:                                          # ... and ties: alone, each of them counts every point
        x, y = en[:, 0].astype(np.float64), en[:, 1].astype(np.float64)
        c = py_hypothesis(en, o, 5, j, 0.02, 1.5)
        assert (np.abs(np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - c[2]) <= 0.02).all()
    assert stub_winner(dn, en, 5, o) == first
    assert stub_winner(dn, en, 5, stub_opts(dn, ransac_iters=valid[1] + 1)) == first
    row, _ = py_fit_slice(en, 5, o, (0.1, 0.02, 0.02, 1.5))
    alone = stub_fit_slice(dn, en, k=5, opts=stub_opts(dn, ransac_iters=first + 1))
    assert stub_fit_slice(dn, en, k=5, opts=o).tobytes() == alone.tobytes() == row.tobytes()
    if first > 0:
        assert stub_winner(dn, en, 5, stub_opts(dn, ransac_iters=first)) == -1


def pole(with_crown=False, drop=()):
    """A thin exact pole 0 .. 3 of 60-point rings every 2 cm, without the rings of the slices in `drop`."""
    z = np.arange(0, 150) * 0.02 + 0.005
    pts = np.concatenate([np.concatenate([ring(60, 0.1), np.full((60, 1), h, np.float32)], 1) for h in z if int(h / 0.1) not in drop])
    return pts.astype(np.float32)


def test_flag_bits(dn):
    g = stub_opts(dn, ground=0.0)                                              # (slices 0.1 k .. 0.1 (k + 1), as pole() drops them)
    res, rows, _ = stub_run(dn, pole(), opts=g)
    assert res.flags == NO_CROWN and math.isnan(res.crown_base_height) and math.isnan(res.spread_ns) and abs(res.dbh - 0.2) < 1e-5
    assert res.crown_base_slice == -1 and rows["stem"].all()
    res, rows, _ = stub_run(dn, pole(drop=(12,)), opts=g)
    assert res.flags == NO_CROWN | DBH_ONE and abs(res.dbh - 0.2) < 1e-5 and rows[12]["count"] == 0
    res, rows, _ = stub_run(dn, pole(drop=(12, 13)), opts=g)
    assert res.flags == NO_CROWN | DBH_NONE and math.isnan(res.dbh) and np.isnan(rows["extent"]).all()
    res, rows, _ = stub_run(dn, pole(), labels=np.zeros(len(pole()), np.int32), label=3)
    assert res.flags == EMPTY and len(rows) == 0 and math.isnan(res.total_height) and res.n_selected == 0
    res, rows, _ = stub_run(dn, np.zeros((0, 3), np.float32))
    assert res.flags == EMPTY
    res, rows, _ = stub_run(dn, np.full((5, 3), np.nan, np.float32))
    assert res.flags == EMPTY
    res, rows, _ = stub_run(dn, pole(), opts=stub_opts(dn, ground=10.0))       # nothing at or above the ground
    assert res.flags == EMPTY


def test_nan_points_change_nothing(dn):
    xyz, _ = planted(8, 6000)
    res, rows, _ = stub_run(dn, xyz)
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 2], [0, 0, -np.inf], [3e38, 3e38, 3e38]], np.float32)
    mixed = np.concatenate([bad[:2], xyz[:100], bad[2:], xyz[100:]])
    res2, rows2, _ = stub_run(dn, mixed, opts=stub_opts(dn, up=(0.6, 0.0, 0.8), north=(0, 1, 0)))   # (3e38 leaves float32 here)
    res3, rows3, _ = stub_run(dn, mixed)
    assert res3.n_selected == len(xyz) + 1 and res2.n_selected == len(xyz)
    res4, rows4, _ = stub_run(dn, np.concatenate([bad[:3], xyz]))
    assert result_bytes(res4) == result_bytes(res) and rows4.tobytes() == rows.tobytes()


def test_single_slice_and_thread_count(dn):
    xyz, _ = planted(9, 3000)
    o = stub_opts(dn, slice=20.0)
    res, rows, _ = stub_run(dn, xyz, opts=o, threads=1)
    assert res.n_slices == 1 and rows[0]["count"] == 3000
    res16, rows16, _ = stub_run(dn, xyz, opts=o, threads=16)
    assert result_bytes(res) == result_bytes(res16) and rows.tobytes() == rows16.tobytes()


@pytest.mark.parametrize("kw", [dict(up=(0, 0, 1.001)), dict(up=(0, 0, 0)), dict(north=(0, 0, 1)), dict(north=(0, 0, 0)), dict(scale=0.0),
                                dict(scale=-1.0), dict(slice=0.0), dict(ransac_iters=0), dict(ransac_iters=4097), dict(r_max=0.01),
                                dict(r_min=-0.1), dict(dbh_height=float("inf")), dict(dbh_height=float("nan")), dict(min_sectors=-1),
                                dict(inlier_tol=-1.0), dict(extent_q=0.0), dict(extent_q=1.5), dict(extent_bin=0.0), dict(crown_factor=0.0),
                                dict(min_inliers=0), dict(min_sectors=17), dict(crown_run=0), dict(min_slice_pts=2),
                                dict(ground=float("inf")), dict(scale=float("nan"))])
def test_refusals(dn, kw):
    assert stub_run(dn, pole(), opts=stub_opts(dn, **kw)) is None
