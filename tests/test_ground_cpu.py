"""The ground-plane fit (csrc/ground.h, DESIGN.md f-12: RANSAC plane, refit, orientation, the frame the dendrometry measures
in) on the CPU, through a g++ build of the header the device code compiles (tests/stub/ground_capi.cpp): a literal Python
transcription of rules 1-8 (hash, fixed-order sums and the 3 x 3 Jacobi SVD included) against the stub byte for byte, the
rule cases built by hand, the accuracy against numpy's SVD plane fit of the planted ground points, the wall scenes, a
sphere shell, and the way into the dendrometry (ground plane -> options -> dnd_run on a rotated, scaled tree).  No GPU."""
import ctypes as C
import ctypes.util
import math
import os
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd.ground import GroundOpts, GroundResult, set_opts
from tests.test_dendro_cpu import dn, planted, py_hash, py_sum, rotation, stub_opts as dendro_opts, stub_run as dendro_run  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "ground_capi.cpp")
FEW, NO_PLANE, REFIT_KEPT, NORTH_REPLACED = 1, 2, 4, 8
STREAM = 0x67726E64
RESULT_FIELDS = [f for f, _ in GroundResult._fields_]
TOL = 0.04                 # the accuracy scenes' tolerance (cloud units of the upright scene); ground noise sigma = TOL / 4
# the worst figures over ACCURACY_SCENES against numpy's SVD plane fit of the planted ground points alone (DESIGN.md f-12
# records them): the angle between the normals in radians, the offset difference in units of tol; the tests assert at twice them
ANGLE_WORST = 2.2e-6
OFFSET_WORST = 2.2e-3
# ... and of the levelled dendrometry against the same tree upright: |dbh / dbh_upright - 1| and |height - height_upright| / tol
E2E_DBH_WORST = 6.3e-5
E2E_HEIGHT_WORST = 7.9e-3


@pytest.fixture(scope="module")
def gn(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ground") / "libgroundcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci, u32 = C.c_void_p, C.c_int, C.c_uint32
    lib.gnd_default_opts.argtypes = [vp]
    lib.gnd_default_opts.restype = None
    lib.gnd_sizes.argtypes = [vp, vp]
    lib.gnd_run.argtypes = [ci, vp, vp, C.c_int32, vp, vp, ci, ci, vp]
    lib.gnd_hypothesis.argtypes = [vp, ci, vp, ci, vp]
    lib.gnd_count.argtypes = [vp, ci, vp, vp, C.c_double, vp]
    lib.gnd_count.restype = None
    lib.gnd_orientation.argtypes = [vp, ci, ci, u32, u32]
    lib.gnd_north.argtypes = [vp, vp, vp]
    lib.gnd_opts_from_ground.argtypes = [vp, vp]
    lib.gnd_svd3.argtypes = [vp, vp, vp]
    lib.gnd_svd3.restype = None
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_ground.py)
def stub_opts(gn, **kw):
    o = GroundOpts()
    gn.gnd_default_opts(C.byref(o))
    return set_opts(o, **kw)


def result_bytes(r):
    return bytes(memoryview(r))


def stub_run(gn, xyz, labels=None, label=0, opts=None, cams=None, threads=16):
    """GroundResult; None when the options are refused."""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32))
    cm = None if cams is None else np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 3))
    opts = opts or stub_opts(gn)
    res = GroundResult()
    rc = gn.gnd_run(len(xyz), xyz.ctypes.data, None if lab is None else lab.ctypes.data, label, C.byref(opts),
                    None if cm is None else cm.ctypes.data, 0 if cm is None else len(cm), threads, C.byref(res))
    return None if rc != 0 else res


def stub_hypothesis(gn, pts, j, opts):
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    out = np.zeros(6)
    ok = gn.gnd_hypothesis(pts.ctypes.data, len(pts), C.byref(opts), j, out.ctypes.data)
    return ok, out[:3].copy(), out[3:].copy()


# ---------------------------------------------------------------- planted scenes
def disc(rng, n, radius=6.0, sigma=TOL / 4):
    a, r = rng.uniform(0, 2 * np.pi, n), radius * np.sqrt(rng.uniform(0, 1, n))
    return np.stack([r * np.cos(a), r * np.sin(a), rng.normal(0, sigma, n)], 1)


def wall(rng, n, x, height=8.0):
    return np.stack([x + rng.normal(0, TOL / 4, n), rng.uniform(-6, 6, n), rng.uniform(0, height, n)], 1)


def scene(seed, n_tree=20000, n_ground=20000, rot=None, scale=1.0, slope=0.0, extra=None):
    """A planted tree (tests/test_dendro_cpu.planted) on a noisy ground disc, rotated by `rot` and divided by `scale`:
    (xyz float32, labels: 0 ground, 1 tree, 2 extra, the ground points float64 in the scene's coordinates, R)."""
    rng = np.random.default_rng(1000 + seed)
    tree, _ = planted(seed, n_tree)
    g = disc(rng, n_ground)
    parts, labs = [g, tree.astype(np.float64)], [np.zeros(len(g), np.int32), np.ones(len(tree), np.int32)]
    if extra is not None:
        parts.append(extra)
        labs.append(np.full(len(extra), 2, np.int32))
    xyz, lab = np.concatenate(parts), np.concatenate(labs)
    if slope:                                            # the ground and everything on it tilted about the y axis
        c, s = math.cos(slope), math.sin(slope)
        xyz = xyz @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
    R = np.eye(3) if rot is None else rotation(rot)
    xyz = (xyz @ R.T) / scale
    perm = rng.permutation(len(xyz))
    xyz, lab = xyz[perm], lab[perm]
    return xyz.astype(np.float32), lab, xyz[lab == 0], R


def svd_plane(pts):
    """numpy's least-squares plane of float64 points: (unit normal, centroid)."""
    c = pts.mean(0)
    return np.linalg.svd(pts - c, full_matrices=False)[2][2], c


# ---------------------------------------------------------------- the transcription of rules 1-8
_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.hypot.argtypes = [C.c_double, C.c_double]
_libm.hypot.restype = C.c_double
DBL_EPS = 2.220446049250313e-16


def py_svd3(A):
    """csrc/jacobi.h's jacobi_svd<3, 3, 3, 3> on the rows of A, as far as W and Vt go (its tail only refills rows of At)."""
    At = [[float(A[i][k]) for k in range(3)] for i in range(3)]
    Vt = [[1.0 if i == k else 0.0 for k in range(3)] for i in range(3)]
    W = [0.0, 0.0, 0.0]
    eps = DBL_EPS * 10
    for i in range(3):
        sd = 0.0
        for k in range(3):
            sd += At[i][k] * At[i][k]
        W[i] = sd
    for _ in range(30):
        changed = False
        for i in range(2):
            for j in range(i + 1, 3):
                a, p, b = W[i], 0.0, W[j]
                for k in range(3):
                    p += At[i][k] * At[j][k]
                if abs(p) <= eps * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = _libm.hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    sn = math.sqrt(delta / gamma)
                    c = p / (gamma * sn * 2)
                else:
                    c = math.sqrt((gamma + beta) / (gamma * 2))
                    sn = p / (gamma * c * 2)
                a = b = 0.0
                for k in range(3):
                    t0 = c * At[i][k] + sn * At[j][k]
                    t1 = -sn * At[i][k] + c * At[j][k]
                    At[i][k], At[j][k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                for k in range(3):
                    t0 = c * Vt[i][k] + sn * Vt[j][k]
                    t1 = -sn * Vt[i][k] + c * Vt[j][k]
                    Vt[i][k], Vt[j][k] = t0, t1
        if not changed:
            break
    for i in range(3):
        sd = 0.0
        for k in range(3):
            sd += At[i][k] * At[i][k]
        W[i] = math.sqrt(sd)
    for i in range(2):
        j = i
        for k in range(i + 1, 3):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return W, Vt


def py_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def py_dist(a, n, x, y, z):
    return (n[0] * (x - a[0]) + n[1] * (y - a[1])) + n[2] * (z - a[2])


def py_prepare(o):
    hint = [float(v) for v in o.up_hint]
    hh = math.sqrt(py_dot(hint, hint))
    if not hh > 0.0:
        return None, -1.0
    return [v / hh for v in hint], math.cos(o.max_tilt_deg * (math.pi / 180.0))


def py_hypothesis(P, o, j, hint, cos_tilt):
    """(a, n) of iteration j over the float64 list P, None when rule 3 skips it."""
    ns = len(P)
    ia, ib, ic = [(py_hash(o.seed, STREAM, j, d) * ns) >> 32 for d in range(3)]
    if ia == ib or ia == ic or ib == ic:
        return None
    a, b, c = P[ia], P[ib], P[ic]
    u, v = [float(b[k]) - float(a[k]) for k in range(3)], [float(c[k]) - float(a[k]) for k in range(3)]
    m = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    mm = py_dot(m, m)
    if mm == 0.0 or not math.isfinite(mm):
        return None
    ln = math.sqrt(mm)
    n = [m[0] / ln, m[1] / ln, m[2] / ln]
    if hint is not None and abs(py_dot(n, hint)) < cos_tilt:
        return None
    return [float(a[0]), float(a[1]), float(a[2])], n


def py_orientation(n, cpos, cneg, pos, neg):
    if cpos != cneg:
        return 1 if cpos > cneg else -1
    if pos != neg:
        return 1 if pos > neg else -1
    f = n[0] if n[0] != 0.0 else (n[1] if n[1] != 0.0 else n[2])
    return -1 if f < 0.0 else 1


def py_north(up, hint):
    h = [float(v) for v in hint]
    hh = math.sqrt(py_dot(h, h))
    replaced = not hh > 0.0
    n, nn = None, 0.0
    if not replaced:
        h = [v / hh for v in h]
        d = py_dot(h, up)
        n = [h[k] - d * up[k] for k in range(3)]
        nn = math.sqrt(py_dot(n, n))
        replaced = not nn > 1e-6
    if replaced:
        ax = 0
        for k in (1, 2):
            if abs(up[k]) < abs(up[ax]):
                ax = k
        h = [1.0 if k == ax else 0.0 for k in range(3)]
        d = py_dot(h, up)
        n = [h[k] - d * up[k] for k in range(3)]
        nn = math.sqrt(py_dot(n, n))
    return [v / nn for v in n], replaced


def py_run(xyz, labels, label, o, cams=None):
    """The result's fields by rules 1-8, written from DESIGN.md f-12 with numpy and plain loops."""
    nan = float("nan")
    out = dict(up=[nan] * 3, north=[nan] * 3, offset=nan, rms=nan, tol=nan, n_selected=0, inliers=0, below=0, above=0, winner=-1, flags=FEW)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    sel = np.isfinite(xyz).all(1)
    if labels is not None:
        sel &= np.asarray(labels) == label
    pts = xyz[sel]                                        # ascending input index
    ns = out["n_selected"] = len(pts)
    if ns < 3:
        return out
    P = pts.astype(np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    if o.inlier_tol > 0.0:
        tol = o.inlier_tol
    else:
        d = pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64)
        tol = o.inlier_rel * math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    out["tol"] = tol
    hint, cos_tilt = py_prepare(o)
    cams = np.zeros((0, 3)) if cams is None else np.asarray(cams, np.float64).reshape(-1, 3)
    cap = math.floor(o.below_max * float(ns))
    best, best_plane = 0, None
    for j in range(o.ransac_iters):
        hyp = py_hypothesis(P, o, j, hint, cos_tilt)
        if hyp is None:
            continue
        a, n = hyp
        s = py_dist(a, n, x, y, z)
        inl, pos, neg = int((np.abs(s) <= tol).sum()), int((s > tol).sum()), int((s < -tol).sum())
        sc = [py_dist(a, n, c[0], c[1], c[2]) for c in cams]
        sign = py_orientation(n, sum(v > 0.0 for v in sc), sum(v < 0.0 for v in sc), pos, neg)
        below = neg if sign > 0 else pos
        if inl < o.min_inliers or below > cap:
            continue
        key = (inl << 32) | (4095 - j)
        if key > best:
            best, best_plane = key, (a, [v if sign > 0 else -v for v in n], j)
    if best == 0:
        out["flags"] = NO_PLANE
        return out
    a, n, jw = best_plane
    flags = 0
    for _ in range(o.refit_rounds):
        s = py_dist(a, n, x, y, z)
        pos_i = np.nonzero(np.abs(s) <= tol)[0]
        N = float(len(pos_i))
        if len(pos_i) < 3:
            flags |= REFIT_KEPT
            continue
        cen = [py_sum(v[pos_i], pos_i, ns) / N for v in (x, y, z)]
        dx, dy, dz = x[pos_i] - cen[0], y[pos_i] - cen[1], z[pos_i] - cen[2]
        cs = [py_sum(t, pos_i, ns) / N for t in (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)]
        _, Vt = py_svd3([[cs[0], cs[1], cs[2]], [cs[1], cs[3], cs[4]], [cs[2], cs[4], cs[5]]])
        v = Vt[2]
        with np.errstate(all="ignore"):
            ln = math.sqrt(py_dot(v, v))
            m = [v[0] / ln, v[1] / ln, v[2] / ln] if ln != 0.0 else [nan] * 3
        if not all(math.isfinite(t) for t in m + cen):
            flags |= REFIT_KEPT
            continue
        if py_dot(m, n) < 0.0:
            m = [-t for t in m]
        a, n = cen, m
    s = py_dist(a, n, x, y, z)
    pos_i = np.nonzero(np.abs(s) <= tol)[0]
    inl = len(pos_i)
    north, replaced = py_north(n, o.north_hint)
    out.update(up=n, north=north, offset=py_dot(n, a), winner=jw, flags=flags | (NORTH_REPLACED if replaced else 0), inliers=inl,
               above=int((s > tol).sum()), below=int((s < -tol).sum()),
               rms=math.sqrt(py_sum(s[pos_i] * s[pos_i], pos_i, ns) / float(inl)) if inl else nan)
    return out


def same(a, b):
    return a == b or (a != a and b != b)


def assert_same_result(res, want):
    for f in RESULT_FIELDS:
        got = getattr(res, f)
        if f in ("up", "north"):
            assert all(same(g, w) for g, w in zip(got, want[f])), (f, list(got), want[f])
        else:
            assert same(got, want[f]), (f, got, want[f])


# ---------------------------------------------------------------- scenes (shared with the GPU test)
def wall_scenes():
    """crossing: a wall with more points than the ground through the ground disc; edge: the same wall at x = 5.9."""
    rng = np.random.default_rng(77)
    return {"crossing": scene(31, 6000, 20000, rot=31, extra=wall(rng, 30000, 0.5)),
            "edge": scene(32, 6000, 20000, rot=32, extra=wall(rng, 30000, 5.9))}


def sphere(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    a, c = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1, 1, n)
    s = np.sqrt(1 - c * c)
    return np.stack([s * np.cos(a), s * np.sin(a), c], 1).astype(np.float32)


def transcription_cases(opts):
    """name -> (xyz, labels, label, opts, cams): what test_transcription walks and the GPU test repeats on the device."""
    out = {}
    for k, seed in enumerate((41, 42, 43)):
        xyz, lab, _, R = scene(seed, 3000, 3000, rot=seed)
        out["rot%d" % k] = (xyz, None, 0, opts(ransac_iters=64), None)
    xyz, lab, _, R = scene(44, 3000, 3000, rot=44, slope=0.2)
    out["slope"] = (xyz, None, 0, opts(ransac_iters=64, inlier_tol=TOL), None)
    xyz, lab, _, R = scene(45, 3000, 3000, rot=45)
    out["labels"] = (xyz, np.where(lab == 1, 4, 9).astype(np.int32), 9, opts(ransac_iters=64, min_inliers=50, refit_rounds=1), None)
    xyz, lab, _, R = scene(46, 3000, 3000, rot=46)
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 2], [0, 0, -np.inf]], np.float32)
    cams = (np.array([[3.0, 0, 1.5], [0, 3.0, 1.5], [-3.0, 0, 1.6]]) @ R.T)
    out["nan_cams_hint"] = (np.concatenate([bad[:2], xyz[:100], bad[2:], xyz[100:]]), None, 0,
                            opts(ransac_iters=64, up_hint=2.0 * R[:, 2], max_tilt_deg=30.0, north_hint=R[:, 1] + 0.2 * R[:, 2], refit_rounds=8), cams)
    out["three"] = (np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], np.float32), None, 0, opts(min_inliers=3, ransac_iters=64), None)
    return out


ACCURACY_SCENES = [dict(seed=s, rot=s) for s in (51, 52, 53, 54)] + [dict(seed=55, rot=55, slope=0.25), dict(seed=56, rot=56, scale=0.37),
                                                                      dict(seed=57, rot=None)]


# ---------------------------------------------------------------- tests
def test_struct_sizes_and_defaults(gn):
    a, b = C.c_int(), C.c_int()
    gn.gnd_sizes(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (C.sizeof(GroundOpts), C.sizeof(GroundResult)) == (96, 96)
    o = stub_opts(gn)
    assert (o.inlier_tol, o.inlier_rel, o.below_max, tuple(o.up_hint), o.max_tilt_deg, tuple(o.north_hint)) == (0.0, 0.005, 0.01, (0, 0, 0), 180.0, (0, 1, 0))
    assert (o.ransac_iters, o.min_inliers, o.refit_rounds, o.seed) == (512, 100, 2, 1)


def test_svd_transcription(gn):
    rng = np.random.default_rng(3)
    for case in range(20):
        B = rng.normal(size=(3, 3)) * (1.0, 1.0, 1e-3 if case % 2 else 1.0)
        A = np.ascontiguousarray(B.T @ B)
        W, Vt = np.zeros(3), np.zeros(9)
        gn.gnd_svd3(A.ctypes.data, W.ctypes.data, Vt.ctypes.data)
        pw, pvt = py_svd3(A)
        assert W.tolist() == pw and Vt.tolist() == [v for row in pvt for v in row]
        assert abs(abs(np.dot(Vt[6:], np.linalg.eigh(A)[1][:, 0])) - 1) < 1e-9


@pytest.mark.parametrize("name", ["rot0", "rot1", "rot2", "slope", "labels", "nan_cams_hint", "three"])
def test_transcription_gives_the_same_bytes(gn, name):
    xyz, lab, label, o, cams = transcription_cases(lambda **kw: stub_opts(gn, **kw))[name]
    res = stub_run(gn, xyz, lab, label, o, cams)
    want = py_run(xyz, lab, label, o, cams)
    assert_same_result(res, want)
    assert res.winner >= 0 and res.flags == 0
    assert result_bytes(stub_run(gn, xyz, lab, label, o, cams, threads=1)) == result_bytes(res)


def test_repeated_draw_and_collinear_triple_skip_the_iteration(gn):
    o = stub_opts(gn)
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    repeated = 0
    for j in range(64):
        ids = [(py_hash(o.seed, STREAM, j, d) * 5) >> 32 for d in range(3)]
        ok, a, n = stub_hypothesis(gn, pts, j, o)
        want = py_hypothesis(pts.astype(np.float64), o, j, None, -1.0)
        assert ok == (want is not None)
        if len(set(ids)) < 3:
            repeated += 1
            assert ok == 0
        if want is not None:
            assert (a.tolist(), n.tolist()) == want and a.tolist() == pts[ids[0]].tolist()
    assert 10 < repeated < 54                                         # both kinds really occur among the 64
    line = np.stack([np.arange(50), 2 * np.arange(50), -np.arange(50)], 1).astype(np.float32)      # exact: every cross product is 0
    assert all(stub_hypothesis(gn, line, j, o)[0] == 0 for j in range(64))
    assert stub_run(gn, line, opts=stub_opts(gn, min_inliers=3)).flags == NO_PLANE
    assert stub_run(gn, np.full((50, 3), 0.5, np.float32), opts=stub_opts(gn, min_inliers=3)).flags == NO_PLANE
    # the tilt limit: with a hint along z, a plane through the x axis tilted 45 degrees passes at 50 degrees and not at 40
    tilted = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1], [2, 1, 1], [3, 2, 2]], np.float32)
    j = next(j for j in range(64) if stub_hypothesis(gn, tilted, j, o)[0])
    assert stub_hypothesis(gn, tilted, j, stub_opts(gn, up_hint=(0, 0, 3), max_tilt_deg=50.0))[0] == 1
    assert stub_hypothesis(gn, tilted, j, stub_opts(gn, up_hint=(0, 0, 3), max_tilt_deg=40.0))[0] == 0
    assert stub_hypothesis(gn, tilted, j, stub_opts(gn, up_hint=(0, 0, -3), max_tilt_deg=50.0))[0] == 1      # |n . hint|


def grid_plane(m=30):
    g = np.arange(m, dtype=np.float64)
    return np.stack([np.repeat(g, m), np.tile(g, m), np.zeros(m * m)], 1)


def test_inlier_tie_goes_to_the_lowest_iteration(gn):
    """An exact plane: every hypothesis that is not skipped counts all 900 points, so they all tie and the first must win."""
    xyz = grid_plane().astype(np.float32)
    o = stub_opts(gn, ransac_iters=64, inlier_tol=0.1, refit_rounds=0)
    valid = [j for j in range(64) if py_hypothesis(xyz.astype(np.float64), o, j, None, -1.0) is not None]
    assert len(valid) >= 2
    res = stub_run(gn, xyz, opts=o)
    assert res.winner == valid[0] and res.inliers == 900 and res.below == 0 and res.above == 0 and res.rms == 0.0
    assert stub_run(gn, xyz, opts=stub_opts(gn, ransac_iters=valid[1] + 1, inlier_tol=0.1, refit_rounds=0)).winner == valid[0]
    assert result_bytes(stub_run(gn, xyz, opts=o, threads=1)) == result_bytes(stub_run(gn, xyz, opts=o, threads=7)) == result_bytes(res)
    assert tuple(res.up) in ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0))
    assert tuple(res.up) == (0.0, 0.0, 1.0)                          # both ties of rule 5: the first non-zero component is positive


def below_scene(n_below):
    """900 points of an exact plane, 100 off it: n_below at z = -1, the rest at z = 1 .. 2."""
    rng = np.random.default_rng(9)
    off = np.stack([rng.uniform(0, 29, 100), rng.uniform(0, 29, 100), rng.uniform(1, 2, 100)], 1)
    off[:n_below, 2] = -1.0
    return np.concatenate([grid_plane(), off]).astype(np.float32)


def test_below_max_at_equality_and_one_over(gn):
    o = stub_opts(gn, inlier_tol=0.1, min_inliers=500, below_max=0.01, ransac_iters=128)       # floor(0.01 * 1000) = 10
    res = stub_run(gn, below_scene(10), opts=o)
    assert res.flags == 0 and (res.inliers, res.below, res.above) == (900, 10, 90) and tuple(res.up) == (0.0, 0.0, 1.0)
    assert_same_result(res, py_run(below_scene(10), None, 0, o))
    res = stub_run(gn, below_scene(11), opts=o)
    assert res.flags == NO_PLANE and res.winner == -1 and math.isnan(res.offset) and math.isnan(res.up[0]) and res.tol == 0.1
    assert (res.n_selected, res.inliers, res.below, res.above) == (1000, 0, 0, 0)
    assert_same_result(res, py_run(below_scene(11), None, 0, o))
    assert stub_run(gn, below_scene(11), opts=stub_opts(gn, inlier_tol=0.1, min_inliers=500, below_max=0.011, ransac_iters=128)).below == 11


def test_each_orientation_rule(gn):
    n = np.array([0.0, -0.6, 0.8])
    ori = lambda cpos, cneg, pos, neg, v=n: gn.gnd_orientation(np.ascontiguousarray(v, np.float64).ctypes.data, cpos, cneg, pos, neg)
    assert ori(3, 1, 0, 100) == 1 and ori(1, 3, 100, 0) == -1                  # the centres decide, whatever the points say
    assert ori(2, 2, 100, 7) == 1 and ori(2, 2, 7, 100) == -1                  # a tie of the centres: the points
    assert ori(0, 0, 100, 7) == 1 and ori(0, 0, 7, 100) == -1                  # no centres: the points
    assert ori(2, 2, 5, 5) == -1 and ori(0, 0, 0, 0) == -1                     # both tied: the first non-zero component (-0.6) positive
    assert ori(0, 0, 5, 5, np.array([0.0, 0.0, 1.0])) == 1 and ori(0, 0, 5, 5, np.array([-1.0, 0.0, 0.0])) == -1
    # ... and through the whole call: 90 points above the plane and 10 below; centres below turn `up` over
    xyz = below_scene(10)
    o = stub_opts(gn, inlier_tol=0.1, min_inliers=500, below_max=1.0, ransac_iters=128)
    assert tuple(stub_run(gn, xyz, opts=o).up) == (0.0, 0.0, 1.0)
    res = stub_run(gn, xyz, opts=o, cams=[[5, 5, -3.0], [6, 5, -2.0], [5, 6, 4.0]])
    assert tuple(res.up) == (0.0, 0.0, -1.0) and (res.below, res.above) == (90, 10) and res.offset == 0.0
    assert_same_result(res, py_run(xyz, None, 0, o, [[5, 5, -3.0], [6, 5, -2.0], [5, 6, 4.0]]))
    res = stub_run(gn, xyz, opts=o, cams=[[5, 5, -3.0], [5, 6, 4.0], [1, 1, 0.0]])          # 1 : 1 and one on the plane: the points decide
    assert tuple(res.up) == (0.0, 0.0, 1.0) and (res.below, res.above) == (10, 90)
    # with below_max at its default the turned-over plane is not admissible
    assert stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=0.1, min_inliers=500, ransac_iters=128), cams=[[5, 5, -3.0]]).flags == NO_PLANE


def test_north_hint(gn):
    up = np.array([0.0, 0.6, 0.8])
    north = np.zeros(3)
    call = lambda hint: gn.gnd_north(up.ctypes.data, np.ascontiguousarray(hint, np.float64).ctypes.data, north.ctypes.data)
    assert call([0, 1, 0]) == 0 and abs(np.dot(north, up)) < 1e-15 and abs(np.linalg.norm(north) - 1) < 1e-15 and north[1] > 0
    assert north.tolist() == py_north(up.tolist(), [0, 1, 0])[0]
    assert call([0, 3, 4]) == 1 and north.tolist() == [1.0, 0.0, 0.0]          # parallel to up: the axis with the smallest |up|
    assert call([0, 0.6, 0.8 + 5e-7]) == 1 and call([0, 0.6, 0.8 + 5e-6]) == 0   # within 1e-6 / beyond it
    assert call([0, 0, 0]) == 1
    res = stub_run(gn, grid_plane().astype(np.float32), opts=stub_opts(gn, inlier_tol=0.1, north_hint=(0, 0, -2)))
    assert res.flags == NORTH_REPLACED and tuple(res.up) == (0.0, 0.0, 1.0) and tuple(res.north) == (1.0, 0.0, 0.0)


@pytest.mark.parametrize("kw", [dict(ransac_iters=0), dict(ransac_iters=4097), dict(inlier_tol=-1e-9), dict(inlier_rel=-1.0),
                                dict(inlier_tol=float("nan")), dict(inlier_rel=float("inf")), dict(below_max=-0.01), dict(below_max=1.01),
                                dict(below_max=float("nan")), dict(up_hint=(0, float("nan"), 1)), dict(up_hint=(float("inf"), 0, 0)),
                                dict(north_hint=(0, float("inf"), 0)), dict(max_tilt_deg=0.0), dict(max_tilt_deg=180.5),
                                dict(max_tilt_deg=float("nan")), dict(refit_rounds=-1), dict(refit_rounds=9), dict(min_inliers=2)])
def test_refusals(gn, kw):
    assert stub_run(gn, grid_plane().astype(np.float32), opts=stub_opts(gn, **kw)) is None


def test_few_points_and_the_limits_that_pass(gn):
    xyz = grid_plane().astype(np.float32)
    for m in (0, 1, 2):
        res = stub_run(gn, xyz[:m])
        assert res.flags == FEW and res.n_selected == m and res.winner == -1 and all(math.isnan(v) for v in (res.up[0], res.north[2], res.offset, res.rms, res.tol))
    res = stub_run(gn, xyz, labels=np.zeros(900, np.int32), label=3)
    assert res.flags == FEW and res.n_selected == 0
    assert stub_run(gn, np.full((10, 3), np.nan, np.float32)).flags == FEW
    for kw in (dict(ransac_iters=1), dict(ransac_iters=4096), dict(max_tilt_deg=180.0), dict(refit_rounds=0), dict(refit_rounds=8),
               dict(below_max=0.0), dict(below_max=1.0), dict(min_inliers=3)):
        assert stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=0.1, **kw)) is not None, kw


def accuracy_figures(run):
    """(angle to the reference normal, |offset difference| / tol) per scene; run(xyz, opts) -> GroundResult."""
    out = []
    for kw in ACCURACY_SCENES:
        scale = kw.get("scale", 1.0)
        xyz, lab, ground, R = scene(n_tree=20000, n_ground=20000, **kw)
        tol = TOL / scale
        res = run(xyz, dict(inlier_tol=tol))
        n_ref, c_ref = svd_plane(ground)
        up = np.array(res.up[:])
        if np.dot(n_ref, up) < 0:
            n_ref = -n_ref
        assert res.flags == 0 and res.inliers >= 0.99 * len(ground), (kw, res.inliers)
        out.append((math.asin(min(1.0, float(np.linalg.norm(np.cross(n_ref, up))))), abs(res.offset - float(np.dot(n_ref, c_ref))) / tol))
    return out


def test_accuracy_against_numpys_plane_fit_of_the_planted_ground(gn):
    fig = accuracy_figures(lambda xyz, kw: stub_run(gn, xyz, opts=stub_opts(gn, **kw)))
    print("angle (rad), offset (tol) per scene:", fig)
    assert max(a for a, _ in fig) <= 2 * ANGLE_WORST and max(d for _, d in fig) <= 2 * OFFSET_WORST, fig


def test_up_points_from_the_ground_to_the_tree_and_the_slope_gives_its_own_normal(gn):
    xyz, lab, ground, R = scene(58, 6000, 6000, rot=58)
    res = stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=TOL))
    assert np.dot(res.up[:], R[:, 2]) > 0.99999 and res.below <= 1 and res.above > 5000
    xyz, lab, ground, R = scene(59, 6000, 6000, slope=0.25)
    res = stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=TOL))
    assert abs(math.acos(res.up[2]) - 0.25) < 1e-3 and res.up[0] > 0           # the slope's normal, not gravity


def test_wall_scenes(gn):
    sc = wall_scenes()
    # a wall of 30 000 points across a ground disc of 20 000: the disc lies on both sides of it, so below_max rejects it
    xyz, lab, ground, R = sc["crossing"]
    res = stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=TOL))
    assert res.flags == 0 and np.dot(res.up[:], R[:, 2]) > 0.9999 and res.inliers >= 0.99 * len(ground)
    wall_only = stub_run(gn, xyz[lab == 2], opts=stub_opts(gn, inlier_tol=TOL))
    assert wall_only.inliers > 29000                                            # (it IS the plane with the most inliers)
    # the same wall at the edge: everything lies on one side of it, and it wins on inliers ...
    xyz, lab, ground, R = sc["edge"]
    res = stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=TOL))
    assert res.flags == 0 and abs(np.dot(res.up[:], R[:, 0])) > 0.9999 and res.inliers > 29000
    # ... until camera centres on its far side say which way is up: every point is then below it
    cams = np.array([[9.0, -3, 1.5], [9.0, 0, 1.6], [9.5, 3, 1.4]]) @ R.T
    res = stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=TOL), cams=cams)
    assert res.flags == 0 and np.dot(res.up[:], R[:, 2]) > 0.9999 and 0.99 * len(ground) <= res.inliers < 25000
    # ... or a hint does
    res = stub_run(gn, xyz, opts=stub_opts(gn, inlier_tol=TOL, up_hint=R[:, 2] + 0.2 * R[:, 0], max_tilt_deg=45.0))
    assert res.flags == 0 and np.dot(res.up[:], R[:, 2]) > 0.9999


def test_a_sphere_shell_has_no_plane(gn):
    res = stub_run(gn, sphere())
    assert res.flags == NO_PLANE and res.winner == -1 and res.n_selected == 4000 and res.tol > 0 and math.isnan(res.up[2])


def levelled_dendrometry(gn, dn, ground_run, seed, scale):
    """(dbh, height) of the planted tree rotated and scaled, through ground_run -> opts_from_ground -> dnd_run, and of the same
    tree upright."""
    xyz, lab, ground, R = scene(seed, 60000, 20000, rot=seed, scale=scale)
    res = ground_run(xyz, dict(inlier_tol=TOL / scale))
    assert res.flags == 0
    o = dendro_opts(dn, scale=scale)
    assert gn.gnd_opts_from_ground(C.byref(res), C.byref(o)) == 0
    assert tuple(o.up) == tuple(res.up) and tuple(o.north) == tuple(res.north) and o.ground == res.offset * scale
    lev, _, _ = dendro_run(dn, xyz, lab, 1, o)
    upright, _, _ = dendro_run(dn, planted(seed, 60000)[0])
    assert lev.flags == 0 and upright.flags == 0
    return (lev.dbh, lev.total_height), (upright.dbh, upright.total_height)


def test_end_to_end_into_the_dendrometry(gn, dn):
    worst_d = worst_h = 0.0
    for seed, scale in ((61, 1.0), (62, 0.37), (63, 2.5)):
        (dbh, h), (dbh0, h0) = levelled_dendrometry(gn, dn, lambda xyz, kw: stub_run(gn, xyz, opts=stub_opts(gn, **kw)), seed, scale)
        worst_d, worst_h = max(worst_d, abs(dbh / dbh0 - 1)), max(worst_h, abs(h - h0) / TOL)
        print("seed %d scale %g: dbh %.6f / %.6f, height %.6f / %.6f" % (seed, scale, dbh, dbh0, h, h0))
    print("worst dbh ratio - 1: %.3g, worst height difference (tol): %.3g" % (worst_d, worst_h))
    assert worst_d <= 2 * E2E_DBH_WORST and worst_h <= 2 * E2E_HEIGHT_WORST
    bad = GroundResult()
    bad.winner = -1
    assert gn.gnd_opts_from_ground(C.byref(bad), C.byref(dendro_opts(dn))) == 1
