"""The cloud registration (csrc/register.h, DESIGN.md f-17: nearest points, rigid and similarity ICP) on the CPU, through a g++
build of the header the device code compiles (tests/stub/register_capi.cpp): the search against brute-force float32 numpy
under the (d2, index) rule, the estimate against numpy's SVD solution, the loop against a plain numpy + cKDTree transcription
of rules 2-6 written from the DESIGN text, a partial overlap under max_dist, the loop's edges and rule 1's refusals.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from sfm_danpipeline_amd.register import DEGENERATE, FEW, RegisterOpts, RegisterResult, Transform, set_opts
from tests.test_dendro_cpu import rotation
from tests.test_trees_cpu import plot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "register_capi.cpp")
INF32 = np.float32(np.inf)
# the worst figures of the stub's estimate against numpy's SVD solution over estimate_scenes() (DESIGN.md f-17 records them): the
# largest entry of R - R_numpy, |scale / scale_numpy - 1| and the largest entry of t - t_numpy; the test asserts at ten times them
EST_R_WORST = 5.6e-16
EST_SCALE_WORST = 6.7e-16
EST_T_WORST = 2.7e-15
# scene 3's bounds: ten times what a numpy + cKDTree ICP of these rules measured on the planted plot
RMSE_MAX, SCALE_ERR_MAX, ANGLE_ERR_MAX_DEG, T_ERR_MAX = 1.3e-6, 1e-8, 2e-5, 5e-8
CENTRES = [(-4, -2), (3, -3), (1, 4.5)]
AXIS = np.array([0.3, -0.2, 0.93])
MOTIONS = [(2.0, 0.1), (4.0, 0.3), (8.0, 0.5)]


@pytest.fixture(scope="module")
def rg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("register") / "libregistercapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.reg_default_opts.argtypes = [vp]
    lib.reg_default_opts.restype = None
    lib.reg_sizes.argtypes = [vp, vp, vp]
    lib.reg_nearest.argtypes = [ci, vp, ci, vp, vp, C.c_double, vp, vp]
    lib.reg_run.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp]
    lib.reg_estimate.argtypes = [ci, vp, vp, ci, vp, vp]
    lib.reg_transform.argtypes = [ci, vp, vp, vp]
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_register.py)
def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def stub_opts(rg, **kw):
    o = RegisterOpts()
    rg.reg_default_opts(C.byref(o))
    return set_opts(o, **kw)


def result_bytes(r):
    return bytes(memoryview(r))


def stub_nearest(rg, tgt, src, T=None, max_dist=math.inf):
    """(idx, d2); None when refused."""
    tgt, src = f32(tgt), f32(src)
    idx, d2 = np.empty(max(len(src), 1), np.int32), np.empty(max(len(src), 1), np.float32)
    rc = rg.reg_nearest(len(tgt), tgt.ctypes.data, len(src), src.ctypes.data, None if T is None else C.byref(T), float(max_dist),
                        idx.ctypes.data, d2.ctypes.data)
    return None if rc else (idx[:len(src)], d2[:len(src)])


def stub_run(rg, tgt, src, init=None, opts=None, **kw):
    """(RegisterResult, idx); None when refused."""
    tgt, src = f32(tgt), f32(src)
    o = set_opts(opts, **kw) if opts is not None else stub_opts(rg, **kw)
    res, idx = RegisterResult(), np.empty(max(len(src), 1), np.int32)
    rc = rg.reg_run(len(tgt), tgt.ctypes.data, len(src), src.ctypes.data, C.byref(o), None if init is None else C.byref(init),
                    C.byref(res), idx.ctypes.data)
    return None if rc else (res, idx[:len(src)])


def stub_estimate(rg, p, m, with_scale, cur=None):
    p, m = f32(p), f32(m)
    cur, nxt = cur or Transform.make(), Transform.make()
    flags = rg.reg_estimate(len(p), p.ctypes.data, m.ctypes.data, int(with_scale), C.byref(cur), C.byref(nxt))
    return flags, nxt


# ---------------------------------------------------------------- scenes (shared with tests/test_gpu_register.py)
def axis_rotation(deg, axis=AXIS):
    a, th = axis / np.linalg.norm(axis), np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def motion(deg, tr, scale=1.0):
    return Transform.make(axis_rotation(deg), tr * np.array([1.0, -0.7, 0.5]), scale)


def moved_back(xyz, M):
    """The points whose image under M is xyz: float32 of R^T (y - t) / scale."""
    y = np.asarray(xyz, np.float64)
    return (((y - M.translation()) / M.scale) @ M.rotation()).astype(np.float32)


def nearest_scene():
    """Scene 1: 500 target points with 20 duplicated and 5 NaN rows, one planted apart; 300 source points with NaN rows and
    points beyond every face, edge and corner of the target's box at 0.1 and 10 box lengths."""
    rng = np.random.default_rng(11)
    tgt = (rng.uniform(0, 1, (500, 3)) * [2.0, 1.5, 0.7] + [1.0, -2.0, 0.3]).astype(np.float32)
    tgt[480:500] = tgt[rng.choice(400, 20, replace=False)]
    tgt[[13, 101, 202, 303, 404], [0, 1, 2, 0, 1]] = np.nan
    tgt[450] = (2.0, -1.0, 1.5)                                   # apart from the rest (z <= 1.0): the kept-at-the-bound point's pair
    lo, hi = np.nanmin(tgt[np.isfinite(tgt).all(1)], 0), np.nanmax(tgt[np.isfinite(tgt).all(1)], 0)
    src = (rng.uniform(-0.2, 1.2, (300, 3)) * (hi - lo) + lo).astype(np.float32)
    k = 0
    for far in (0.1, 10.0):
        for d in np.ndindex(3, 3, 3):
            d = np.array(d) - 1
            if not d.any():
                continue
            inside = lo + rng.uniform(0, 1, 3) * (hi - lo)
            src[100 + k] = np.where(d < 0, lo - far * (hi - lo), np.where(d > 0, hi + far * (hi - lo), inside))
            k += 1
    src[[7, 8, 9], [0, 1, 2]] = np.nan
    src[10, 0] = np.inf
    src[200] = (2.0, -1.0, 1.75)                                  # exactly 0.25 above tgt[450]: d2 = 0.0625
    return tgt, src


def brute_nearest(tgt, q):
    """(idx, d2) of float32 q against the finite rows of tgt, the family's float d2, least (d2, index); a non-finite q: -1, inf."""
    idx, d2 = np.full(len(q), -1, np.int32), np.full(len(q), INF32, np.float32)
    ok = np.isfinite(tgt).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(q)):
            if not np.isfinite(q[i]).all() or not ok.any():
                continue
            d = tgt - q[i]
            dd = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            dd[~ok] = INF32
            j = int(np.argmin(dd))                                # (the first of equal minima: the lower index)
            idx[i], d2[i] = j, dd[j]
    return idx, d2


def least_max_dist(d2):
    """The least double max_dist with (float)(max_dist * max_dist) == d2."""
    d2 = np.float32(d2)
    md = math.sqrt(0.5 * (float(d2) + float(np.nextafter(d2, np.float32(0)))))
    while np.float32(md * md) < d2:
        md = math.nextafter(md, math.inf)
    while np.float32(math.nextafter(md, 0.0) ** 2) == d2:
        md = math.nextafter(md, 0.0)
    assert np.float32(md * md) == d2 and np.float32(math.nextafter(md, 0.0) ** 2) < d2
    return md


_PLOT = {}


def planted_plot():
    """Scene 3's target (8 500 points), computed once."""
    if "t" not in _PLOT:
        _PLOT["t"] = plot(1, CENTRES, n_tree=1500, n_ground=4000)[0]
        _PLOT["t"].setflags(write=False)
    return _PLOT["t"]


def icp_scene(deg, tr, scale):
    """(target, source, the motion that brings the source back): every third target point moved by the motion's inverse."""
    tgt = planted_plot()
    M = motion(deg, tr, scale)
    return tgt, moved_back(tgt[::3], M), M


def partial_scene(deg, tr, scale):
    """Scene 4: the source of scene 3 where the target's x < 1, then 400 strangers above every crown."""
    tgt, src, M = icp_scene(deg, tr, scale)
    own = src[tgt[::3, 0] < 1]
    strangers = np.random.default_rng(5).uniform([-8, -8, 12], [0, 8, 14], (400, 3)).astype(np.float32)
    return tgt, np.concatenate([own, strangers]), M, len(own)


def motion_errors(T, M):
    """(|scale / planted - 1|, the angle between the rotations in degrees, the largest translation entry's error)."""
    dR = T.rotation() @ M.rotation().T
    ang = math.degrees(math.atan2(np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2, (np.trace(dR) - 1) / 2))
    return abs(T.scale / M.scale - 1), ang, float(np.abs(T.translation() - M.translation()).max())


# ---------------------------------------------------------------- the transcription of rules 2-6 (numpy + cKDTree)
def np_estimate(p, m, with_scale, cur_scale):
    """Rule 5 by numpy's SVD on f64 sums: (R, t, scale, degenerate)."""
    p, m = p.astype(np.float64), m.astype(np.float64)
    mu_p, mu_m = p.mean(0), m.mean(0)
    dp, dm = p - mu_p, m - mu_m
    H, sigma = dm.T @ dp, float((dp * dp).sum())
    U, W, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = (W[0] + W[1] + d * W[2]) / sigma if with_scale else cur_scale
    deg = sigma == 0 or W[1] <= 1e-12 * W[0] or not (np.isfinite(scale) and scale > 0)
    return R, mu_m - scale * (R @ mu_p), scale, deg


def np_icp(tgt, src, init=None, max_iters=50, with_scale=0, min_pairs=3, max_dist=math.inf, eps=0.0):
    """Rule 6: dict(T, iterations, pairs, converged, flags, mse, idx)."""
    T = init or Transform.make()
    ok_t = np.isfinite(tgt).all(1)
    rows = np.flatnonzero(ok_t)
    tree = cKDTree(tgt[rows].astype(np.float64)) if len(rows) else None
    md2 = np.float32(max_dist * max_dist)
    prev_idx, prev_T, k = None, None, 0
    while True:
        q = T.apply(src)
        idx, d2 = np.full(len(src), -1, np.int32), np.full(len(src), INF32, np.float32)
        ok = np.isfinite(src).all(1) & np.isfinite(q).all(1)
        if tree is not None and ok.any():
            j = rows[tree.query(q[ok].astype(np.float64))[1]]
            d = q[ok] - tgt[j]
            dd = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            idx[ok], d2[ok] = np.where(dd <= md2, j, -1), dd
        pr = idx >= 0
        out = dict(T=T, iterations=k, pairs=int(pr.sum()), converged=0, flags=0, idx=idx,
                   mse=float(d2[pr].astype(np.float64).mean()) if pr.any() else math.nan)
        if out["pairs"] < min_pairs:
            out["flags"] = FEW
            return out
        if k > 0 and np.array_equal(idx, prev_idx):
            out["converged"] = 1
            return out
        if k > 0 and eps > 0 and np.abs(T.matrix()[:3] - prev_T.matrix()[:3]).max() <= eps:
            out["converged"] = 2
            return out
        if k == max_iters:
            return out
        R, t, scale, deg = np_estimate(src[pr], tgt[idx[pr]], with_scale, T.scale)
        if deg:
            out["flags"] = DEGENERATE
            return out
        prev_idx, prev_T, T, k = idx, T, Transform.make(R, t, scale), k + 1


# ---------------------------------------------------------------- 1. nearest
def test_struct_sizes_agree(rg):
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    rg.reg_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(Transform), C.sizeof(RegisterOpts), C.sizeof(RegisterResult)) == (104, 32, 128)


@pytest.mark.parametrize("max_dist", [math.inf, 0.3])
@pytest.mark.parametrize("moved", [False, True])
def test_nearest_equals_brute_force(rg, max_dist, moved):
    tgt, src = nearest_scene()
    T = motion(5.0, 0.2, 1.1) if moved else None
    idx, d2 = stub_nearest(rg, tgt, src, T, max_dist)
    q = T.apply(src) if moved else src
    q = np.where(np.isfinite(src).all(1)[:, None], q, np.float32(np.nan))
    bi, bd = brute_nearest(tgt, q)
    bi = np.where(bd <= np.float32(max_dist * max_dist), bi, -1)
    assert np.array_equal(d2.view(np.uint32), bd.view(np.uint32)) and np.array_equal(idx, bi)
    assert (idx[7:11] == -1).all() and np.isinf(d2[7:11]).all()
    if not moved:                                                 # the duplicates resolve to the lower index
        assert (idx >= 0).sum() > 100 and not np.isin(idx, np.arange(480, 500)).any()


def test_nearest_keeps_a_pair_at_the_bound(rg):
    tgt, src = nearest_scene()
    idx, d2 = stub_nearest(rg, tgt, src)
    assert idx[200] == 450 and d2[200] == np.float32(0.0625)
    md = least_max_dist(d2[200])
    assert stub_nearest(rg, tgt, src, None, md)[0][200] == 450
    idx2, d22 = stub_nearest(rg, tgt, src, None, math.nextafter(md, 0.0))
    assert idx2[200] == -1 and d22[200] == d2[200]                # rejected, and the distance stays
    i = int(np.flatnonzero(idx >= 0)[17])                         # and a bound nobody planted
    md = least_max_dist(d2[i])
    assert stub_nearest(rg, tgt, src, None, md)[0][i] == idx[i] and stub_nearest(rg, tgt, src, None, math.nextafter(md, 0.0))[0][i] == -1


# ---------------------------------------------------------------- 2. the estimate on exact pairs
def estimate_scenes():
    """(name, p, m, with_scale): a planted similarity, a rigid one, a near-planar set whose noise asks for the reflection fix."""
    rng = np.random.default_rng(21)
    out = []
    p = rng.normal(size=(700, 3)) * [3.0, 2.0, 1.0] + [5.0, -3.0, 2.0]
    for name, s, ws in (("similarity", 1.37, 1), ("shrink", 0.6, 1), ("rigid", 1.0, 0)):
        R, t = rotation(5 + len(out)), rng.normal(size=3) * 4
        out.append((name, p.astype(np.float32), (s * p.astype(np.float32).astype(np.float64) @ R.T + t).astype(np.float32), ws))
    flat = rng.normal(size=(300, 3)) * [3.0, 2.0, 1e-4] + [-2.0, 4.0, 1.0]  # thinner than the noise: the third direction is the noise's
    R = rotation(9)
    for seed in range(40):                                        # the first noise whose H has det(U) det(Vt) < 0
        m = (flat @ R.T + np.random.default_rng(100 + seed).normal(size=flat.shape) * 5e-3).astype(np.float32)
        pf = flat.astype(np.float32)
        dp, dm = pf.astype(np.float64) - pf.astype(np.float64).mean(0), m.astype(np.float64) - m.astype(np.float64).mean(0)
        U, _, Vt = np.linalg.svd(dm.T @ dp)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0:
            out.append(("planar-reflected", pf, m, 1))
            break
    assert out[-1][0] == "planar-reflected"
    return out


def test_estimate_recovers_planted_motion_and_equals_numpy(rg):
    worst = np.zeros(3)
    for name, p, m, ws in estimate_scenes():
        flags, T = stub_estimate(rg, p, m, ws)
        R, t, scale, deg = np_estimate(p, m, ws, 1.0)
        assert flags == 0 and not deg, name
        assert abs(np.linalg.det(T.rotation()) - 1) < 1e-12 and np.abs(T.rotation() @ T.rotation().T - np.eye(3)).max() < 1e-12, name
        dev = np.array([np.abs(T.rotation() - R).max(), abs(T.scale / scale - 1), np.abs(T.translation() - t).max()])
        print(f"estimate {name}: R {dev[0]:.2e} scale {dev[1]:.2e} t {dev[2]:.2e}")
        worst = np.maximum(worst, dev)
        if name != "planar-reflected":                            # the planted motion itself, to float32's rounding of m
            res = np.abs(T.apply(p).astype(np.float64) - m).max()
            assert res < 4e-6 * (1 + np.abs(m).max()), (name, res)
    assert worst[0] <= 10 * EST_R_WORST and worst[1] <= 10 * EST_SCALE_WORST and worst[2] <= 10 * EST_T_WORST, worst


def test_estimate_degenerate_cases(rg):
    two = np.array([[0, 0, 0], [1, 2, 3]], np.float32)
    same = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (50, 1))
    line = np.outer(np.arange(40, dtype=np.float32), np.array([1.0, 2.0, -1.0], np.float32))
    for ws in (0, 1):
        assert stub_estimate(rg, two, two, ws)[0] == DEGENERATE
        assert stub_estimate(rg, same, same, ws)[0] == DEGENERATE
        assert stub_estimate(rg, line, line * np.float32(2), ws)[0] == DEGENERATE
    assert stub_estimate(rg, two[:0], two[:0], 1)[0] == FEW


# ---------------------------------------------------------------- 3. ICP on the planted plot
@pytest.mark.parametrize("max_dist", [1.0, math.inf])
@pytest.mark.parametrize("scale", [None, 1.04, 0.95])
@pytest.mark.parametrize("deg,tr", MOTIONS)
def test_icp_on_the_planted_plot(rg, deg, tr, scale, max_dist):
    tgt, src, M = icp_scene(deg, tr, scale or 1.0)
    assert len(tgt) == 8500 and len(src) == 2834
    kw = dict(with_scale=int(scale is not None), max_dist=max_dist)
    res, idx = stub_run(rg, tgt, src, **kw)
    ref = np_icp(tgt, src, **kw)
    es, ea, et = motion_errors(res.T, M)
    print(f"icp {deg} {tr} {scale} {max_dist}: it {res.iterations} (numpy {ref['iterations']}) pairs {res.pairs} conv {res.converged} "
          f"rmse {math.sqrt(res.mse):.3g} scale {es:.3g} angle {ea:.3g} t {et:.3g}")
    assert res.converged == 1 and res.flags == 0 and res.iterations <= 30 and res.pairs == len(src)
    assert math.sqrt(res.mse) <= RMSE_MAX and es <= SCALE_ERR_MAX and ea <= ANGLE_ERR_MAX_DEG and et <= T_ERR_MAX
    assert np.array_equal(idx, np.arange(0, len(tgt), 3))
    assert res.iterations == ref["iterations"] and np.array_equal(idx, ref["idx"])


# ---------------------------------------------------------------- 4. partial overlap
@pytest.mark.parametrize("max_dist", [0.5, 1.0])
@pytest.mark.parametrize("scale", [None, 1.04])
def test_icp_partial_overlap(rg, scale, max_dist):
    tgt, src, M, n_own = partial_scene(4.0, 0.3, scale or 1.0)
    assert n_own == 1541 and len(src) == 1941
    kw = dict(with_scale=int(scale is not None), max_dist=max_dist)
    res, idx = stub_run(rg, tgt, src, **kw)
    ref = np_icp(tgt, src, **kw)
    es, ea, et = motion_errors(res.T, M)
    print(f"partial {scale} {max_dist}: it {res.iterations} (numpy {ref['iterations']}) pairs {res.pairs} rmse {math.sqrt(res.mse):.3g} "
          f"scale {es:.3g} angle {ea:.3g} t {et:.3g}")
    assert res.converged == 1 and res.flags == 0 and res.pairs == 1541 and 12 <= res.iterations <= 13
    assert (idx[:n_own] >= 0).all() and (idx[n_own:] == -1).all()
    assert math.sqrt(res.mse) <= RMSE_MAX and es <= SCALE_ERR_MAX and ea <= ANGLE_ERR_MAX_DEG and et <= T_ERR_MAX
    assert res.iterations == ref["iterations"] and np.array_equal(idx, ref["idx"])


# ---------------------------------------------------------------- 5. the loop's edges
def test_loop_edges(rg):
    tgt, src, M = icp_scene(4.0, 0.3, 1.0)
    full, _ = stub_run(rg, tgt, src)
    r0, i0 = stub_run(rg, tgt, src, max_iters=0)                  # evaluation only
    assert (r0.iterations, r0.converged, r0.flags, r0.pairs) == (0, 0, 0, len(src))
    assert result_bytes(r0.T) == result_bytes(Transform.make()) and np.array_equal(i0, stub_nearest(rg, tgt, src)[0])
    assert r0.mse == pytest.approx(float(stub_nearest(rg, tgt, src)[1].astype(np.float64).mean()), rel=1e-12)
    r1, _ = stub_run(rg, tgt, src, max_iters=1)
    assert (r1.iterations, r1.converged) == (1, 0) and r1.mse < r0.mse
    rl, _ = stub_run(rg, tgt, src, max_iters=full.iterations - 2)  # a limit hit
    assert (rl.iterations, rl.converged, rl.flags) == (full.iterations - 2, 0, 0)
    re_, _ = stub_run(rg, tgt, src, eps=1e-2)                      # eps stops before the fixed point
    assert re_.converged == 2 and 1 < re_.iterations < full.iterations
    ref = np_icp(tgt, src, eps=1e-2)
    assert (ref["converged"], ref["iterations"]) == (2, re_.iterations)
    away = tgt + np.float32(20)                                    # source == target, no coordinate near zero: T_1 is the identity
    rs, isame = stub_run(rg, away, away)                           # to 1e-16 and every q rounds to its own float again
    assert (rs.iterations, rs.converged, rs.flags, rs.pairs, rs.mse) == (1, 1, 0, len(tgt), 0.0)
    k0, _ = stub_nearest(rg, away, away)
    assert np.array_equal(isame, k0) and (isame <= np.arange(len(tgt))).all()
    rz, _ = stub_run(rg, tgt, tgt)                                 # with a coordinate that is exactly 0, t's 1e-16 shows there
    assert (rz.iterations, rz.converged, rz.pairs) == (1, 1, len(tgt)) and rz.mse < 1e-30
    ri, _ = stub_run(rg, tgt, src, init=M)                         # from the planted motion: the pairs are there at once
    assert ri.converged == 1 and ri.iterations <= 3


def test_no_pairs_is_few_not_an_error(rg):
    tgt, src, _ = icp_scene(2.0, 0.1, 1.0)
    nan = np.full((4, 3), np.nan, np.float32)
    for t, s, kw in ((tgt, src[:0], {}), (tgt[:0], src, {}), (nan, src, {}), (tgt, nan, {}), (tgt, src + np.float32(100), dict(max_dist=0.5)),
                     (tgt, src[:2], {}), (tgt, src, dict(max_iters=0, max_dist=1e-6))):
        res, idx = stub_run(rg, t, s, **kw)
        assert res.flags == FEW and res.converged == 0 and res.iterations == 0 and res.pairs < 3
        assert (res.pairs == 0) == math.isnan(res.mse) and (idx >= 0).sum() == res.pairs
        assert result_bytes(res.T) == result_bytes(Transform.make())


def test_degenerate_pairs_stop_the_loop(rg):
    line = np.outer(np.arange(40, dtype=np.float32), np.array([1.0, 2.0, -1.0], np.float32))
    res, _ = stub_run(rg, line, line + np.float32(0.01))
    assert res.flags == DEGENERATE and res.iterations == 0 and res.pairs == 40


def test_refusals(rg):
    tgt, src, _ = icp_scene(2.0, 0.1, 1.0)
    tgt, src = tgt[:200], src[:50]
    assert stub_run(rg, tgt, src) is not None
    for kw in (dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=math.nan), dict(eps=-1e-12), dict(eps=math.nan), dict(max_iters=-1),
               dict(min_pairs=2)):
        assert stub_run(rg, tgt, src, **kw) is None, kw
    for bad in (Transform.make(scale=0.0), Transform.make(scale=-1.0), Transform.make(scale=math.nan), Transform.make(scale=math.inf),
                Transform.make(t=[0, math.inf, 0]), Transform.make(R=np.diag([1.0, math.nan, 1.0]))):
        assert stub_run(rg, tgt, src, init=bad) is None and stub_nearest(rg, tgt, src, bad) is None
    for md in (0.0, -2.0, math.nan):
        assert stub_nearest(rg, tgt, src, None, md) is None


def test_transform_rule_8(rg):
    tgt, src = nearest_scene()
    M = motion(30.0, 2.0, 1.3)
    out = np.empty_like(src)
    assert rg.reg_transform(len(src), src.ctypes.data, C.byref(M), out.ctypes.data) == 0
    want = M.apply(src)
    bad = ~np.isfinite(src).all(1)
    want[bad] = src[bad]                                          # a non-finite point stays as it is
    assert bad.sum() == 4 and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert rg.reg_transform(len(src), src.ctypes.data, C.byref(Transform.make(scale=0.0)), out.ctypes.data) == 1


def test_transform_helpers():
    A, B = motion(30.0, 2.0, 1.3), Transform.make(rotation(4), [1, 2, 3], 0.7)
    x = np.random.default_rng(0).normal(size=(50, 3))
    h = np.c_[x, np.ones(50)]
    assert np.allclose((A.compose(B).matrix() @ h.T).T, (A.matrix() @ B.matrix() @ h.T).T, atol=1e-12)
    assert np.allclose(A.inverse().matrix() @ A.matrix(), np.eye(4), atol=1e-12)
    assert np.allclose(Transform.from_matrix(A.matrix()).matrix(), A.matrix(), atol=1e-12)
    assert np.allclose(A.apply(x), (A.matrix() @ h.T).T[:, :3], atol=1e-5)
