"""RANSAC-EPnP camera registration (csrc/pnp.h: findCameraPosePNP's solvePnPRansac, reference src/Sfm.cpp:1137-1210) on the
CPU, through a g++ build of the header the device kernels compile (tests/stub/pnp_capi.cpp).  Nothing here asserts
against OpenCV (it is not in the image): EPnP and the RANSAC are checked against ground truth with numpy / scipy geometry
that owes nothing to the header, and the stopping rule against the oracle's RANSACUpdateNumIters."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import sfm_oracle_score as orc_score
from sfm_danpipeline_amd import pnp
from tests import pnp_scenes as S

SEEDS = range(20)
# measured worst cases over SEEDS x both distortions x n in (5, 6, 10, 100, 2000) (see test_epnp_noise_free); asserted at 10 x
EPNP_ANGLE_WORST, EPNP_TRANS_WORST = 2.44e-13, 6.95e-14
EPNP_ANGLE_BOUND, EPNP_TRANS_BOUND = 10 * EPNP_ANGLE_WORST, 10 * EPNP_TRANS_WORST
# measured largest ratio refit RMS / maximum-likelihood RMS over SEEDS x both distortions; asserted at 1.25 x
REFIT_RATIO_WORST = 1.00704
REFIT_RATIO_BOUND = 1.25 * REFIT_RATIO_WORST


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return S.build_stub(tmp_path_factory.mktemp("pnp"))


def test_restated_trigonometry_is_within_two_ulp(L):
    """sin, cos and acos of csrc/pnp.h (plain f64, so that host and device agree) against libm"""
    g = np.random.default_rng(0)
    sc = np.zeros(2)
    for x in g.uniform(0, 2 * math.pi, 20000):
        L.pnp_sincos(float(x), sc.ctypes.data)
        for got, ref in ((sc[0], math.sin(x)), (sc[1], math.cos(x))):
            assert abs(got - ref) <= 2 * math.ulp(ref) + 1e-17
    for x in list(g.uniform(-1, 1, 20000)) + [1.0, -1.0, 0.0, 0.5, -0.5, 1 - 1e-12, -1 + 1e-12]:
        assert abs(L.pnp_acos(float(x)) - math.acos(x)) <= 2 * math.ulp(math.acos(x))


def test_rodrigues_round_trip(L):
    g = np.random.default_rng(1)
    for _ in range(200):
        r = g.normal(0, 1, 3)
        r *= g.uniform(1e-3, 3.1) / np.linalg.norm(r)
        R, back = np.zeros(9), np.zeros(3)
        L.pnp_rodrigues_to_matrix(np.ascontiguousarray(r).ctypes.data, R.ctypes.data)
        assert np.allclose(R.reshape(3, 3), S.rot(r), atol=1e-14)
        assert L.pnp_rodrigues_to_vector(R.ctypes.data, back.ctypes.data) == 0
        assert np.allclose(back, r, atol=1e-9)


@pytest.mark.parametrize("dist", [S.DIST0, S.DIST1], ids=["nodist", "dist"])
@pytest.mark.parametrize("n", [5, 6, 10, 100, 2000])
def test_epnp_noise_free(L, n, dist):
    """EPnP on exact correspondences against ground truth.  Measured worst case over 20 seeds, both distortions and all n:
    rotation angle 2.44e-13 rad, relative translation error 6.95e-14 (both at n = 6, without distortion); the assertion
    is 10 x that: 2.44e-12 rad and 6.95e-13."""
    worst_a = worst_t = 0.0
    for seed in SEEDS:
        sc = S.scene(seed, n, dist)
        R, t, fl = S.stub_epnp(L, [sc["X"]], [S.normalise(sc["xy"], S.K, dist)])
        assert fl == 0
        worst_a = max(worst_a, S.rot_angle(R[0], sc["R"]))
        worst_t = max(worst_t, float(np.linalg.norm(t[0] - sc["t"]) / np.linalg.norm(sc["t"])))
    print(f"MEASURE epnp n={n} angle {worst_a:.3e} trans {worst_t:.3e}")
    assert worst_a <= EPNP_ANGLE_BOUND and worst_t <= EPNP_TRANS_BOUND


def _rms(X, xy, R, t, dist):
    return float(np.sqrt(np.mean(np.sum((S.project(X, R, t, S.K, dist) - xy) ** 2, 1))))


@pytest.mark.parametrize("dist", [S.DIST0, S.DIST1], ids=["nodist", "dist"])
def test_epnp_refit_is_near_maximum_likelihood(L, dist):
    """n = 200, Gaussian 0.5 px: the reprojection RMS of the EPnP pose against that of scipy's least_squares started from
    ground truth (the maximum-likelihood pose).  Measured largest ratio over 20 seeds and both distortions: 1.00704; the
    assertion is 1.25 x that: 1.2588."""
    from scipy.optimize import least_squares
    worst = 0.0
    for seed in SEEDS:
        sc = S.scene(seed, 200, dist, noise=0.5)
        R, t, fl = S.stub_epnp(L, [sc["X"]], [S.normalise(sc["xy"], S.K, dist)])
        assert fl == 0

        def res(p):
            return (S.project(sc["X"], S.rot(p[:3]) @ sc["R"], p[3:], S.K, dist) - sc["xy"]).ravel()
        ml = least_squares(res, np.concatenate([np.zeros(3), sc["t"]]), xtol=1e-14, ftol=1e-14, gtol=1e-14)
        rms_ml = float(np.sqrt(np.mean(np.sum(ml.fun.reshape(-1, 2) ** 2, 1))))
        worst = max(worst, _rms(sc["X"], sc["xy"], R[0], t[0], dist) / rms_ml)
    print(f"MEASURE refit ratio {worst:.5f}")
    assert worst <= REFIT_RATIO_BOUND


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("dist", [S.DIST0, S.DIST1], ids=["nodist", "dist"])
def test_ransac_masks_outliers_and_stops_by_the_rule(L, dist):
    """30 % outliers displaced by >= 20 thresholds, 0.5 px inlier noise, the reference's threshold, 20 scenes"""
    for seed in SEEDS:
        n = 300
        sc = S.ransac_scene(seed, n, dist)
        thr = sc["thr"]
        clean = S.project(sc["X"], sc["R"], sc["t"], S.K, dist)
        assert np.all(np.linalg.norm(sc["xy"] - clean, axis=1)[sc["truth"] == 0] >= 20 * thr)
        r = S.stub_ransac(L, [sc["X"]], [sc["xy"]], S.K, dist)
        assert r["status"][0] == 1 and r["flags"] & ~pnp.FLAG_RANK_DEFICIENT == 0
        mask = r["masks"][0]
        assert not np.any(mask[sc["truth"] == 0]), "a true outlier is in the mask"
        assert int(r["inliers"][0]) == int(mask.sum())
        # the mask against an f64 numpy recomputation for the returned RANSAC model (the float points, as the rule says)
        Rm = S.rot(r["rvec_ransac"][0])
        err = np.linalg.norm(S.project(_f32(sc["X"]), Rm, r["tvec_ransac"][0], S.K, dist) - _f32(sc["xy"]), axis=1)
        near = np.abs(err - thr) <= 1e-3 * thr
        assert near.sum() <= 0.01 * n
        assert np.array_equal(mask[~near] != 0, (err <= thr)[~near])
        # the stopping rule, replayed: per-iteration counts from the stub's sample solver, the limit from the oracle
        its = int(r["iterations"][0])
        assert 0 < its <= 1000
        samp = np.zeros(5 * its, np.int32)
        L.pnp_samples(n, its, samp.ctypes.data)
        fx, fy = sc["X"].astype(np.float32), sc["xy"].astype(np.float32)
        Kc, dc = np.ascontiguousarray(S.K.reshape(9)), np.ascontiguousarray(dist)
        best, niters, best_model = 0, 1000, None
        for it in range(its):
            assert it < niters, "the loop ran past its own limit"
            s = samp[5 * it:5 * it + 5]
            a, b = np.ascontiguousarray(fx[s]), np.ascontiguousarray(fy[s])
            model = np.zeros(6)
            ok = L.pnp_sample(a.ctypes.data, b.ctypes.data, Kc.ctypes.data, dc.ctypes.data, model.ctypes.data)
            if ok & 0xff == 0:
                continue
            cnt = L.pnp_count(n, fx.ctypes.data, fy.ctypes.data, Kc.ctypes.data, dc.ctypes.data, model.ctypes.data, thr, None)
            if cnt > max(best, 4):
                best, best_model = cnt, model.copy()
                niters = orc_score.ransac_update_num_iters(0.99, (n - cnt) / n, 5, niters)
        assert its == niters and best == int(r["inliers"][0])
        assert np.array_equal(best_model[:3], r["rvec_ransac"][0]) and np.array_equal(best_model[3:], r["tvec_ransac"][0])
        # the returned pose is the RANSAC model; both it and the refit are close to ground truth
        assert np.array_equal(r["rvec"][0], r["rvec_ransac"][0]) and np.array_equal(r["tvec"][0], r["tvec_ransac"][0])
        assert S.rot_angle(S.rot(r["rvec_refit"][0]), sc["R"]) < 5e-3
        assert np.linalg.norm(r["tvec_refit"][0] - sc["t"]) / np.linalg.norm(sc["t"]) < 5e-3


def _bits(r, v):
    return [r[k][v].tobytes() for k in ("rvec", "tvec", "rvec_ransac", "tvec_ransac", "rvec_refit", "tvec_refit")] + \
           [int(r["status"][v]), int(r["inliers"][v]), int(r["iterations"][v]), r["masks"][v].tobytes()]


def test_batch_independence(L):
    """view v's outputs are bit-equal whether it runs alone or inside a batch of 7"""
    scs = [S.ransac_scene(100 + v, 40 + 37 * v, S.DIST1 if v % 2 else S.DIST0) for v in range(7)]
    # (one K and dist per call: take DIST1 for all, the scenes made without distortion are then simply other data)
    X, xy = [s["X"] for s in scs], [s["xy"] for s in scs]
    thr = [s["thr"] for s in scs]
    batch = S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr)
    for v in range(7):
        alone = S.stub_ransac(L, [X[v]], [xy[v]], S.K, S.DIST1, thresholds=[thr[v]])
        assert _bits(alone, 0) == _bits(batch, v), v


def test_edges(L):
    sc = S.scene(3, 50)
    # fewer than five correspondences (four included: P3P is not built)
    r = S.stub_ransac(L, [sc["X"][:4], sc["X"][:0], sc["X"][:5]], [sc["xy"][:4], sc["xy"][:0], sc["xy"][:5]], S.K, S.DIST0,
                      thresholds=[3.0, 3.0, 3.0])
    assert list(r["status"]) == [-1, -1, 1] and list(r["inliers"]) == [0, 0, 5] and r["masks"][2].tolist() == [1] * 5
    assert not np.any(r["rvec"][:2]) and not np.any(r["tvec"][:2])
    # all-outlier data: no pose, or a pose with fewer than 8 inliers; never a crash
    g = np.random.default_rng(5)
    junk = g.uniform(0, 600, (200, 2))
    r = S.stub_ransac(L, [g.uniform(-1, 1, (200, 3))], [junk], S.K, S.DIST0, thresholds=[0.5])
    assert r["status"][0] == 0 or r["inliers"][0] < 8
    assert r["iterations"][0] <= 1000
    # a coplanar point set sets the flag and is not solved
    P = sc["X"][:12].copy()
    P[:, 2] = 0.25
    R, t, fl = S.stub_epnp(L, [P], [S.normalise(S.project(P, sc["R"], sc["t"], S.K, S.DIST0), S.K, S.DIST0)])
    assert fl & pnp.FLAG_RANK_DEFICIENT and not np.any(R) and not np.any(t)
    # ... and a RANSAC over coplanar points skips every hypothesis: no model, the flag
    xyP = S.project(P, sc["R"], sc["t"], S.K, S.DIST0)
    r = S.stub_ransac(L, [P], [xyP], S.K, S.DIST0, thresholds=[3.0], max_iters=50)
    assert r["status"][0] == 0 and r["inliers"][0] == 0 and r["flags"] & pnp.FLAG_RANK_DEFICIENT


def test_find_camera_pose_pnp_wrapper_rules(L):
    """the reference's rules around solvePnPRansac (src/Sfm.cpp:1139-1208), on the stub's outputs"""
    def solver(*a, **k):
        return S.stub_ransac(L, *a, **k)
    sc = S.ransac_scene(7, 120)
    got = pnp.find_camera_pose_pnp(S.K, S.DIST0, sc["X"], sc["xy"], solver=solver)
    assert got is not None and got["P"].shape == (3, 4)
    assert S.rot_angle(got["P"][:, :3], sc["R"]) < 5e-3 and np.allclose(got["P"][:, 3], sc["t"], rtol=5e-3, atol=5e-3)
    # 7 or fewer points, or lists of different length
    assert pnp.find_camera_pose_pnp(S.K, S.DIST0, sc["X"][:7], sc["xy"][:7], solver=solver) is None
    assert pnp.find_camera_pose_pnp(S.K, S.DIST0, sc["X"][:9], sc["xy"][:8], solver=solver) is None
    # the same scene 300 units away: norm(T) > 200
    far = dict(sc)
    far_t = sc["t"] + np.array([0, 0, 300.0])
    far_xy = S.project(sc["X"] * 40, sc["R"], far_t, S.K, S.DIST0)
    got = pnp.find_camera_pose_pnp(S.K, S.DIST0, sc["X"] * 40, far_xy, solver=solver)
    assert got is None
    r = solver([sc["X"] * 40], [far_xy], S.K, S.DIST0)
    assert r["status"][0] == 1 and np.linalg.norm(r["tvec"][0]) > 200      # (refused by the rule, not for want of a pose)
    # an incoherent rotation, no pose, too large a translation: accept_pose alone
    assert pnp.accept_pose(10, 10, (1, np.zeros(3), np.array([0, 0, 5.0]))) is not None
    assert pnp.accept_pose(10, 10, (0, np.zeros(3), np.array([0, 0, 5.0]))) is None
    assert pnp.accept_pose(10, 10, (1, np.zeros(3), np.array([0, 0, 200.5]))) is None
    assert pnp.accept_pose(10, 10, (1, np.zeros(3), np.array([0, 0, 200.0]))) is not None
    # the coherent-rotation rule inside accept_pose: the same outcome passes with a rotation and is refused when what
    # Rodrigues hands back has |det| - 1 > 1e-7
    ok = (1, np.array([0.1, -0.2, 0.3]), np.array([0, 0, 5.0]))
    assert pnp.accept_pose(10, 10, ok) is not None
    assert pnp.accept_pose(10, 10, ok, to_matrix=lambda r: 1.001 * pnp.rodrigues(r)) is None
    # (the reference's test is one-sided, fabsf(det) - 1 > 1e-7: a |det| below 1 passes, src/Sfm.cpp:793)
    assert pnp.accept_pose(10, 10, ok, to_matrix=lambda r: np.diag([1.0, 1.0, 0.5]) @ pnp.rodrigues(r)) is not None
    assert pnp.accept_pose(10, 10, ok, to_matrix=lambda r: (1 + 1e-9) * pnp.rodrigues(r)) is not None
    assert pnp.reference_threshold(sc["xy"]) == 0.006 * sc["xy"].max()
