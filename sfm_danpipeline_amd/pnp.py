"""Camera registration (reference src/Sfm.cpp:1137-1210, findCameraPosePNP) over the C ABI: cv::solvePnPRansac(...,
CV_EPNP) batched over views in one sfmhip_pnp_ransac call, the EPnP solve alone (sfmhip_pnp_epnp), and the reference's
wrapper rules around them.  The contract is the rule list in include/sfmhip.h; parity with OpenCV is unpinned."""
import numpy as np

from ._lib import check, default_context, lib
from .pose import check_coherent_rotation

MIN_POINTS = 8            # findCameraPosePNP refuses 7 or fewer correspondences (src/Sfm.cpp:1139)
MAX_TRANSLATION = 200.0   # ... and a pose whose norm(T) is above this (src/Sfm.cpp:1175)
THRESHOLD_FACTOR = 0.006  # reprojection threshold = 0.006 * the largest 2-D coordinate (src/Sfm.cpp:1151-1154)
FLAG_RANK_DEFICIENT, FLAG_SVD_RANDOM, FLAG_QR_SINGULAR = 1, 2, 4


def _pack(xyz_list, xy_list):
    n = len(xyz_list)
    if len(xy_list) != n:
        raise ValueError("one 2-D point list per 3-D point list")
    cnt = [len(a) for a in xyz_list]
    if any(len(b) != c for b, c in zip(xy_list, cnt)):
        raise ValueError("a view's 3-D and 2-D points differ in number")
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    total = int(off[-1])
    if total:
        xyz = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in xyz_list]))
        xy = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float64).reshape(-1, 2) for b in xy_list]))
    else:
        xyz, xy = np.zeros((1, 3)), np.zeros((1, 2))
    return n, off, xyz, xy


def reference_threshold(xy):
    """0.006 * maxVal of cv::minMaxIdx over every coordinate of the view's 2-D points."""
    xy = np.asarray(xy, np.float64)
    return THRESHOLD_FACTOR * float(xy.max()) if xy.size else 0.0


def rodrigues(rvec):
    """Rodrigues' formula in numpy (the wrapper's cv::Rodrigues(rvec, R); the library's own is csrc/pnp.h's)."""
    r = np.asarray(rvec, np.float64).reshape(3)
    th = float(np.linalg.norm(r))
    if th < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx


def pnp_ransac(xyz_list, xy_list, K, dist, thresholds=None, confidence=0.99, max_iters=1000, ctx=None):
    """sfmhip_pnp_ransac for a batch of views.  xyz_list[v]: n_v x 3, xy_list[v]: n_v x 2 pixels; thresholds: pixels per
    view (None: the reference's 0.006 * max coordinate).  Returns dict(status (1 pose, 0 no model, -1 fewer than five
    points), rvec, tvec (the returned pose: the RANSAC model), rvec_ransac, tvec_ransac, rvec_refit, tvec_refit (n x 3),
    inliers, iterations (n,), masks [uint8 per view], flags)."""
    ctx = ctx or default_context()
    n, off, xyz, xy = _pack(xyz_list, xy_list)
    if thresholds is None:
        thresholds = [reference_threshold(b) for b in xy_list]
    thr = np.ascontiguousarray(np.asarray(thresholds, np.float64).reshape(-1))
    if len(thr) != n:
        raise ValueError("one threshold per view")
    Kc = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    dc = np.zeros(5) if dist is None else np.ascontiguousarray(np.asarray(dist, np.float64).reshape(-1)[:5])
    if len(dc) != 5:
        raise ValueError("dist holds k1 k2 p1 p2 k3")
    m = max(n, 1)
    status, inl, its = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    vec = [np.zeros((m, 3)) for _ in range(6)]
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    if len(thr) == 0:
        thr = np.zeros(1)
    check(lib().sfmhip_pnp_ransac(ctx.h, n, off.ctypes.data, xyz.ctypes.data, xy.ctypes.data, Kc.ctypes.data, dc.ctypes.data,
                                  thr.ctypes.data, float(confidence), int(max_iters), status.ctypes.data, vec[0].ctypes.data,
                                  vec[1].ctypes.data, vec[2].ctypes.data, vec[3].ctypes.data, vec[4].ctypes.data, vec[5].ctypes.data,
                                  inl.ctypes.data, mask.ctypes.data, its.ctypes.data), "sfmhip_pnp_ransac")
    return dict(status=status[:n], rvec=vec[0][:n], tvec=vec[1][:n], rvec_ransac=vec[2][:n], tvec_ransac=vec[3][:n],
                rvec_refit=vec[4][:n], tvec_refit=vec[5][:n], inliers=inl[:n], iterations=its[:n],
                masks=[mask[off[i]:off[i + 1]].copy() for i in range(n)], flags=last_flags(ctx))


def epnp(xyz_list, xy_normalised_list, ctx=None):
    """sfmhip_pnp_epnp: the EPnP solve alone per point set (>= 5 points; 2-D points undistorted and normalised).
    Returns (R (n, 3, 3), t (n, 3), flags)."""
    ctx = ctx or default_context()
    n, off, xyz, xy = _pack(xyz_list, xy_normalised_list)
    R, t = np.zeros((max(n, 1), 9)), np.zeros((max(n, 1), 3))
    check(lib().sfmhip_pnp_epnp(ctx.h, n, off.ctypes.data, xyz.ctypes.data, xy.ctypes.data, R.ctypes.data, t.ctypes.data),
          "sfmhip_pnp_epnp")
    return R[:n].reshape(-1, 3, 3), t[:n], last_flags(ctx)


def last_flags(ctx=None):
    """sfmhip_pnp_last_flags: bit 0 a rank-deficient (planar / collinear) point set was not solved, bit 1 a 3 x 3 singular
    value <= DBL_MIN, bit 2 a singular Gauss-Newton step."""
    return int(lib().sfmhip_pnp_last_flags((ctx or default_context()).h))


def last_timing(ctx=None):
    """(solver, scoring, mask + refit) kernel milliseconds of the last pnp_ransac call on a context with timing on."""
    ms = np.zeros(3)
    check(lib().sfmhip_pnp_last_timing((ctx or default_context()).h, ms.ctypes.data), "sfmhip_pnp_last_timing")
    return tuple(float(x) for x in ms)


def accept_pose(n_points3d, n_points2d, outcome, to_matrix=None):
    """findCameraPosePNP's rules around solvePnPRansac (src/Sfm.cpp:1139-1208) on one view's outcome = (status, rvec,
    tvec): None when 7 or fewer points (or the counts differ), no pose, norm(T) > 200 or an incoherent rotation; else the
    3 x 4 pose [R|T].  to_matrix: what turns rvec into R (default: rodrigues)."""
    if n_points3d < MIN_POINTS or n_points2d < MIN_POINTS or n_points3d != n_points2d:
        return None
    status, rvec, tvec = outcome
    if status != 1:
        return None
    T = np.asarray(tvec, np.float64).reshape(3)
    if float(np.sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2])) > MAX_TRANSLATION:
        return None
    R = (to_matrix or rodrigues)(rvec)
    if not check_coherent_rotation(R):
        return None
    return np.hstack([R, T[:, None]])


def find_camera_pose_pnp(K, dist, points3d, points2d, ctx=None, solver=None):
    """findCameraPosePNP for one view: threshold 0.006 * max coordinate, 1000 iterations, confidence 0.99.  solver: what
    runs the RANSAC (default pnp_ransac; tests pass the CPU stub's twin).  Returns None or dict(P, rvec, tvec, inliers,
    mask)."""
    points3d = np.asarray(points3d, np.float64).reshape(-1, 3)
    points2d = np.asarray(points2d, np.float64).reshape(-1, 2)
    if len(points3d) < MIN_POINTS or len(points2d) < MIN_POINTS or len(points3d) != len(points2d):
        return None
    run = solver or (lambda *a, **k: pnp_ransac(*a, ctx=ctx, **k))
    r = run([points3d], [points2d], K, dist, thresholds=[reference_threshold(points2d)], confidence=0.99, max_iters=1000)
    P = accept_pose(len(points3d), len(points2d), (int(r["status"][0]), r["rvec"][0], r["tvec"][0]))
    if P is None:
        return None
    return dict(P=P, rvec=r["rvec"][0], tvec=r["tvec"][0], inliers=int(r["inliers"][0]), mask=r["masks"][0])
