"""The pose step of baseReconstruction (reference src/Sfm.cpp:408-492, 713-799) over the C ABI: getCameraPose =
findEssentialMat(RANSAC, 0.999, 1.0) -> recoverPose(E, ..., fx, (cx, cy), mask) -> CheckCoherentRotation, batched over
pairs in one sfmhip_essential_pose call (E and the RANSAC mask stay on the device).  Mirrors csrc/host/SfmPose.cpp."""
import numpy as np

from ._lib import check, default_context, lib
from . import triangulate as _tri

MIN_ALIGNED = 8          # getCameraPose refuses 7 or fewer aligned points (src/Sfm.cpp:734)
DISTANCE_THRESH = 50.0   # recoverPose's focal / principal-point overload


def _cat(pairs_points, k):
    n = len(pairs_points)
    total = sum(len(p[0]) for p in pairs_points)
    if not n or not total:
        return np.zeros((1, 2))
    return np.ascontiguousarray(np.concatenate([np.asarray(p[k], np.float64).reshape(-1, 2) for p in pairs_points]))


def _offsets(pairs_points):
    return np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs_points])]).astype(np.int32)


def recover_pose(pairs_points, E, focal, pp, masks=None, distance_thresh=DISTANCE_THRESH, ctx=None):
    """sfmhip_recover_pose: cv::recoverPose(E, p1, p2, R, t, focal, pp, mask) per pair.  pairs_points: [(left n x 2,
    right n x 2)] pixels; E: (n_pairs, 3, 3); masks: None or one uint8 array per pair.  Returns (R (n, 3, 3), t (n, 3),
    n_good (n,), output masks [uint8 per pair])."""
    ctx = ctx or default_context()
    n = len(pairs_points)
    off = _offsets(pairs_points)
    left, right = _cat(pairs_points, 0), _cat(pairs_points, 1)
    Ec = np.ascontiguousarray(np.asarray(E, np.float64).reshape(-1, 9)) if n else np.zeros((1, 9))
    total = int(off[-1])
    m_in = np.ascontiguousarray(np.concatenate([np.asarray(m, np.uint8).reshape(-1) for m in masks])) if masks is not None and total else None
    R, t = np.zeros((max(n, 1), 9)), np.zeros((max(n, 1), 3))
    ng = np.zeros(max(n, 1), np.int32)
    out = np.zeros(max(total, 1), np.uint8)
    check(lib().sfmhip_recover_pose(ctx.h, n, off.ctypes.data, left.ctypes.data, right.ctypes.data, Ec.ctypes.data, float(focal),
                                    float(pp[0]), float(pp[1]), float(distance_thresh), m_in.ctypes.data if m_in is not None else None,
                                    R.ctypes.data, t.ctypes.data, ng.ctypes.data, out.ctypes.data), "sfmhip_recover_pose")
    return R[:n].reshape(-1, 3, 3), t[:n], ng[:n], [out[off[i]:off[i + 1]].copy() for i in range(n)]


def essential_pose(pairs_points, K, prob=0.999, threshold=1.0, ctx=None):
    """sfmhip_essential_pose: findEssentialMat(K, RANSAC, prob, threshold) then recoverPose with its mask, per pair.
    Returns dict(E (n, 3, 3), inliers, R (n, 3, 3), t (n, 3), n_good (-1: no model), masks [uint8 per pair])."""
    ctx = ctx or default_context()
    n = len(pairs_points)
    off = _offsets(pairs_points)
    left, right = _cat(pairs_points, 0), _cat(pairs_points, 1)
    K = np.asarray(K, np.float64)
    E, R, t = np.zeros((max(n, 1), 9)), np.zeros((max(n, 1), 9)), np.zeros((max(n, 1), 3))
    inl, ng = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    out = np.zeros(max(int(off[-1]), 1), np.uint8)
    check(lib().sfmhip_essential_pose(ctx.h, n, off.ctypes.data, left.ctypes.data, right.ctypes.data, float(K[0, 0]), float(K[1, 1]),
                                      float(K[0, 2]), float(K[1, 2]), float(prob), float(threshold), E.ctypes.data, inl.ctypes.data,
                                      R.ctypes.data, t.ctypes.data, ng.ctypes.data, out.ctypes.data), "sfmhip_essential_pose")
    return dict(E=E[:n].reshape(-1, 3, 3), inliers=inl[:n], R=R[:n].reshape(-1, 3, 3), t=t[:n], n_good=ng[:n],
                masks=[out[off[i]:off[i + 1]].copy() for i in range(n)])


def last_flags(ctx=None):
    """sfmhip_pose_last_flags: bit 0 = a singular value of some E was <= DBL_MIN (OpenCV's random-vector branch, not
    restated)."""
    return int(lib().sfmhip_pose_last_flags((ctx or default_context()).h))


def determinante(R):
    """StructFromMotion::determinante (src/Sfm.cpp:1119-1131): Eigen::FullPivLU(R).determinant(), as csrc/pose.h restates it."""
    m = [[float(v) for v in row] for row in np.asarray(R, np.float64).reshape(3, 3)]
    swaps = 0
    for k in range(3):
        br, bc, best = k, k, abs(m[k][k])
        for j in range(k, 3):
            for i in range(k, 3):
                if abs(m[i][j]) > best:
                    best, br, bc = abs(m[i][j]), i, j
        if best == 0:
            break
        if br != k:
            m[k], m[br] = m[br], m[k]
            swaps += 1
        if bc != k:
            for row in m:
                row[k], row[bc] = row[bc], row[k]
            swaps += 1
        for i in range(k + 1, 3):
            m[i][k] /= m[k][k]
        for j in range(k + 1, 3):
            for i in range(k + 1, 3):
                m[i][j] -= m[i][k] * m[k][j]
    return (-1.0 if swaps % 2 else 1.0) * (m[0][0] * m[1][1] * m[2][2])


def check_coherent_rotation(R):
    """CheckCoherentRotation (src/Sfm.cpp:791-799): fabsf(det) - 1.0 > 1e-07 fails; fabsf narrows det to float, so a det
    that rounds to 1.0f passes and a NaN passes."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = float(np.abs(np.float32(determinante(R))))
    return not (d - 1.0 > 1e-07)


def get_camera_pose(K, left, right, ctx=None):
    """getCameraPose's numerics for one pair of aligned points: None when K is empty, 7 or fewer points are aligned, RANSAC
    finds no model or the rotation check fails; else dict(Pleft, Pright, E, R, t, n_good, mask, inliers)."""
    if K is None or np.asarray(K).size == 0 or len(left) < MIN_ALIGNED:
        return None
    r = essential_pose([(left, right)], K, ctx=ctx)
    return _pose_result(r, 0)


def _pose_result(r, i):
    if r["n_good"][i] < 0 or not check_coherent_rotation(r["R"][i]):
        return None
    Pright = np.hstack([r["R"][i], r["t"][i][:, None]])
    return dict(Pleft=np.hstack([np.eye(3), np.zeros((3, 1))]), Pright=Pright, E=r["E"][i], R=r["R"][i], t=r["t"][i],
                n_good=int(r["n_good"][i]), mask=r["masks"][i], inliers=int(r["inliers"][i]))


def base_reconstruction(best_views, points, matches, K, dist=None, ctx=None):
    """baseReconstruction (src/Sfm.cpp:408-492) after findBestPair: best_views = [(ratio, (q, t))] ascending (the map's
    order); points[i] = image i's 2-D points; matches[(q, t)] = (query indices, train indices).  One essential_pose call
    over every entry, then the first pair whose pose passes is triangulated.  Returns None (no pair) or dict(pair, pose,
    cloud) -- the cloud as triangulate.triangulate_views returns it."""
    entries = [pair for _, pair in best_views]
    if not entries or K is None or np.asarray(K).size == 0:     # (getCameraPose refuses an empty K for every pair)
        return None
    pts = [(np.asarray(points[q], np.float64)[np.asarray(matches[(q, t)][0])], np.asarray(points[t], np.float64)[np.asarray(matches[(q, t)][1])])
           for q, t in entries]
    r = essential_pose(pts, K, ctx=ctx)
    for i, (q, t) in enumerate(entries):
        if len(pts[i][0]) < MIN_ALIGNED:
            continue
        pose = _pose_result(r, i)
        if pose is None:
            continue
        cloud = _tri.triangulate_views(points[q], points[t], pose["Pleft"], pose["Pright"], matches[(q, t)][0], matches[(q, t)][1], K,
                                       np.zeros(5) if dist is None else dist, (q, t), ctx=ctx)
        return dict(pair=(q, t), pose=pose, cloud=cloud)
    return None
