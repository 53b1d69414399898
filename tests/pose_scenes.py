"""Scenes of the pose tests (tests/test_pose_cpu.py on the CPU, tests/test_gpu_pose.py on the device).  A plain module:
numpy only, no fixtures, no device code.  synth.two_view_scene has one pose for every seed, and recoverPose picks its
candidate 2 for it every time; the scenes here are built so that each of the four candidates [R1|t], [R2|t], [R1|-t],
[R2|-t] wins somewhere, so that counts tie, and so that E leaves the range the decomposition is comfortable in.  What
the header makes of them (the winners, the tied counts, the flags) is asserted in tests/test_pose_cpu.py, so a change
here cannot quietly empty a device test."""
import numpy as np

K = np.array([[1520.0, 0, 302.2], [0, 1490.0, 246.87], [0, 0, 1]])   # fx != fy: recoverPose takes fx for both axes
F, PPX, PPY = K[0, 0], K[0, 2], K[1, 2]
K1 = np.array([[F, 0, PPX], [0, F, PPY], [0, 0, 1]])                 # the calibration scene() projects with: one focal


def rod(*r):
    """the rotation matrix of the axis-angle vector r"""
    r = np.asarray(r[0] if len(r) == 1 else r, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def essential(R, t):
    """[t]x R at Frobenius norm 1"""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


def scene(R, t, m, seed, noise, outliers=0.0):
    """m world points in [-1, 1]^2 x [4, 8] seen by P1 = [I | 0] and P2 = [R | t], in pixels of the one focal K[0, 0]
    about (K[0, 2], K[1, 2]) -- recoverPose's normalisation -- with `noise` px of Gaussian noise on both views and the
    fraction `outliers` of the right pixels displaced by up to 60 px.  Every point is in front of both cameras (asserted).
    Returns (left m x 2, right m x 2)."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(4, 8, m)], axis=1)
    X2 = X @ np.asarray(R).T + np.asarray(t)
    assert (X[:, 2] > 0).all() and (X2[:, 2] > 0).all()
    a = X[:, :2] / X[:, 2:3] * F + [PPX, PPY]
    b = X2[:, :2] / X2[:, 2:3] * F + [PPX, PPY]
    a = a + rng.normal(0, noise, (m, 2))
    b = b + rng.normal(0, noise, (m, 2))
    bad = rng.random(m) < outliers
    b[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
    return a, b


# ---------------------------------------------------------------- the four-pose family
# One E up to sign has four poses: (R, t), (R, -t), (Rtw, t), (Rtw, -t) with Rtw = rot(pi about t) R, the twisted pair.
# A forward baseline keeps the twisted camera looking at the scene; one mostly along x or y has no twisted scene in
# front of both cameras.
T = np.array([0.1, 0.05, 1.0])
R0 = rod(0.02, -0.15, 0.01)
ROTATIONS = [R0, rod(0.3, 0.1, -0.2), rod(-0.1, 0.2, 0.4)]


def twisted(R, t=T):
    return rod(np.pi * np.asarray(t) / np.linalg.norm(t)) @ R


def family(R=R0, t=T):
    """the four true poses [(R, t)] that share essential(R, t) up to sign, in the order (R, +t), (R, -t), (Rtw, +t),
    (Rtw, -t)"""
    Rtw = twisted(R, t)
    return [(R, t), (R, -t), (Rtw, t), (Rtw, -t)]


# the candidate the header picks for family(R0)'s members in order, for E and for -E alike (asserted on the CPU)
FAMILY_WINNERS = [1, 3, 0, 2]

E0 = essential(R0, T)


# ---------------------------------------------------------------- ties
# (members of family(R0) and how many noise-free points of each, the four counts, the chosen candidate), all under E0
TIES = [
    ([(0, 5), (1, 5)], [0, 5, 0, 5], 1),
    ([(2, 7), (1, 7)], [7, 0, 0, 7], 0),
    ([(0, 3), (1, 3), (2, 3), (3, 3)], [3, 3, 3, 3], 0),
    ([(1, 4), (2, 5)], [5, 0, 0, 4], 0),
]


def mixture(parts, seed=500):
    """noise-free points of family(R0)'s members, concatenated: parts = [(member, count)]"""
    fam = family()
    ab = [scene(*fam[k], n, seed + 10 * i + k, 0.0) for i, (k, n) in enumerate(parts)]
    return np.concatenate([a for a, _ in ab]), np.concatenate([b for _, b in ab])


# ---------------------------------------------------------------- degenerate and scaled E
# name -> (E, the header's flags).  Squares of E's entries feed sfm_hypot: below 1e-75 they are under its TINY_VAL
# (2^-459), at 1e-200 they underflow to zero and at 1e200 overflow to inf, where a singular value is not > DBL_MIN
# (FLAG_SVD_RANDOM).
_u, _v = np.array([1.0, -2.0, 0.5]), np.array([0.3, 0.7, -1.1])
DEGENERATE = {
    "zero": (np.zeros((3, 3)), 1),
    "rank1": (np.outer(_u, _v), 1),
    "nan": (np.full((3, 3), np.nan), 1),
    "1e-200": (E0 * 1e-200, 1),
    "1e200": (E0 * 1e200, 1),
    "1e-75": (E0 * 1e-75, 0),
    "1e-100": (E0 * 1e-100, 0),
    "1e-140": (E0 * 1e-140, 0),
    "1e60": (E0 * 1e60, 0),
    "1e75": (E0 * 1e75, 0),
}
FLAGGED = [k for k, (_, fl) in DEGENERATE.items() if fl]
UNFLAGGED = [k for k, (_, fl) in DEGENERATE.items() if not fl]

MASK_BYTES = np.array([0, 1, 7, 200, 255], np.uint8)
THRESHOLDS = [50.0, 6.0, 3.0, 0.0, -1.0, float("inf"), float("nan")]


def mask_bytes(m, seed=8):
    """m bytes drawn from MASK_BYTES, every one of the five present"""
    out = MASK_BYTES[np.random.default_rng(seed).integers(0, 5, m)]
    out[:5] = MASK_BYTES
    return out
