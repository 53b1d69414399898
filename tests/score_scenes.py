"""Scene tables and generators of the pair-scoring tests (tests/test_gpu_score.py on the device, the guard in
tests/test_oracle_score.py on the CPU).  A plain module: numpy, the synthetic scenes and the oracle, no device code.
Every table entry was found by a seed search with the oracle on the CPU; the guard asserts that the oracle still gives
what the tables promise, so a change to synth.two_view_scene cannot quietly empty a device test."""
import numpy as np

from oracle import orc
from oracle import sfm_oracle_score as S
from sfm_danpipeline_amd import synth

K = np.array([[1520.0, 0, 302.2], [0, 1520.0, 246.87], [0, 0, 1]])          # the calibration of tests/test_gpu_score.py


def scene(m, seed, outliers=0.1, noise=0.3, K=K):
    sc = synth.two_view_scene(m=m, seed=seed, K=K, noise_px=noise, outlier_frac=outliers)
    return sc["xy1"], sc["xy2"]


# ---------------------------------------------------------------- 1. essential RANSAC off its defaults
# fx != fy in both: score_normalize scales x by 1 / fx and y by 1 / fy, the threshold is divided by (fx + fy) / 2.
# K_TALL has fx < fy, K_WIDE fx > fy: a swap of the axes moves the principal point by ~75 px and the scale by 15 %.
K_TALL = np.array([[1400.0, 0, 310.0], [0, 1650.0, 235.0], [0, 0, 1]])
K_WIDE = np.array([[1710.0, 0, 295.0], [0, 1330.0, 260.0], [0, 0, 1]])
# (prob, threshold) -> the oracle's (inliers, iterations) on two_view_scene(500, 77, K, 0.5, 0.4) for either K
OPTIONS_TALL = [((0.999, 1.0), (280, 122)), ((0.99, 1.0), (280, 81)), ((0.9999, 1.0), (280, 163)),
                ((0.999, 0.5), (193, 803)), ((0.999, 2.5), (302, 82)), ((0.9, 3.0), (302, 27))]
OPTIONS_WIDE = [((0.999, 1.0), (222, 397)), ((0.99, 1.0), (222, 265)), ((0.9999, 1.0), (249, 473)),
                ((0.999, 0.5), (153, 1000)), ((0.999, 2.5), (297, 90)), ((0.9, 3.0), (299, 29))]


def options_scene(K):
    sc = synth.two_view_scene(m=500, seed=77, K=K, noise_px=0.5, outlier_frac=0.4)
    return sc["xy1"], sc["xy2"]


# ---------------------------------------------------------------- 2. exact chunk ends
# The drivers run 32, 64, 128, then 256 iterations per chunk: cumulative ends at 32, 96, 224, 480, 736, 992.
# (m, outlier_frac, seed, expected_iterations) of scene(m, seed, outlier_frac, 0.3) at prob 0.999, threshold 1:
# a run that ends on a chunk end or one iteration after it, for every end below the cap, and one that runs to the cap.
CHUNK_ENDS = (32, 96, 224, 480, 736, 992)
CHUNK_TABLE = [
    (400, 0.28, 5040, 32), (400, 0.28, 5063, 33),
    (305, 0.413, 5002, 96), (400, 0.42, 5062, 97),
    (350, 0.503, 5001, 224), (300, 0.493, 5021, 225),
    (400, 0.58, 5070, 480), (344, 0.573, 5003, 481),
    (331, 0.607, 5008, 736), (326, 0.607, 5003, 737),
    (303, 0.617, 5014, 737),     # the best model is found IN iteration 737, the first of its chunk, and ends the run there
    (354, 0.607, 5019, 992),     # the same at the last iteration of a chunk
    (300, 0.62, 5031, 993),
    (300, 0.8, 5000, 1000),      # the cap
]


def chunk_pairs():
    return [scene(m, seed, outliers=o, noise=0.3) for m, o, seed, _ in CHUNK_TABLE]


# ---------------------------------------------------------------- 3. small counts, ties
def tie_census(a, b, K=K, prob=0.999, threshold=1.0):
    """(best count, iterations, number of (iteration, model) that reach the final best count) of the oracle's RANSAC on
    a pair, re-run in numpy from the oracle's parts: S.subset_table, orc.em_normalize, orc.five_point, and the oracle's
    threshold rule (float)(error) <= (float)(thr^2) with thr = threshold / ((fx + fy) / 2).  More than one: the strict
    `>` and the order of a sample's models decide which of them is kept, and only the mask shows which."""
    n = len(a)
    cnt, mask, _, iters = S.find_essential_mat_ransac(a, b, K, prob, threshold)
    if n <= 5 or cnt == 0:
        return cnt, iters, 0
    n1, n2 = orc.em_normalize(a, K), orc.em_normalize(b, K)
    thr = threshold / ((K[0, 0] + K[1, 1]) / 2)
    t = np.float32(thr * thr)
    x1, y1, x2, y2 = n1[:, 0], n1[:, 1], n2[:, 0], n2[:, 1]
    reach, first = 0, None
    for idx in S.subset_table(n, iters):
        models, _ = orc.five_point(n1[idx], n2[idx])
        for E in models:
            e = E.reshape(9)
            ex0 = e[0] * x1 + e[1] * y1 + e[2] * 1.0
            ex1 = e[3] * x1 + e[4] * y1 + e[5] * 1.0
            ex2 = e[6] * x1 + e[7] * y1 + e[8] * 1.0
            et0 = e[0] * x2 + e[3] * y2 + e[6] * 1.0
            et1 = e[1] * x2 + e[4] * y2 + e[7] * 1.0
            d = x2 * ex0 + y2 * ex1 + 1.0 * ex2
            with np.errstate(all="ignore"):
                err = (d * d / (ex0 * ex0 + ex1 * ex1 + et0 * et0 + et1 * et1)).astype(np.float32)
            inl = err <= t
            if int(inl.sum()) == cnt:
                reach += 1
                if first is None:
                    first = inl
    assert first is not None and np.array_equal(first, mask.astype(bool))     # the census re-runs the oracle's own loop
    return cnt, iters, reach


# (count, seed, outlier_frac): scene(60, seed, outlier_frac)[:count] for counts 6 to 24, three scenes each.  On the CPU
# tie_census finds more than one (iteration, model) at the final best count in 17 of the 57: seeds 602, 701, 702, 802,
# 1102, 1201, 1202, 1301, 1303, 1502, 1701, 1702, 1703, 2001, 2102, 2201, 2202 (602, 702, 802 and 1202 with dozens to
# hundreds of models tied at five or six inliers).  The guard in tests/test_oracle_score.py asserts at least MIN_TIES.
SMALL_TABLE = [(count, 100 * count + k, o) for count in range(6, 25) for k, o in ((1, 0.1), (2, 0.3), (3, 0.0))]
MIN_TIES = 10


def small_pairs():
    out = []
    for count, seed, o in SMALL_TABLE:
        a, b = scene(60, seed, outliers=o)
        out.append((a[:count], b[:count]))
    return out


# ---------------------------------------------------------------- 6. homography scenes
H_TRUE = np.array([[1.02, 0.05, 12.0], [-0.03, 0.98, -7.0], [1e-5, -2e-5, 1.0]])


def planar(n, seed, outliers, noise=0.4):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 640, (n, 2))
    ph = np.concatenate([p, np.ones((n, 1))], 1) @ H_TRUE.T
    q = ph[:, :2] / ph[:, 2:] + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outliers
    q[out] = rng.uniform(0, 640, (int(out.sum()), 2))
    return p, q


# ---------------------------------------------------------------- 7. rejection sampling
def line_scene(n_off, seed, noise):
    """40 points on a line and n_off points off it, mapped by H_TRUE with `noise` px of noise: checkSubset rejects
    most samples (the last point collinear with two others), getSubset draws again and consumes cv::RNG doing so"""
    rng = np.random.default_rng(seed)
    k = np.sort(rng.choice(75, 40, replace=False)).astype(np.float64)
    line = np.stack([16.0 + 8.0 * k, 60.0 + 5.0 * k], 1)       # (integers: exactly collinear as float too)
    off = rng.uniform(0, 640, (n_off, 2))
    p = np.concatenate([line, off])
    p = p[rng.permutation(len(p))]
    ph = np.concatenate([p, np.ones((len(p), 1))], 1) @ H_TRUE.T
    q = ph[:, :2] / ph[:, 2:] + rng.normal(0, noise, p.shape)
    return p, q


# (points off the line, seed, the oracle's (inliers, iterations) at noise 0.3 and the reference's threshold): a sample
# whose last point is one of the 40 is rejected unless two of the other three are off the line, and the oracle runs at
# least 20 iterations on every set
LINE_NOISE = 0.3
LINE_TABLE = [(2, 0, (16, 249)), (2, 13, (19, 124)), (3, 28, (42, 44)), (4, 34, (44, 24)), (6, 19, (44, 20))]
