"""The edge scenes of tests/test_ground_edges_cpu.py and tests/test_gpu_ground_edges.py: a plane patch with an off-plane column at
any size from 3 points up, so that the selection list of csrc/ground.hip can end exactly on, one before and one past a wave
(64), a refit pass (256), gnd_score's LDS chunk (1 024), for_own_points' batch (256 * 8 = 2 048) and gnd_score's point block
(8 192); and an exact plane under a scattered slab, whose tied iterations the option seed places in any wave and stride of
gnd_pick.  tests/test_ground_cpu.scene cannot go below three trunk points; these builders can.  A builder returns the cloud,
(labels and label,) the option keywords it is meant to run with and a dict of what was planted."""
import numpy as np

from tests.test_dendro_cpu import rotation

SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 2047, 2048, 2049, 8191, 8192, 8193, 16385)
DISC_KW = dict(min_inliers=3, ransac_iters=64, inlier_tol=0.03)
DISC_SEED = 7


def _disc(n, seed):
    rng = np.random.default_rng(seed)
    n_plane = (3 * n + 3) // 4                                                       # three quarters, rounded up: 3 of 3, 3 of 4
    plane = np.stack([rng.uniform(-5, 5, n_plane), rng.uniform(-5, 5, n_plane), rng.normal(0, 0.01, n_plane)], 1)
    m = n - n_plane
    column = np.stack([rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m), rng.uniform(0.5, 6.0, m)], 1)
    xyz = np.concatenate([plane, column])
    on_plane = np.concatenate([np.ones(n_plane, bool), np.zeros(m, bool)])
    perm = rng.permutation(n)
    R = rotation(seed)
    return (xyz[perm] @ R.T).astype(np.float32), on_plane[perm], R, rng


def ground_disc(n, seed=DISC_SEED):
    """n points: three quarters (rounded up) a noisy plane patch (sigma 0.01 over +-5), the rest a column above it at heights
    0.5 .. 6; shuffled, and rotated by rotation(seed) (the column's side is +R[:, 2]).  Every point is finite: n_selected = n."""
    xyz, on_plane, R, _ = _disc(n, seed)
    return xyz, dict(DISC_KW), dict(n=n, n_plane=int(on_plane.sum()), on_plane=on_plane, up=R[:, 2])


TIE_SLAB_KW = dict(ransac_iters=1024, refit_rounds=0, inlier_tol=0.1, min_inliers=200)
TIE_SLAB_WINNERS = {4: 88, 28: 149, 12: 192, 89: 320, 76: 475}          # option seed -> the first iteration that draws three plane points


def tie_slab():
    """225 points of the exact plane z = 0 (a 15 x 15 grid) under 675 points scattered at heights 1 .. 5, shuffled.  An iteration
    counts all 225 plane points if its three draws are plane points that span the plane, and at most a handful otherwise: the
    iterations of the first kind tie, and the first of them wins.  Which one that is depends on the option seed alone:
    TIE_SLAB_WINNERS lists seeds that put it in gnd_pick's second, third and fourth wave (threads 64 .., 128 .., 192 ..) and in
    its second stride (iterations 256 ..), each with later iterations that tie.  grid_plane()'s tie is always won by iteration 0,
    thread 0."""
    g = np.arange(15, dtype=np.float64)
    plane = np.stack([np.repeat(g, 15), np.tile(g, 15), np.zeros(225)], 1)
    rng = np.random.default_rng(3)
    slab = np.stack([rng.uniform(0, 14, 675), rng.uniform(0, 14, 675), rng.uniform(1, 5, 675)], 1)
    xyz = np.concatenate([plane, slab])[rng.permutation(900)].astype(np.float32)
    return xyz, dict(TIE_SLAB_KW), dict(n_plane=225, winners=dict(TIE_SLAB_WINNERS))


def pick_labels(planted, m):
    """Labels (1: picked, 0: not) that select m points of a ground_disc: the first 3 m / 4 of its plane points and the first m / 4
    of its column, by index."""
    on = planted["on_plane"]
    lab = np.zeros(len(on), np.int32)
    lab[np.nonzero(on)[0][:m - m // 4]] = 1
    lab[np.nonzero(~on)[0][:m // 4]] = 1
    assert int(lab.sum()) == m
    return lab


def ground_disc_masked(n_sel, n, seed=DISC_SEED):
    """ground_disc(n_sel) under label 4 among n rows: of the n - n_sel others, every second one is not finite (NaN, +inf or -inf in
    one coordinate, label 4 too) and the rest are finite points under label 9, far off the plane.  The selection list has n_sel
    rows, on an edge, while the kernels that walk all n rows (gnd_flag, gnd_emit, the scan) end on none.
    Returns (xyz, labels, label, option keywords, planted)."""
    disc, on_plane, R, rng = _disc(n_sel, seed)
    extra = n - n_sel
    other = rng.uniform(-5, 5, (extra, 3)).astype(np.float32)
    lab_other = np.full(extra, 9, np.int32)
    bad = np.arange(extra) % 2 == 0
    other[bad, np.arange(extra)[bad] % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[(np.arange(extra)[bad] // 2) % 3]
    lab_other[bad] = 4
    xyz = np.concatenate([disc, other])
    lab = np.concatenate([np.full(n_sel, 4, np.int32), lab_other])
    perm = rng.permutation(n)
    return xyz[perm], lab[perm], 4, dict(DISC_KW), dict(n_sel=n_sel, n=n, n_bad=int(bad.sum()), n_other=int((~bad).sum()))
