"""The edge scenes of tests/test_dendro_edges_cpu.py and tests/test_gpu_dendro_edges.py: deterministic clouds, each built for one
place where csrc/dendro.hip can go wrong without the planted trees of tests/test_dendro_cpu.py noticing -- slice populations on
the 64-lane stride, the 1 024-pair LDS chunk and the 256-thread refit pass, a cloud beyond one trip of dnd_keys' grid, the slice
cap, finite points under a given ground, the extent histogram's last bin and both ends of extent_q.  A builder returns
(xyz float32 [n, 3], the option keywords it is meant to run with, a dict of what was planted); the CPU file asserts the planted
facts on the stub's output, so a scene that stops reaching its edge fails there and not silently on the device."""
import numpy as np

from tests.test_dendro_cpu import planted

# around min_slice_pts = 10, a wave (64), dnd_refit's pass (256), dnd_ransac's LDS chunk (1 024), two chunks, and three chunks + 1
POPS = (9, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
SLICE_STACK_SEED = 4
RING_R, RING_SIGMA = 0.15, 0.005


def slice_stack(pops=POPS, seed=SLICE_STACK_SEED):
    """Slice k holds exactly pops[k] points, all at height 0.05 + 0.1 k (with ground = 0 and 0.1 slices: the middle of slice k).
    Two thirds of a slice (rounded down) are a noisy ring about the origin (r = 0.15, sigma 0.005), the rest uniform clutter in
    [-1, 1]^2; the cloud is shuffled.  With the default pops the DBH slices 12 and 13 hold 2 047 and 2 048 points."""
    rng = np.random.default_rng(seed)
    parts = []
    for k, m in enumerate(pops):
        nr = (2 * m) // 3
        a = rng.uniform(0, 2 * np.pi, nr)
        r = RING_R + rng.normal(0, RING_SIGMA, nr)
        en = np.concatenate([np.stack([r * np.cos(a), r * np.sin(a)], 1), rng.uniform(-1, 1, (m - nr, 2))])
        parts.append(np.concatenate([en, np.full((m, 1), 0.05 + 0.1 * k)], 1))
    xyz = np.concatenate(parts)
    xyz = xyz[rng.permutation(len(xyz))].astype(np.float32)
    return xyz, dict(ground=0.0, min_inliers=5), dict(pops=list(pops), n=int(sum(pops)))


CAP_SEED, CAP_SLICE, CAP_RING = 31, 0.002, 200
CAP_DBH_SLICES = (649, 650)            # 1.3 / 0.002 - 0.5 = 649.5: the two slices rule 7 interpolates between


def capped_slices():
    """planted(31, 6000) in 0.002 slices: 9.05 / 0.002 = 4 525 slices, capped at MAX_SLICES = 4 096, so the top slice 4 095 takes
    every point from 8.19 up (646 of them).  The trunk leaves about one point per slice, which is no stem, so an exact ring of 200
    points (r = 0.15) is added at heights 1.299 and 1.301, the slices 649 and 650 around the DBH height: both are stems, rule 7
    interpolates and dnd_extent runs over all 4 096 slices.  (The capped slice's crown points hold a circle of 20 inliers in 6
    sectors as well: it is the table's third stem row, and its last.)
    Flags: NO_CROWN (8) with these options -- only slices 649, 650 and 4 095 reach min_slice_pts, so no run of crown_run = 3
    slices qualifies.  With crown_run = 1 (`planted["crown_kw"]`) the capped slice alone is the crown base: flags 0,
    crown_base_slice 4 095, and rule 10's spread is taken over the points of that slice."""
    xyz, _ = planted(CAP_SEED, 6000)
    a = 2 * np.pi * np.arange(CAP_RING) / CAP_RING
    rings = [np.stack([RING_R * np.cos(a + 0.01 * j), RING_R * np.sin(a + 0.01 * j), np.full(CAP_RING, h)], 1)
             for j, h in enumerate((1.299, 1.301))]
    xyz = np.concatenate([xyz] + [r.astype(np.float32) for r in rings])
    xyz = xyz[np.random.default_rng(CAP_SEED).permutation(len(xyz))]
    kw = dict(slice=CAP_SLICE)
    return xyz, kw, dict(S=4096, top_count=646, dbh_slices=CAP_DBH_SLICES, ring=CAP_RING, crown_kw=dict(kw, crown_run=1))


BELOW_SEED, BELOW_GROUND = 32, 0.75


def below_ground():
    """planted(32, 30000) measured from ground = 0.75: the 1 913 trunk points under it are selected (n_selected = 30 000) and lie
    in no slice (the histogram's bucket S, past dnd_gather's end).  extent_bin = 0.001 puts every crown slice's farthest points
    beyond 1 023 bins, so with extent_q = 1 the largest extent is the clamped last bin, 1 024 * 0.001.  `planted["tiny_q_kw"]`
    is the other end: extent_q = 1e-9, need = 1, the bin of the nearest point."""
    xyz, _ = planted(BELOW_SEED, 30000)
    kw = dict(ground=BELOW_GROUND, extent_bin=0.001, extent_q=1.0)
    return xyz, kw, dict(under=1913, n=len(xyz), last_extent=1024 * 0.001, tiny_q_kw=dict(kw, extent_q=1e-9))


KEY_GRID = 1024 * 256                  # dnd_keys' launch: at most 1 024 blocks of 256 threads
KEY_GRID_SEED, KEY_GRID_N = 33, 270000


def past_the_key_grid():
    """planted(33, 270000): more points than one trip of dnd_keys' grid-stride loop covers."""
    xyz, _ = planted(KEY_GRID_SEED, KEY_GRID_N)
    return xyz, dict(ransac_iters=16), dict(n=KEY_GRID_N)
