"""The planted crown scenes of tests/test_crowns_cpu.py and tests/test_gpu_crowns.py: paraboloid crowns without a stem over a
flat ground, as a cloud taken from above shows a plot.  The ground is uniform on the square [-half, half]^2 with z-noise
sigma 0.02.  A tree (cx, cy, ht, rad) has `per` points uniform over its disc at heights 0.4 ht + 0.6 ht (1 - (r / rad)^2) plus
N(0, 0.05), and one point exactly at (cx, cy, ht).  APART's crowns are further from each other than any window; TOUCHING's
overlap."""
import numpy as np

APART = [(-9, -8, 18, 3.0), (8, -9, 9, 1.5), (0, 0, 24, 4.0), (-8, 9, 12, 2.0), (9, 8, 15, 2.5), (0, -10.5, 6, 1.2)]
TOUCHING = [(-4, 0, 18, 3.0), (1.2, 0, 12, 2.2), (4.6, 0.5, 9, 1.5), (0, 5, 22, 3.5), (-5.5, 5, 8, 1.4)]


def scene(seed, trees, half=14, n_ground=20000, per=4000):
    """(xyz float32 [n, 3], member int32 [n]: -1 ground, k tree k), in input order: ground, then tree by tree, a tree's apex
    last."""
    rng = np.random.default_rng(9000 + seed)
    g = rng.uniform(-half, half, (n_ground, 2))
    parts = [np.column_stack([g, rng.normal(0, 0.02, n_ground)])]
    member = [np.full(n_ground, -1, np.int32)]
    for k, (cx, cy, ht, rad) in enumerate(trees):
        r, a = rad * np.sqrt(rng.uniform(0, 1, per)), rng.uniform(0, 2 * np.pi, per)
        z = 0.4 * ht + 0.6 * ht * (1 - (r / rad) ** 2) + rng.normal(0, 0.05, per)
        parts.append(np.column_stack([cx + r * np.cos(a), cy + r * np.sin(a), z]))
        parts.append(np.array([[cx, cy, ht]], np.float64))
        member.append(np.full(per + 1, k, np.int32))
    return np.concatenate(parts).astype(np.float32), np.concatenate(member)


def max_raster(xyz, c, half=14):
    """The canopy raster taken directly: each cell's largest z, NaN for a cell without points; [Dn, De] over [-half, half]^2."""
    D = int(round(2 * half / c))
    ix = np.clip(np.floor((xyz[:, 0].astype(np.float64) + half) / c).astype(int), 0, D - 1)
    iy = np.clip(np.floor((xyz[:, 1].astype(np.float64) + half) / c).astype(int), 0, D - 1)
    Z = np.full(D * D, -np.inf, np.float32)
    np.maximum.at(Z, iy * D + ix, xyz[:, 2])
    Z[np.isneginf(Z)] = np.nan
    return Z.reshape(D, D), iy * D + ix
