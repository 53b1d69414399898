"""The planted terrain scenes of tests/test_terrain_cpu.py and tests/test_gpu_terrain.py: five planted trees
(tests/test_dendro_cpu.planted) on a 24 m square whose ground is z = s x + a sin(x / 4) cos(y / 5) with noise sigma 0.01 and
no ground point within 1.5 m of a stem (the hole a crown's shadow leaves), optionally rotated and divided by a scale."""
import numpy as np

from tests.test_dendro_cpu import planted, rotation

CENTRES = [(-7.0, -6.0), (6.0, -7.0), (0.5, 0.0), (-6.0, 7.0), (7.0, 6.0)]
HALF, HOLE, SIGMA = 12.0, 1.5, 0.01
# the two scenes whose accuracy DESIGN.md f-20 records: (a, s, cell)
TABLE = {"gentle": (1.0, 0.25, 0.25), "steep": (1.5, 0.5, 0.25)}


def surface(x, y, a, s):
    return s * x + a * np.sin(x / 4.0) * np.cos(y / 5.0)


def scene(seed, a=1.0, s=0.25, n_tree=20000, n_ground=40000, rot=None, scale=1.0, centres=CENTRES):
    """(xyz float32 [n, 3], member [n]: -1 ground, k tree k, above float64 [n]: the true height of every point above the analytic
    terrain at its own (x, y), in metres, R)."""
    rng = np.random.default_rng(7000 + seed)
    g = rng.uniform(-HALF, HALF, (n_ground, 2))
    keep = np.ones(n_ground, bool)
    for cx, cy in centres:
        keep &= np.hypot(g[:, 0] - cx, g[:, 1] - cy) >= HOLE
    g = g[keep]
    noise = rng.normal(0, SIGMA, len(g))
    parts = [np.column_stack([g, surface(g[:, 0], g[:, 1], a, s) + noise])]
    member = [np.full(len(g), -1, np.int32)]
    for k, (cx, cy) in enumerate(centres):
        t = planted(100 * seed + k, n_tree)[0].astype(np.float64)
        parts.append(t + np.array([cx, cy, surface(cx, cy, a, s)]))
        member.append(np.full(len(t), k, np.int32))
    xyz, member = np.concatenate(parts), np.concatenate(member)
    above = xyz[:, 2] - surface(xyz[:, 0], xyz[:, 1], a, s)
    R = np.eye(3) if rot is None else rotation(rot)
    perm = rng.permutation(len(xyz))
    return ((xyz @ R.T) / scale)[perm].astype(np.float32), member[perm], above[perm], R


def plane_heights(xyz, member):
    """Heights above the least-squares plane z = p x + q y + r through the true ground points of an unrotated scene."""
    p = xyz.astype(np.float64)
    g = p[member < 0]
    coef, *_ = np.linalg.lstsq(np.column_stack([g[:, 0], g[:, 1], np.ones(len(g))]), g[:, 2], rcond=None)
    return p[:, 2] - (coef[0] * p[:, 0] + coef[1] * p[:, 1] + coef[2])
