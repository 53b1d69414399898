"""Host-clock time of map3D's step 10 on the GPU (sfmhip_cloud_*, cloud.py) for a 1 M point cloud: surfaces plus 5 %
uniform outliers, scaled so that r = 0.07 holds 150-600 neighbours.  Prints one JSON line: ms per stage after a
warm-up (the median of --reps runs), and the same queries on scipy's cKDTree with 16 workers -- a CPU k-d tree, NOT
PCL.  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python scripts/gpu_cloud_time.py`.

  stage            what one run does
  create           upload + the host's box pass (sfmhip_cloud_create)
  passthrough      x in [0.003, 0.83]: flags, scan, scatter, download
  radius_grid      the first radius call on a handle: grid build + capped counts + compaction
  radius_outlier   the same call again (grid reused): capped counts (cap 151) + compaction
  radius_count     exact counts (no cap), grid reused
  knn10            the k-NN grid (built on a fresh handle's first call) + 10 nearest, download
  normals10        NormalEstimation k = 10 on the same handle (grid reused)
  step10           map3d_step10: create + the three calls on a fresh handle, as the reference runs them
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (load torch's ROCm runtime first, as bench.py does)
except ImportError:
    pass
from sfm_danpipeline_amd import _lib, cloud  # noqa: E402
from tests.test_cloud_cpu import surface_cloud  # noqa: E402


def ms(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    xyz = surface_cloud(a.n, 0, outliers=0.05, scale=3.0 * np.sqrt(a.n / 1e6))
    ctx = _lib.default_context()
    out = {"n": a.n}
    cloud.map3d_step10(xyz, ctx=ctx)                                     # warm-up: code objects, scratch
    out["create"] = ms(lambda: cloud.Cloud(xyz, ctx=ctx).close(), a.reps)
    c = cloud.Cloud(xyz, ctx=ctx)
    out["passthrough"] = ms(lambda: c.passthrough(), a.reps)

    def fresh_radius():
        with cloud.Cloud(xyz, ctx=ctx) as f:
            f.radius_outlier()
    out["radius_grid"] = round(ms(fresh_radius, a.reps) - out["create"], 3)
    out["radius_outlier"] = ms(lambda: c.radius_outlier(), a.reps)
    counts = c.radius_count(cloud.RADIUS)
    out["radius_count"] = ms(lambda: c.radius_count(cloud.RADIUS), a.reps)
    out["median_neighbours"] = int(np.median(counts))
    out["kept"] = int(len(c.radius_outlier()))

    def fresh_knn():
        with cloud.Cloud(xyz, ctx=ctx) as f:
            f.knn(10)
    out["knn10"] = round(ms(fresh_knn, a.reps) - out["create"], 3)
    c.knn(10)
    out["knn10_grid_reused"] = ms(lambda: c.knn(10), a.reps)
    out["normals10"] = ms(lambda: c.normals(10), a.reps)
    out["step10"] = ms(lambda: cloud.map3d_step10(xyz, ctx=ctx), a.reps)
    c.close()
    if not a.no_scipy:
        from scipy.spatial import cKDTree
        x64 = xyz.astype(np.float64)
        t0 = time.perf_counter()
        t = cKDTree(x64)
        out["cpu_kdtree_build"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["cpu_kdtree_radius_count"] = ms(lambda: t.query_ball_point(x64, cloud.RADIUS, return_length=True, workers=16), 1)
        out["cpu_kdtree_knn10"] = ms(lambda: t.query(x64, k=10, workers=16), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
