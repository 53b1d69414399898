"""Host-clock time of the colour region growing after map3D on the GPU (sfmhip_cloud_segment_rgb, segment.py) on the
patch scene of tests/test_segment_cpu.py (six colour patches, a gradient patch, 3 % salt points) at 200 k and 1 M
points.  Prints one JSON line and, with --out, writes it to a file: per size, the stages of one call as the library
clocks them (the median of --reps calls after a warm-up), and beside them the CPU build of the same header (the test
stub, 16 threads) and scipy's cKDTree 100-nearest query with 16 workers -- a CPU k-d tree, NOT PCL; context, not a gate.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python scripts/gpu_segment_time.py --no-cpu`.

  stage        what it covers
  knn          upload of the index list, gather, the grid of the indexed points, the 100 nearest of every indexed point
  growth       label propagation to the fixpoint (`rounds` launches)
  statistics   segment numbers, counts and colours, the segment-pair minima (sort + reduce), the top-100 lists, downloads
  regions      rules 8-10 on the host
  total        the whole sfmhip_cloud_segment_rgb call
  minmax       sfmhip_cloud_minmax (Dendrometry's bounds)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (load torch's ROCm runtime first, as bench.py does)
except ImportError:
    pass
from sfm_danpipeline_amd import _lib, cloud, segment  # noqa: E402
from tests.test_segment_cpu import STUB, load_stub, passthrough_z, patch_scene, ref_opts, stub_segment  # noqa: E402


def ms(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(ts)), 3)


def one_size(n, reps, ctx, sc):
    xyz, rgb, _, _ = patch_scene(n, 0)
    ind = passthrough_z(xyz)
    out = {"n": n, "n_idx": int(len(ind))}
    with cloud.Cloud(xyz, ctx=ctx) as c:
        labels, nc, st = segment.segment_rgb(c, rgb, ind)                  # warm-up: code objects, scratch
        runs = []
        for _ in range(reps):
            _, _, st = segment.segment_rgb(c, rgb, ind)
            runs.append(dict(segment.last_timing(c), rounds=st.rounds))
        for key in ("knn", "growth", "statistics", "regions", "total", "rounds"):
            out[key] = round(float(np.median([r[key] for r in runs])), 3)
        out.update(n_segments=st.n_segments, n_regions=st.n_regions, n_clusters=nc)
        out["minmax"] = ms(lambda: segment.minmax(c), reps)
    if sc is not None:
        t = time.perf_counter()
        slabels = stub_segment(sc, xyz, rgb, ind, ref_opts())[0]
        out["cpu_stub_16_threads"] = round((time.perf_counter() - t) * 1e3, 3)
        out["equal_to_stub"] = bool(np.array_equal(labels, slabels))
        from scipy.spatial import cKDTree
        x64 = xyz[ind].astype(np.float64)
        t = time.perf_counter()
        tree = cKDTree(x64)
        out["cpu_kdtree_build"] = round((time.perf_counter() - t) * 1e3, 3)
        out["cpu_kdtree_knn100"] = ms(lambda: tree.query(x64, k=100, workers=16), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[200_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    sc = None
    if not a.no_cpu:
        so = os.path.join(tempfile.mkdtemp(), "libsegmentcapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
        sc = load_stub(so)
    ctx = _lib.default_context()
    res = {"sizes": [one_size(n, a.reps, ctx, sc) for n in a.n]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
