"""Host-clock time of the two cloud filters on the GPU (sfmhip_cloud_voxel_grid, sfmhip_cloud_statistical_outlier; DESIGN.md
f-15) on the benchmark scene of tests/test_gpu_cloud.py at 1 M and 4 M points: leaf 0.02 (about ten points per voxel there)
and mean_k 16, std_mul 1.  Prints one JSON line and, with --out, writes it to a file.  Per size: the stages of each call as
the library clocks them under sfmhip_set_timing (of --reps calls after a warm-up, the call with the median sum), each
call's wall time without stage timing, and the yardsticks of the same job -- Cloud.knn(17) on the same handle (it writes
34 n words where the outlier call writes n floats), and the g++ build of the same header (the test stub: the voxel grid on
one thread, the outlier removal on 16) with whether the two agree bit for bit.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of
time ends the script: nothing more is started on the GPU after it.

  stage      what it covers
  key_sort   vg_keys and the radix sort of (voxel, point) pairs
  reduce     run heads, both scans and their read-backs, vg_reduce, vg_voxel_of, the copies to the host
  means      the k-NN grid on first use (not in the warmed figure), sor_mean_dist
  threshold  sor_partials, their copy and the host's sum, the flags, the scan, the scatter and the copies to the host
`voxel_bytes` is what a voxel grid has to move whatever its method: 12 n in, 4 n (voxel_of) and 12 m out.  Over the call's
device stages (key_sort + reduce) and the HBM peak of 8.0 TB/s it gives `voxel_share_of_hbm_peak`: the bound is bandwidth,
the call has no arithmetic to speak of.
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
HBM_PEAK = 8.0e12
LEAF, MEAN_K, STD_MUL = 0.02, 16, 1.0


def median_call(f, reps):
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        walls.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(walls)), 3)


def child(n, reps, cpu):
    from sfm_danpipeline_amd import _lib
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_cloud_cpu import surface_cloud
    from tests.test_cloud_filter_cpu import bits, build_stub, stub_sor, stub_voxel_grid
    xyz = surface_cloud(n, 0, outliers=0.05, scale=3.0 * np.sqrt(n / 1e6))
    ctx = _lib.default_context()
    out = {"n": n, "leaf": LEAF, "mean_k": MEAN_K}
    with Cloud(xyz, ctx=ctx) as c:
        vg = c.voxel_grid(LEAF)                                  # warm-up: the handle's blocks, rocPRIM's temporary storage
        kept, md, thr = c.statistical_outlier(MEAN_K, STD_MUL, return_distances=True)   # ... and the k-NN grid
        c.knn(MEAN_K + 1)
        out["voxels"], out["kept"] = int(len(vg["xyz"])), int(len(kept))
        out["voxel_grid_call"] = median_call(lambda: c.voxel_grid(LEAF), reps)
        out["outlier_call"] = median_call(lambda: c.statistical_outlier(MEAN_K, STD_MUL), reps)
        out["knn17_call"] = median_call(lambda: c.knn(MEAN_K + 1), reps)
        ctx.set_timing(True)
        stages = []
        for _ in range(reps):
            c.voxel_grid(LEAF)
            c.statistical_outlier(MEAN_K, STD_MUL)
            stages.append(c.filter_last_timing())
        ctx.set_timing(False)
        stages.sort(key=sum)
        out.update({k: round(v, 3) for k, v in zip(("key_sort", "reduce", "means", "threshold"), stages[len(stages) // 2])})
    out["voxel_bytes"] = 12 * n + 4 * n + 12 * out["voxels"]
    dev = (out["key_sort"] + out["reduce"]) * 1e-3
    out["voxel_share_of_hbm_peak"] = round(out["voxel_bytes"] / HBM_PEAK / dev, 5) if dev > 0 else None
    if cpu:
        cf = build_stub(__import__("pathlib").Path(tempfile.mkdtemp()))
        t0 = time.perf_counter()
        rc, svg = stub_voxel_grid(cf, xyz, LEAF)
        out["cpu_stub_voxel_grid_1_thread"] = round((time.perf_counter() - t0) * 1e3, 3)
        t0 = time.perf_counter()
        rc2, skept, smd, sthr = stub_sor(cf, xyz, MEAN_K, STD_MUL)
        out["cpu_stub_outlier_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["equal_to_stub"] = bool(rc == 0 and rc2 == 0 and np.array_equal(bits(svg["xyz"]), bits(vg["xyz"])) and
                                    np.array_equal(svg["voxel_of"], vg["voxel_of"]) and np.array_equal(skept, kept) and
                                    np.array_equal(bits(smd), bits(md)) and sthr == thr)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,4000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, not a.no_cpu)
        return 0
    result = {"device": "MI355X", "reps": a.reps, "sizes": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps)] + (["--no-cpu"] if a.no_cpu else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            return 1                                             # nothing more on the GPU after a failure
        result["sizes"].append(json.loads(line[0][7:]))
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
