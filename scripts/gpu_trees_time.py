"""Host-clock time of the tree extraction on the GPU (sfmhip_cloud_trees, trees.py) on nine planted trees 5 apart on a ground
disc (tests/test_trees_cpu.plot), at 200 k and 1 M points and the default options.  Prints one JSON line and, with --out,
writes it to a file: per size, the stages of one call as the library clocks them under sfmhip_set_timing (of --reps calls
after a warm-up, the call with the median total), the call's wall time without stage timing (the median of --reps warm
calls), the sweeps enqueued, and beside them the g++ build of the same header (the test stub, run_host) on 16 threads and
whether the two agree byte for byte.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of
time ends the script: nothing more is started on the GPU after it.

  stage    what it covers
  frame    labels upload, trs_frame, the bounds of A and their read-back
  stems    the band histogram, the components, the per-component sums, two scans and their read-backs
  voxels   trs_vkeys, the cell sort, trs_heads, the scan and its read-back, trs_vox_emit, trs_adj
  sweeps   trs_sweep in batches of 16, one 4-byte read-back per batch
  labels   trs_vlabel, trs_plabel, tree_of and the stem table back on the host
  total    the whole call
`relaxations` = voxels x sweeps enqueued; over the sweeps' time it is the voxel relaxations (26 neighbour keys each) per second
the loop sustains, read-backs included.
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

GRID9 = [(5.0 * i, 5.0 * j) for j in (-1, 0, 1) for i in (-1, 0, 1)]


def child(n, reps, cpu):
    from sfm_danpipeline_amd import _lib, trees
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_trees_cpu import STUB, load_stub, plot, same_run, stub_opts, stub_run
    n_tree = (6 * n // 10) // len(GRID9)
    xyz = plot(41, GRID9, n_tree=n_tree, n_ground=n - n_tree * len(GRID9), radius=12.0)[0]
    ctx = _lib.default_context()
    out = {"n": len(xyz), "trees_planted": len(GRID9)}
    with Cloud(xyz, ctx=ctx) as c:
        o = trees.default_opts(ground=0.0)
        run = trees.trees(c, opts=o)                         # warm-up: the handle's blocks, rocPRIM's temporary storage
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            trees.trees(c, opts=o)
            walls.append((time.perf_counter() - t0) * 1e3)
        out["call"] = round(float(np.median(walls)), 3)
        ctx.set_timing(True)
        stages = []
        for _ in range(reps):
            trees.trees(c, opts=o)
            stages.append(trees.last_timing(c))
        ctx.set_timing(False)
        stages.sort(key=lambda s: s["total"])
        mid = stages[len(stages) // 2]
        out.update({k: round(v, 3) for k, v in mid.items() if k != "n_sweeps"})
        out["sweeps_enqueued"] = int(mid["n_sweeps"])
    res = run[2]
    out["relaxations"] = int(res.n_voxels) * out["sweeps_enqueued"]
    out["relaxations_per_s"] = round(out["relaxations"] / (out["sweeps"] * 1e-3), 1) if out["sweeps"] > 0 else None
    out.update(n_above=int(res.n_above), n_band=int(res.n_band), n_trees=int(res.n_trees), n_voxels=int(res.n_voxels),
               n_labelled=int(res.n_labelled), max_cost=int(res.max_cost), flags=int(res.flags))
    if cpu:
        so = os.path.join(tempfile.mkdtemp(), "libtreescapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
        tr = load_stub(so)
        t0 = time.perf_counter()
        srun = stub_run(tr, xyz, opts=stub_opts(tr, ground=0.0), threads=16)
        out["cpu_stub_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["equal_to_stub"] = bool(same_run(srun, run))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240)
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
