"""Host-clock time of the dendrometry call on the GPU (sfmhip_cloud_dendrometry, dendro.py) on the planted tree of
tests/test_dendro_cpu.py (a trunk, a crown shell) at 200 k and 1 M points.  Prints one JSON line and, with --out, writes
it to a file: per size, the stages of one call as the library clocks them under sfmhip_set_timing (of --reps calls after
a warm-up, the call with the median total), the call's wall time without stage timing, the slice count, and beside them
the g++ build of the same header (the test stub, run_host) on 16 threads and whether the two agree bit for bit.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of
time ends the script: nothing more is started on the GPU after it.

  stage    what it covers
  frame    labels upload, dnd_frame, the ground / top reduction and its read-back
  slices   dnd_keys, the slice scan, the stable cell sort, dnd_gather
  ransac   dnd_ransac (iterations x slices hypotheses, every point of the slice against each)
  refit    dnd_refit and the read-back of the slice table
  crown    dnd_extent, the second read-back, the crown base on the host, the spread reduction
  total    the whole call
dnd_ransac's rate: `pair_tests` = the sum over slices with >= min_slice_pts points of iterations x points; over the ransac
stage's time it is the point-against-circle tests per second the kernel sustains (an upper bound on the work: hypotheses
that are skipped test nothing).
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


def child(n, reps, cpu):
    from sfm_danpipeline_amd import _lib, dendro
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_dendro_cpu import STUB, load_stub, planted, result_bytes, stub_opts, stub_run
    xyz, _ = planted(31, n)
    ctx = _lib.default_context()
    out = {"n": n}
    with Cloud(xyz, ctx=ctx) as c:
        o = dendro.default_opts()
        res = dendro.measure(c, opts=o)                      # warm-up: the handle's blocks, rocPRIM's temporary storage
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            dendro.measure(c, opts=o)
            walls.append((time.perf_counter() - t0) * 1e3)
        out["call"] = round(float(np.median(walls)), 3)
        ctx.set_timing(True)
        stages = []
        for _ in range(reps):
            dendro.measure(c, opts=o)
            stages.append(dendro.last_timing(c))
        ctx.set_timing(False)
        stages.sort(key=lambda s: s["total"])
        out.update({k: round(v, 3) for k, v in stages[len(stages) // 2].items()})
        rows = dendro.profile(c, opts=o)
    out["slices"] = int(res.n_slices)
    out["pair_tests"] = int(rows["count"][rows["count"] >= o.min_slice_pts].sum()) * int(o.ransac_iters)
    out["pair_tests_per_s"] = round(out["pair_tests"] / (out["ransac"] * 1e-3), 1) if out["ransac"] > 0 else None
    out.update(dbh=res.dbh, total_height=res.total_height, crown_base_height=res.crown_base_height, flags=int(res.flags))
    if cpu:
        so = os.path.join(tempfile.mkdtemp(), "libdendrocapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
        dn = load_stub(so)
        t0 = time.perf_counter()
        sres, srows, _ = stub_run(dn, xyz, opts=stub_opts(dn), threads=16)
        out["cpu_stub_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["equal_to_stub"] = bool(result_bytes(sres) == result_bytes(res) and srows.tobytes() == rows.tobytes())
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
