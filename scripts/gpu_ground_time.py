"""Host-clock time of the ground-plane call on the GPU (sfmhip_cloud_ground_plane, ground.py) on the planted tree on its
ground disc of tests/test_ground_cpu.py, rotated, at 200 k and 1 M points and 512 iterations.  Prints one JSON line and, with
--out, writes it to a file: per size, the stages of one call as the library clocks them under sfmhip_set_timing (of --reps
calls after a warm-up, the call with the median total), the call's wall time without stage timing, and beside them the g++
build of the same header (the test stub, run_host) on 16 threads and whether the two agree bit for bit.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of
time ends the script: nothing more is started on the GPU after it.

  stage    what it covers
  select   labels upload, gnd_flag, the bounding box, the scan and its read-back, gnd_emit, gnd_hyp
  score    gnd_score (iterations x selected points)
  refit    gnd_pick, gnd_refit per round and once more for the final counts, the read-back, the frame on the host
  total    the whole call
gnd_score's rate: `plane_tests` = iterations x selected points; over the score stage's time it is the point-against-plane
tests per second the kernel sustains (an upper bound on the work: hypotheses that are skipped test nothing).
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
    from sfm_danpipeline_amd import _lib, ground
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_ground_cpu import STUB, load_stub, result_bytes, scene, stub_opts, stub_run
    xyz = scene(31, n // 2, n - n // 2, rot=31)[0]
    ctx = _lib.default_context()
    out = {"n": n}
    with Cloud(xyz, ctx=ctx) as c:
        o = ground.default_opts()
        res = ground.ground_plane(c, opts=o)                 # warm-up: the handle's blocks, rocPRIM's temporary storage
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ground.ground_plane(c, opts=o)
            walls.append((time.perf_counter() - t0) * 1e3)
        out["call"] = round(float(np.median(walls)), 3)
        ctx.set_timing(True)
        stages = []
        for _ in range(reps):
            ground.ground_plane(c, opts=o)
            stages.append(ground.last_timing(c))
        ctx.set_timing(False)
        stages.sort(key=lambda s: s["total"])
        out.update({k: round(v, 3) for k, v in stages[len(stages) // 2].items()})
    out["iterations"] = int(o.ransac_iters)
    out["plane_tests"] = int(res.n_selected) * int(o.ransac_iters)
    out["plane_tests_per_s"] = round(out["plane_tests"] / (out["score"] * 1e-3), 1) if out["score"] > 0 else None
    out.update(inliers=int(res.inliers), below=int(res.below), winner=int(res.winner), rms=res.rms, tol=res.tol, flags=int(res.flags))
    if cpu:
        so = os.path.join(tempfile.mkdtemp(), "libgroundcapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
        gn = load_stub(so)
        t0 = time.perf_counter()
        sres = stub_run(gn, xyz, opts=stub_opts(gn), threads=16)
        out["cpu_stub_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["equal_to_stub"] = bool(result_bytes(sres) == result_bytes(res))
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
