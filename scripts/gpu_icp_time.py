"""Host-clock time of the second registration entry on the GPU (sfmhip_cloud_register_icp) on the planted plot of
tests/test_trees_cpu.py at 10^5, 10^6 and 10^7 target points.  Prints one JSON line and, with --out, writes it to a file.  Per
target size the source is a tenth as many target points with 1 cm of noise, moved by the inverse of a 2 degree, 0.1 motion, in
random order; the target's normals are the cloud's own (sfmhip_cloud_normals, k = 10: `normals_call` is that call's wall time).
Per metric (0 point-to-point, 1 point-to-plane), without and with the trim (0.8), and for the trim also one-to-one:

  call                          the whole registration from the identity, max_dist 1.0, at most 10 iterations, eps 1e-6, without
                                stage timing: the median wall time of --reps warm calls
  search / rejectors / sums / update   ms per iteration of that call as the library clocks them under sfmhip_set_timing (a
                                stream synchronisation per stage), of the call with the median sum; iterations, pairs, converged,
                                flags, rmse, the angle and translation error against the planted motion

There is no earlier version to compare with: the numbers are recorded, not gated.  Every target size is measured in a child
process of its own under a time limit (--limit seconds); a child that fails or runs out of time ends the script: nothing more is
started on the GPU after it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("search", "rejectors", "sums", "update")


def median_call(f, reps):
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        walls.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(walls)), 3)


def child(n_tgt, reps):
    from sfm_danpipeline_amd import _lib, register
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_register_cpu import CENTRES, motion, motion_errors, moved_back
    from tests.test_trees_cpu import plot
    tgt = plot(3, CENTRES, n_tree=n_tgt // 5, n_ground=n_tgt - 3 * (n_tgt // 5))[0]
    M = motion(2.0, 0.1, 1.0)
    n = n_tgt // 10
    rng = np.random.default_rng(n)
    src = moved_back(tgt[rng.integers(0, len(tgt), n)].astype(np.float64) + rng.normal(size=(n, 3)) * 0.01, M)
    ctx = _lib.default_context()
    out = {"n_target": len(tgt), "n_source": n, "rows": []}
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        t0 = time.perf_counter()
        nrm = tc.normals(10)
        out["normals_call"] = round((time.perf_counter() - t0) * 1e3, 3)
        for metric in (0, 1):
            for trim, o2o in ((1.0, 0), (0.8, 0), (0.8, 1)):
                kw = dict(metric=metric, trim=trim, one_to_one=o2o, max_dist=1.0, max_iters=10, eps=1e-6, min_pairs=6 if metric else 3)
                nm = nrm if metric else None
                res = register.icp_ex(tc, sc, nm, **kw)           # warm-up
                row = dict(metric=metric, trim=trim, one_to_one=o2o, call=median_call(lambda: register.icp_ex(tc, sc, nm, **kw), reps))
                ctx.set_timing(True)
                stages = []
                for _ in range(reps):
                    register.icp_ex(tc, sc, nm, **kw)
                    stages.append(register.icp_last_timing(tc))
                ctx.set_timing(False)
                stages.sort(key=lambda s: sum(s[k] for k in STAGES))
                s = stages[len(stages) // 2]
                its = max(s["iterations"] + 1, 1)                 # (k iterations evaluate k + 1 pairings)
                row.update({k: round(s[k] / its, 4) for k in STAGES})
                _, ang, terr = motion_errors(res.T, M)
                row.update(iterations=res.iterations, pairs=res.pairs, converged=res.converged, flags=res.flags, rmse=float(np.sqrt(res.mse)),
                           angle_error_deg=ang, t_error=terr)
                out["rows"].append(row)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--out")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return 0
    result = dict(device="MI355X", reps=a.reps, targets=[])
    for n in [int(s) for s in a.targets.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"target {n}: no result within {a.limit} s", file=sys.stderr)
            return 1                                             # nothing more on the GPU after it
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            return 1                                             # nothing more on the GPU after a failure
        result["targets"].append(json.loads(line[0][7:]))
        print(json.dumps(result["targets"][-1]), flush=True)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
