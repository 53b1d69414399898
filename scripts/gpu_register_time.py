"""Host-clock time of the cloud registration on the GPU (sfmhip_cloud_nearest, sfmhip_cloud_register) on the
planted plot of tests/test_trees_cpu.py scaled up to 10^6 target points.  Prints one JSON line and, with --out, writes it to a
file.  Per source size (10^5 and 10^6 points: target points with 1 cm of noise, moved by the inverse of a 4 degree, 0.3 motion at
scale 1.04, in random order):

  nearest_call          sfmhip_cloud_nearest under the planted motion, max_dist +inf: the median wall time of --reps warm calls
                        (search kernel, the copies of idx and d2 to the host)
  nearest_sorted_call   the same with the source uploaded in the order of the target's cells (sorted on the host by a 0.25 grid of
                        the moved points): what a cell sort of the source in front of reg_nearest could gain at best
  ckdtree_query         scipy's cKDTree.query(k=1, workers=16) of the same moved points in the same target (tree built before)
  icp_call              the whole similarity ICP from the identity, max_dist 1.0, without stage timing
  search / sums / update  ms per iteration of that call as the library clocks them under sfmhip_set_timing (a stream
                        synchronisation per stage), of the call with the median sum; iterations, pairs, converged, scale error

The measurement runs in a child process under a time limit (--limit seconds); a child that fails or runs out of time ends the
script: nothing more is started on the GPU after it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_call(f, reps):
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        walls.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(walls)), 3)


def child(n_tgt, sizes, reps):
    from scipy.spatial import cKDTree
    from sfm_danpipeline_amd import _lib, register
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_register_cpu import CENTRES, motion, moved_back
    from tests.test_trees_cpu import plot
    tgt = plot(3, CENTRES, n_tree=n_tgt // 5, n_ground=n_tgt - 3 * (n_tgt // 5))[0]
    M = motion(4.0, 0.3, 1.04)
    ctx = _lib.default_context()
    t0 = time.perf_counter()
    tree = cKDTree(tgt.astype(np.float64))
    out = {"n_target": len(tgt), "ckdtree_build": round((time.perf_counter() - t0) * 1e3, 3), "sources": []}
    with Cloud(tgt, ctx=ctx) as tc:
        t0 = time.perf_counter()
        tc.knn(1)                                                 # the k-NN grid, once per handle
        out["first_knn_call_with_grid_build"] = round((time.perf_counter() - t0) * 1e3, 3)
        for n in sizes:
            rng = np.random.default_rng(n)
            src = moved_back(tgt[rng.integers(0, len(tgt), n)].astype(np.float64) + rng.normal(size=(n, 3)) * 0.01, M)
            q = M.apply(src)
            order = np.lexsort(np.floor(q / 0.25).T[::-1].astype(np.int64))     # z-major cells, as the grid's rows run
            row = {"n_source": n}
            with Cloud(src, ctx=ctx) as sc, Cloud(src[order], ctx=ctx) as so:
                idx, d2 = register.nearest(tc, sc, M)             # warm-up
                idx_s, _ = register.nearest(tc, so, M)
                row["sorted_equals_unsorted"] = bool(np.array_equal(idx_s, idx[order]))
                row["nearest_call"] = median_call(lambda: register.nearest(tc, sc, M), reps)
                row["nearest_sorted_call"] = median_call(lambda: register.nearest(tc, so, M), reps)
                row["ckdtree_query"] = median_call(lambda: tree.query(q.astype(np.float64), k=1, workers=16), max(reps // 2, 1))
                j = tree.query(q.astype(np.float64), k=1, workers=16)[1]
                row["pairs_differing_from_ckdtree"] = int((j != idx).sum())      # (float d2 ties and near-ties)
                kw = dict(with_scale=1, max_dist=1.0)
                res = register.icp(tc, sc, **kw)
                row["icp_call"] = median_call(lambda: register.icp(tc, sc, **kw), reps)
                ctx.set_timing(True)
                stages = []
                for _ in range(reps):
                    register.icp(tc, sc, **kw)
                    stages.append(register.last_timing(tc))
                ctx.set_timing(False)
                stages.sort(key=lambda s: s["search"] + s["sums"] + s["update"])
                s = stages[len(stages) // 2]
                its = max(s["iterations"] + 1, 1)                 # (k iterations evaluate k + 1 pairings)
                row.update({k: round(s[k] / its, 4) for k in ("search", "sums", "update")})
                row.update(iterations=res.iterations, pairs=res.pairs, converged=res.converged, flags=res.flags,
                           rmse=float(np.sqrt(res.mse)), scale_error=abs(res.T.scale / 1.04 - 1))
            out["sources"].append(row)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=1000000)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.child:
        child(a.target, sizes, a.reps)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--target", str(a.target), "--sizes", a.sizes, "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        return 1                                                 # nothing more on the GPU after a failure
    result = dict(device="MI355X", reps=a.reps, **json.loads(line[0][7:]))
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
