"""Host-clock time of the coarse plot alignment on the GPU (sfmhip_cloud_align_vote, sfmhip_cloud_register_batch,
sfmhip_cloud_align).  Prints one JSON line and, with --out, writes it to a file.  Two scenes, each a target and
every third of its points (with 1 cm of noise, where the target's x < 2) moved by the inverse of a yaw of 137 degrees, a shift
of (11, -7) and scale 2.3: the 8 500-point planted plot of tests/test_register_cpu.py and a 200 000-point plot.  Per scene, with
the default options (15 scales x 72 yaws, 2 048 samples a side, 64 x 64 bins, 64 candidates), h_tol 0.3, scales 1.5 .. 3.5:

  vote                 sfmhip_cloud_align_vote: the two sides' samples, the vote kernel, the candidates (the library's own
                       clock, the median of --reps warm calls); vote_pairs the pair tests of the kernel
  batch_icp_64         sfmhip_cloud_register_batch from the 64 candidates on the source's sample against the whole target
                       (the median wall time of --reps warm calls); batch_iterations those of its longest problem
  sequential_icp_64    the same 64 starts through 64 sfmhip_cloud_register calls, one after the other: the only way before
  align                the whole sfmhip_cloud_align call (vote, select, batch, winner), the library's clock
  winner               scale and yaw error against the planted motion, pairs, how many candidates reached the same transform

The measurement runs in a child process under a time limit (--limit seconds); a child that fails or runs out of time ends the
script: nothing more is started on the GPU after it."""
import argparse
import json
import math
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


def child(reps):
    from sfm_danpipeline_amd import _lib, register
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_align_cpu import LEVEL, np_sample, yaw_motion
    from tests.test_register_cpu import CENTRES, motion_errors, moved_back, planted_plot
    from tests.test_trees_cpu import plot
    ctx = _lib.default_context()
    M = yaw_motion(137.0, 2.3)
    out = {"scenes": []}
    for name, tgt in (("planted_plot", planted_plot()), ("plot_200k", plot(2, CENTRES, n_tree=40000, n_ground=80000)[0])):
        keep = np.arange(0, len(tgt), 3)
        keep = keep[tgt[keep, 0] < 2]
        src = moved_back(tgt[keep].astype(np.float64) + np.random.default_rng(7).normal(size=(len(keep), 3)) * 0.01, M)
        o = register.align_default_opts(scale_lo=1.5, scale_hi=3.5, h_tol=0.3)
        row = {"scene": name, "n_target": len(tgt), "n_source": len(src)}
        with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
            cands, st = register.align_vote(tc, sc, LEVEL, LEVEL, opts=o)        # warm-up (and the k-NN grid below)
            votes = []
            for _ in range(reps):
                register.align_vote(tc, sc, LEVEL, LEVEL, opts=o)
                votes.append(register.align_last_timing(tc)["vote"])
            row.update(vote=round(float(np.median(votes)), 3), vote_pairs=int(o.n_scale) * int(o.n_yaw) * st.n_src * st.n_tgt,
                       samples=[st.n_src, st.n_tgt], candidates=len(cands), bin_width=st.w)
            sel = src[np_sample(src, LEVEL, o.clear_rel, o.src_samples)[3]]      # rule V3's sample, as entry 3 gathers it
            kw = dict(with_scale=1, max_iters=int(o.icp_max_iters), max_dist=o.icp_dist_bins * st.w)
            inits = [c.T for c in cands]
            with Cloud(sel, ctx=ctx) as ss:
                batch = register.icp_batch(tc, ss, inits, **kw)                  # warm-up
                singles = [register.icp(tc, ss, T, **kw) for T in inits]
                row["batch_equals_sequential"] = all(bytes(memoryview(a)) == bytes(memoryview(b)) for a, b in zip(batch, singles))
                row["batch_icp_64"] = median_call(lambda: register.icp_batch(tc, ss, inits, **kw), reps)
                row["batch_iterations"] = register.batch_last_timing(tc)["iterations"]
                row["sequential_icp_64"] = median_call(lambda: [register.icp(tc, ss, T, **kw) for T in inits], reps)
                row["sequential_iterations_sum"] = int(sum(r.iterations for r in singles))
            totals = []
            for _ in range(reps):
                res = register.align(tc, sc, LEVEL, LEVEL, opts=o)
                totals.append(register.align_last_timing(tc))
            totals.sort(key=lambda t: t["total"])
            row["align"] = {k: round(v, 3) for k, v in totals[len(totals) // 2].items()}
            es, ea, et = motion_errors(res.reg.T, M)
            row["winner"] = dict(flags=res.flags, candidate=res.cand_index, same=res.n_same, pairs=res.reg.pairs, of=st.n_src, scale_error=es,
                                 angle_error_deg=ea, t_error=et, scale_guess=register.scale_guess(st))
        out["scenes"].append(row)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        return 1                                                 # nothing more on the GPU after a failure
    result = dict(device="MI355X", reps=a.reps, **json.loads(line[0][7:]))
    assert all(math.isfinite(s["vote"]) for s in result["scenes"])
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
