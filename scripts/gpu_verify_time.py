"""Time of the two-view verification between the matcher and the tracks (sfmhip_matchplan_verify,
sfmhip_tracks_build_from_verified) at cfg2's size.  Prints one JSON line and, with --out, writes it to a file.

The shape: synth.sift_image_set's 50 images x 2000 SIFT-like features, all 1225 pairs in one match plan; a feature's pixel is
the projection of its bank row's world point in a ring of 50 cameras (radius 10, f = 1520, 0.3 px noise), a tenth of the
features displaced by 20 to 60 px (tests/test_gpu_verify.py's plan_scene).

  device_route   plan run -> verify_plan -> tracks.build_from_verified: the lists never visit the host
  host_route     the same plan run -> fetch -> a numpy gather of the pixel pairs -> scoring.score_essential with masks -> a
                 numpy filter by V4 / V5 -> tracks.build on the filtered lists: what a caller had to do before

Per route the wall time of --reps runs after a warm-up (median, and every run), for the device route also the stage split of
sfmhip_verified_last_timing of the median run, and whether the two routes end in the same tracks.  The whole measurement is
one child process under a time limit (--limit seconds); no profiler counters."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(reps):
    from sfm_danpipeline_amd import _lib, matcher, scoring, synth, tracks, verify
    from tests.test_gpu_verify import plan_scene
    from tests.test_tracks_cpu import K_RING
    from tests.test_verify_cpu import gather, np_filter
    ctx = _lib.default_context()
    imgs, xy_ptr, xy = plan_scene(50, 2000, 20000, seed=1234)
    nf = np.array([len(im) for im in imgs], np.int32)
    pairs = synth.all_pairs(50)
    s = matcher.ImageSet(imgs, ctx=ctx)
    s.prepare_async()
    pl = matcher.MatchPlan(s, pairs)
    keep = {}

    def device_route():
        pl.run_async(0.8)
        v = verify.verify_plan(pl, xy_ptr, xy, K_RING)
        tr = tracks.build_from_verified(v)
        keep["device"] = (v.last_timing(), {f: int(getattr(v.stats, f)) for f, _ in verify.VerifyStats._fields_},
                          {f: int(getattr(tr.stats, f)) for f, _ in tracks.TracksStats._fields_}, tr.download())
        tr.close(), v.close()

    def host_route():
        pl.run_async(0.8)
        counts, q, t, _ = pl.fetch()
        pts = gather(pairs, counts, q, t, xy_ptr, xy)
        inl, masks, _ = scoring.score_essential(pts, K_RING, want_mask=True, ctx=ctx)
        has = np.where(inl > 0, np.where(counts == 5, 2, 1), 0)
        c2, q2, t2, _ = np_filter(counts, q, t, np.concatenate(masks), has, inl, 15)
        tr = tracks.build(ctx, nf, pairs, c2, q2, t2)
        keep["host"] = ({f: int(getattr(tr.stats, f)) for f, _ in tracks.TracksStats._fields_}, tr.download())
        tr.close()

    out = {}
    for name, route in (("device_route", device_route), ("host_route", host_route)):
        route()                                                          # warm-up
        runs, stages = [], []
        for _ in range(reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            route()
            runs.append(time.perf_counter() - t0)
            stages.append(keep["device"][0] if name == "device_route" else None)
        order = np.argsort(runs)
        out[name] = {"wall_s": round(float(runs[order[len(runs) // 2]]), 6), "runs_s": [round(float(x), 6) for x in runs]}
        if name == "device_route":
            out[name]["verify_stages_s"] = {k: round(v, 6) for k, v in stages[order[len(runs) // 2]].items()}
    out["verify_stats"], out["tracks_stats"] = keep["device"][1], keep["device"][2]
    out["routes_agree"] = bool(keep["device"][2] == keep["host"][0] and all(a.tobytes() == b.tobytes() for a, b in zip(keep["device"][3], keep["host"][1])))
    raw = tracks.build_from_plan(pl)
    out["unverified_tracks_stats"] = {f: int(getattr(raw.stats, f)) for f, _ in tracks.TracksStats._fields_}
    raw.close(), pl.close(), s.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        return 1
    result = {"device": "MI355X", "shape": "50 images x 2000 features, 1225 pairs", "reps": a.reps, **json.loads(line[0][7:])}
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
