"""Time of the multi-view tracks on the GPU (sfmhip_tracks_build, sfmhip_tracks_build_from_plan, sfmhip_tracks_triangulate;
DESIGN.md f-16) at cfg2's size.  Prints one JSON line and, with --out, writes it to a file.

  host_lists   50 images x 2000 features, all 1225 pairs, about 10^6 matches made from world ids with one false match in 10^4
               (tests/test_tracks_cpu.py's generator): the build from host lists, then the triangulation of its tracks on a
               ring of 50 cameras (radius 10, f = 1520, 0.5 px noise) that see those world points
  from_plan    synth.sift_image_set's 50 x 2000 SIFT-like images through one match plan over the same pairs, then the build
               from the lists the plan left on the device

Per case: the device seconds by stage as sfmhip_tracks_last_timing reports them under sfmhip_set_timing (of --reps calls after
a warm-up, the call with the median sum), the wall time of a call without stage timing, the statistics, and for host_lists the
g++ build of the same header (tests/stub/tracks_capi.cpp, one thread) on the same machine with whether the two agree byte
for byte.  The whole measurement is one child process under a time limit (--limit seconds); no profiler counters."""
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


def median_stages(call, timing, reps):
    runs = []
    for _ in range(reps):
        call()
        runs.append(timing())
    runs.sort(key=lambda d: sum(d.values()))
    return {k: round(v, 6) for k, v in runs[len(runs) // 2].items()}


def wall(call, reps):
    w = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        w.append(time.perf_counter() - t0)
    return round(float(np.median(w)), 6)


def child(reps, cpu):
    from sfm_danpipeline_amd import _lib, matcher, synth, tracks
    from tests.test_tracks_cpu import K_RING, STAT_FIELDS, load_stub, ring_scene, stub_build, stub_triangulate, world_graph, STUB
    ctx = _lib.default_context()
    out = {}
    # ---- host lists
    nf, pairs, counts, q, t, feat_of = world_graph(7, 50, 2000, 2000, p_seen=0.7, p_match=0.83, p_false=1e-4)
    poses, dist, xy_ptr, by_world, _ = ring_scene(7, 50, 2000)
    by_world = by_world.reshape(50, 2000, 2)
    xy = by_world.copy()                                              # (a feature that is no world point keeps some pixel)
    for i in range(50):
        seen = np.flatnonzero(feat_of[i] >= 0)
        xy[i, feat_of[i, seen]] = by_world[i, seen]
    has = np.ones(50, np.uint8)
    hold = {}

    def build():
        if "h" in hold:
            hold["h"].close()
        hold["h"] = tracks.build(ctx, nf, pairs, counts, q, t)

    def tri():
        hold["tri"] = hold["h"].triangulate(poses, has, K_RING, dist, xy_ptr, xy)

    build(), tri()                                                    # warm-up: rocPRIM's temporary storage, the slab
    r = {"edges": int(q.size), **{f: int(getattr(hold["h"].stats, f)) for f in STAT_FIELDS}}
    r["build_call_s"], r["triangulate_call_s"] = wall(build, reps), wall(tri, reps)
    ctx.set_timing(True)
    r["build_stages_s"] = {k: v for k, v in median_stages(build, lambda: hold["h"].last_timing(), reps).items() if k != "triangulate"}
    r["triangulate_kernel_s"] = median_stages(tri, lambda: hold["h"].last_timing(), reps)["triangulate"]
    ctx.set_timing(False)
    ptr = hold["h"].download()[0]
    lens = np.diff(ptr)
    r["track_length_mean"], r["track_length_max"] = round(float(lens.mean()), 3), int(lens.max())
    r["points_kept"] = int(hold["tri"][3].sum())
    # the Jacobi's slab: 4 rows x 2 entries per observation x 8 B, read and written once per sweep and pair of rows at the least
    srt = np.sort(lens)
    r["slab_bytes"] = int(512 * 8 * sum(int(srt[min(64 * w + 63, srt.size - 1)]) for w in range((srt.size + 63) // 64)))
    if cpu:
        so = os.path.join(tempfile.mkdtemp(), "libtrackscapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
        tk = load_stub(so)
        t0 = time.perf_counter()
        rc, st, *arrays = stub_build(tk, nf, pairs, counts, q, t)
        r["cpu_stub_build_s"] = round(time.perf_counter() - t0, 6)
        t0 = time.perf_counter()
        ref = stub_triangulate(tk, arrays[0], arrays[1], arrays[2], poses, has, K_RING, dist, xy_ptr, xy)
        r["cpu_stub_triangulate_s"] = round(time.perf_counter() - t0, 6)
        got = hold["h"].download()
        r["equal_to_stub"] = bool(rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got, arrays)) and
                                  all(a.tobytes() == b.tobytes() for a, b in zip(hold["tri"], ref)))
    hold.pop("h").close()
    out["host_lists"] = r
    # ---- from a plan
    imgs = synth.sift_image_set(50, 2000, 128)
    s = matcher.ImageSet(imgs, ctx=ctx)
    s.prepare_async()
    pl = matcher.MatchPlan(s, synth.all_pairs(50))
    pl.run_async(0.8)
    ctx.synchronize()

    def from_plan():
        if "h" in hold:
            hold["h"].close()
        hold["h"] = tracks.build_from_plan(pl)

    from_plan()
    p = {"edges": int(hold["h"].stats.edges), **{f: int(getattr(hold["h"].stats, f)) for f in STAT_FIELDS}}
    p["build_call_s"] = wall(from_plan, reps)
    ctx.set_timing(True)
    p["build_stages_s"] = {k: v for k, v in median_stages(from_plan, lambda: hold["h"].last_timing(), reps).items() if k != "triangulate"}
    ctx.set_timing(False)
    hold.pop("h").close()
    pl.close(), s.close()
    out["from_plan"] = p
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps, not a.no_cpu)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--no-cpu"] if a.no_cpu else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        return 1
    result = {"device": "MI355X", "reps": a.reps, **json.loads(line[0][7:])}
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
