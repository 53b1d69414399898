"""Host-clock time of the crown delineation on the GPU (sfmhip_cloud_crowns, crowns.py) on the planted plots of
scripts/gpu_terrain_time.py (trees 8 apart on an undulating square whose side grows with the square root of the point count:
24 m at 10^5 points, 240 m at 10^7), on the canopy raster a terrain call with cells of 0.5 and 0.1 m leaves on the handle, with
the default crown options.  Prints one JSON line and, with --out, writes it to a file: per size and cell, the call's wall time
without stage timing (the median of --reps warm calls), the stages of one call as the library clocks them under
sfmhip_set_timing (of --reps calls, the one with the median total), the raster, the canopy cells, the summits and their share
of the cells, the doubling rounds of the ascent and of the parents, the trees found; beside them, for proportion, the wall time
of sfmhip_cloud_terrain on the same cloud and of sfmhip_cloud_trees on its normalised cloud.  Every run is first checked byte
for byte against the g++ build of the same header (the test stubs of the terrain and of the crowns, one thread).

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of time
ends the script: nothing more is started on the GPU after it.

  stage    what it covers
  smooth   crn_smooth, one launch per pass
  ascent   crn_up, crn_jump in batches of 4 rounds with one read-back each, the scan of the summit flags, crn_compact
  windows  crn_window (a wave per summit), crn_pjump in batches, the scan of the top flags, crn_tops
  labels   crn_labels
  points   crn_points, crn_area, tree_of, the rows and the counts back on the host
  total    the whole call
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

CELLS = (0.5, 0.1)


def stub(path, name):
    so = os.path.join(tempfile.mkdtemp(), name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, path])
    return so


def child(n, reps):
    from scripts.gpu_terrain_time import plot
    from sfm_danpipeline_amd import _lib, crowns, terrain, trees
    from sfm_danpipeline_amd.cloud import Cloud
    from tests import test_crowns_cpu as tc, test_terrain_cpu as tt
    xyz, planted_trees, side = plot(n)
    ctx = _lib.default_context()
    out = {"n": len(xyz), "side_m": round(float(side), 1), "trees_planted": planted_trees, "cells": []}
    cn, tn = tc.load_stub(stub(tc.STUB, "libcrownscapi.so")), tt.load_stub(stub(tt.STUB, "libterraincapi.so"))
    with Cloud(xyz, ctx=ctx) as c:
        for cell in CELLS:
            topt = terrain.default_opts(cell=cell)
            terrain.terrain(c, opts=topt)                        # warm-up
            t0 = time.perf_counter()
            terrain.terrain(c, opts=topt)
            row = {"cell": cell, "terrain_call": round((time.perf_counter() - t0) * 1e3, 3)}
            o = crowns.default_opts()
            tree_of, tops, res = crowns.crowns(c, o)             # warm-up: the handle's blocks
            smooth, labels = crowns.raster(c)
            t0 = time.perf_counter()
            want = tc.stub_cloud_run(cn, tt.stub_run(tn, xyz, opts=tt.stub_opts(tn, cell=cell)), tc.stub_opts(cn))
            row["cpu_stubs_1_thread"] = round((time.perf_counter() - t0) * 1e3, 3)
            got = dict(labels=labels, smooth=smooth, tree_of=tree_of, tops=tops, res=res)
            row["equal_to_stub"] = bool(tc.same_run(got, want, tc.ARRAYS + ("tree_of",)))
            if not row["equal_to_stub"]:
                print("the device and the stub differ at", n, cell, file=sys.stderr)
                sys.exit(1)
            walls = []
            for _ in range(reps):
                t0 = time.perf_counter()
                crowns.crowns(c, o)
                walls.append((time.perf_counter() - t0) * 1e3)
            row["call"] = round(float(np.median(walls)), 3)
            ctx.set_timing(True)
            stages = []
            for _ in range(reps):
                crowns.crowns(c, o)
                stages.append(crowns.last_timing(c))
            ctx.set_timing(False)
            stages.sort(key=lambda s: s["total"])
            row.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in stages[len(stages) // 2].items()})
            ncell = int(res.De) * int(res.Dn)
            row.update(De=int(res.De), Dn=int(res.Dn), n_canopy=int(res.n_canopy), n_summits=int(res.n_summits),
                       summit_share_of_cells=round(res.n_summits / max(ncell, 1), 5), n_trees=int(res.n_trees), max_depth=int(res.max_depth),
                       n_labelled_cells=int(res.n_labelled_cells), n_labelled=int(res.n_labelled), flags=int(res.flags))
            with terrain.normalize(c) as nc:
                sopts = trees.default_opts(ground=0.0, stem_cell=0.1)
                try:
                    trees.trees(nc, opts=sopts)                  # warm-up
                    t0 = time.perf_counter()
                    sres = trees.trees(nc, opts=sopts)[2]
                    row["trees_call_on_normalised"] = round((time.perf_counter() - t0) * 1e3, 3)
                    row["stems_found"] = int(sres.n_trees)
                except _lib.SfmHipError as e:                    # (a grid cap of f-13 on the largest plot)
                    row["trees_call_on_normalised"], row["trees_error"] = None, str(e)[:80]
            out["cells"].append(row)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return 0
    result = {"device": "MI355X", "run": "python scripts/gpu_crowns_time.py --out profiles/crowns_time_mi355x.json", "reps": a.reps, "sizes": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"size {n} ran out of time", file=sys.stderr)
            return 1
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
