"""Host-clock time of the terrain model on the GPU (sfmhip_cloud_terrain, terrain.py) on planted plots whose ground is
z = 0.1 x + sin(x / 4) cos(y / 5): trees 8 apart on a square whose side grows with the square root of the point count (24 m
at 10^5 points, 240 m at 10^7), with cells of 0.5 and 0.1 m and otherwise the default options.  Prints one JSON line and, with
--out, writes it to a file: per size and cell, the stages of one call as the library clocks them under sfmhip_set_timing (of
--reps calls after a warm-up, the call with the median total), the call's wall time without stage timing (the median of
--reps warm calls), the raster and the windows, the time of sfmhip_cloud_terrain_normalize, beside them sfmhip_cloud_trees'
whole-call time on the normalised cloud, and the g++ build of the same header (the test stub, run_host, one thread) and
whether the two agree byte for byte.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of
time ends the script: nothing more is started on the GPU after it.

  stage    what it covers
  frame    labels upload, ter_frame, the bounds and their read-back, ter_cells, the cell sort, ter_runs, ter_z0
  windows  per window: four passes of ter_scan + ter_combine and two ter_transpose
  ground   ter_ground, ter_cellsum
  fill     ter_fill in batches of 16 with one read-back each, ter_relax, ter_cellstats
  heights  ter_hag, ter_chm, the per-point outputs and the totals back on the host
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


def plot(n, seed=5):
    """About n points: 60 % in planted trees 8 apart, the rest ground with noise 0.01 and no point within 1.5 of a stem."""
    from tests.test_dendro_cpu import planted
    rng = np.random.default_rng(seed)
    side = 24.0 * np.sqrt(n / 1e5)
    m = max(int(side // 8.0), 1)
    centres = (np.stack(np.meshgrid(np.arange(m), np.arange(m)), -1).reshape(-1, 2) + 0.5) * (side / m) - side / 2
    surface = lambda x, y: 0.1 * x + np.sin(x / 4.0) * np.cos(y / 5.0)
    n_tree = (6 * n // 10) // len(centres)
    pool = [planted(200 + k, n_tree)[0].astype(np.float64) for k in range(min(8, len(centres)))]
    parts = [pool[k % len(pool)] + np.array([cx, cy, surface(cx, cy)]) for k, (cx, cy) in enumerate(centres)]
    g = rng.uniform(-side / 2, side / 2, (n - n_tree * len(centres), 2))
    cell = np.clip(((g + side / 2) // (side / m)).astype(np.int64), 0, m - 1)
    near = centres[cell[:, 1] * m + cell[:, 0]]                  # the stem of a ground point's own square is its nearest
    g = g[np.hypot(g[:, 0] - near[:, 0], g[:, 1] - near[:, 1]) >= 1.5]
    parts.append(np.column_stack([g, surface(g[:, 0], g[:, 1]) + rng.normal(0, 0.01, len(g))]))
    xyz = np.concatenate(parts)
    return xyz[rng.permutation(len(xyz))].astype(np.float32), len(centres), side


def child(n, reps, cpu):
    from sfm_danpipeline_amd import _lib, terrain, trees
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.test_terrain_cpu import STUB, load_stub, same_run, stub_opts, stub_run
    xyz, planted_trees, side = plot(n)
    ctx = _lib.default_context()
    out = {"n": len(xyz), "side_m": round(float(side), 1), "trees_planted": planted_trees, "cells": []}
    tn = None
    if cpu:
        so = os.path.join(tempfile.mkdtemp(), "libterraincapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
        tn = load_stub(so)
    with Cloud(xyz, ctx=ctx) as c:
        for cell in CELLS:
            o = terrain.default_opts(cell=cell)
            is_ground, hag, res = terrain.terrain(c, opts=o)     # warm-up: the handle's blocks, rocPRIM's temporary storage
            walls = []
            for _ in range(reps):
                t0 = time.perf_counter()
                terrain.terrain(c, opts=o)
                walls.append((time.perf_counter() - t0) * 1e3)
            row = {"cell": cell, "call": round(float(np.median(walls)), 3)}
            ctx.set_timing(True)
            stages = []
            for _ in range(reps):
                terrain.terrain(c, opts=o)
                stages.append(terrain.last_timing(c))
            ctx.set_timing(False)
            stages.sort(key=lambda s: s["total"])
            row.update({k: round(v, 3) for k, v in stages[len(stages) // 2].items()})
            row.update(De=int(res.De), Dn=int(res.Dn), n_windows=int(res.n_windows), n_ground=int(res.n_ground), n_kind1=int(res.n_kind1),
                       n_kind2=int(res.n_kind2), n_kind0=int(res.n_kind0), fill_rounds=int(res.fill_rounds), flags=int(res.flags))
            t0 = time.perf_counter()
            nc = terrain.normalize(c)
            row["normalize"] = round((time.perf_counter() - t0) * 1e3, 3)
            with nc:
                topts = trees.default_opts(ground=0.0, stem_cell=0.1)
                try:
                    trees.trees(nc, opts=topts)                  # warm-up
                    t0 = time.perf_counter()
                    tres = trees.trees(nc, opts=topts)[2]
                    row["trees_call_on_normalised"] = round((time.perf_counter() - t0) * 1e3, 3)
                    row["trees_found"] = int(tres.n_trees)
                except _lib.SfmHipError as e:                    # (a grid cap of f-13 on the largest plot)
                    row["trees_call_on_normalised"], row["trees_error"] = None, str(e)[:80]
                norm = nc.download()
            if tn is not None:
                dtm, kind, chm = terrain.raster(c)
                t0 = time.perf_counter()
                want = stub_run(tn, xyz, opts=stub_opts(tn, cell=cell))
                row["cpu_stub_1_thread"] = round((time.perf_counter() - t0) * 1e3, 3)
                row["equal_to_stub"] = bool(same_run(dict(is_ground=is_ground, hag=hag, norm=norm, dtm=dtm, kind=kind, chm=chm, res=res), want))
            out["cells"].append(row)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300)
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
