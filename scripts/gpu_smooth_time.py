"""Host-clock time of the moving-least-squares smoothing on the GPU (sfmhip_cloud_mls) on a scanned surface
(tests/mls_scenes.py: surface_cloud) of 10^5 and 10^6 points, at the radii that give about 30 and about 150 neighbours.  Prints
one JSON line and, with --out, writes it to a file.  Per size and radius: the wall time of a call at order 0 and at order 2
(the median of --reps calls after --warm warm-up rounds, outputs copied to the host), the stages of each as the library clocks them under
sfmhip_set_timing (grid: 0 once the handle has it; fit: the kernel; compaction: the scan, the gather and the copies), and the
yardsticks of the same job -- sfmhip_cloud_radius_count with cap 0 on the same handle and radius (the smoothing is two such
sweeps plus arithmetic; its wall time includes the copy of n counts), and the g++ build of the same header at order 2 (the
test stub on 16 threads) with whether the two agree bit for bit.  `fit_over_radius_count` is order 2's fit stage over
radius_count's call.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of time
ends the script: nothing more is started on the GPU after it."""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile
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


def child(n, reps, warm, cpu, neighbours):
    from sfm_danpipeline_amd import _lib
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.mls_scenes import bits, build_stub, radius_for, stub_mls, surface_cloud
    xyz = surface_cloud(n, 0, sigma=0.0005)                      # (noise well below the smaller radius at 10^6 points: a sheet, not a slab)
    ctx = _lib.default_context()
    ms = build_stub(pathlib.Path(tempfile.mkdtemp())) if cpu else None
    rows = []
    with Cloud(xyz, ctx=ctx) as c:
        for k in neighbours:
            r = radius_for(k, n, 1.0)
            row = {"n": n, "radius": round(r, 6)}
            got = c.mls(r, 2)                                    # warm-up: the grid, the handle's blocks, the clocks
            for _ in range(warm):
                c.mls(r, 0), c.mls(r, 2), c.radius_count(r)
            row["mean_neighbours"] = round(float(c.radius_count(r).mean()), 1)
            row["max_neighbours"] = got["stats"]["max_neighbours"]
            row["radius_count_call"] = median_call(lambda: c.radius_count(r), reps)
            for order in (0, 2):
                row[f"order{order}_call"] = median_call(lambda: c.mls(r, order), reps)
                ctx.set_timing(True)
                stages = []
                for _ in range(reps):
                    c.mls(r, order)
                    stages.append(c.mls_last_timing())
                ctx.set_timing(False)
                stages.sort(key=sum)
                row[f"order{order}_stages"] = dict(zip(("grid", "fit", "compaction"), (round(v, 3) for v in stages[len(stages) // 2])))
            row["fit_over_radius_count"] = round(row["order2_stages"]["fit"] / row["radius_count_call"], 2)
            if cpu:
                t0 = time.perf_counter()
                rc, want = stub_mls(ms, xyz, r, 2)
                row["cpu_stub_order2_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
                row["equal_to_stub"] = bool(rc == 0 and want["stats"] == got["stats"] and np.array_equal(want["src_index"], got["src_index"]) and
                                            np.array_equal(bits(want["xyz"]), bits(got["xyz"])) and
                                            np.array_equal(bits(want["normals"]), bits(got["normals"])))
            rows.append(row)
    print("RESULT " + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--neighbours", default="30,150")
    ap.add_argument("--limit", type=int, default=280)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.warm, not a.no_cpu, [int(k) for k in a.neighbours.split(",")])
        return 0
    result = {"device": "MI355X", "reps": a.reps, "rows": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps), "--warm", str(a.warm), "--neighbours", a.neighbours] + (["--no-cpu"] if a.no_cpu else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            return 1                                             # nothing more on the GPU after a failure
        result["rows"] += json.loads(line[0][7:])
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
