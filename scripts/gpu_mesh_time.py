"""Host-clock time of the mesh finishing on the GPU (sfmhip_cloud_mesh_finish) on the depth-7 Poisson mesh of
surface_cloud(1_000_000, 21), built as tests/test_gpu_poisson.py builds it (the normals of sfmhip_cloud_normals flipped, a few
rows spoilt), with r = 1.5 cells of the Poisson cube, min_support 1 and random colours.  Prints one JSON line and, with --out,
writes it to a file: the wall time of a warm call (the median of --reps calls, outputs copied to the host), the four stage
times of a warm call as the library clocks them under sfmhip_set_timing (the median call by its total) and with them the input
mesh's upload, which is the call less its three stages; beside them the yardsticks of the same job -- a warm
sfmhip_cloud_poisson call on the same handle, and the g++ build of the same header (the test stub's grid walk on 16 threads)
with whether the two agree bit for bit.  `repeat_call_allocates_bytes` is the change of the device's free memory over the
timed repeat calls (0: a repeat call on the handle allocates nothing; other processes on the device would show here too).

The work runs in a child process under a time limit (--limit seconds); a child that fails or runs out of time ends the
script: nothing more is started on the GPU after it."""
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


def child(n, depth, reps, cpu):
    import torch
    from sfm_danpipeline_amd import _lib, mesh, poisson
    from sfm_danpipeline_amd.cloud import Cloud
    from tests.mesh_scenes import ARRAYS, COUNTS, bits, build_stub, stub_finish
    from tests.test_gpu_poisson import surface_cloud
    from tests.test_poisson_cpu import cg_cap
    xyz = surface_cloud(n, 21)
    rgb = np.random.default_rng(21).integers(0, 1 << 24, len(xyz), dtype=np.uint32)
    ctx = _lib.default_context()
    row = {"points": n, "depth": depth}
    with Cloud(xyz, ctx=ctx) as c:
        nrm = c.normals()
        nrm[:, :3] *= -1.0
        nrm[::997, 0] = np.nan
        popts = poisson.default_opts(depth=depth, cg_max_iter=cg_cap(depth))
        v, t, ps = poisson.reconstruct(c, nrm, popts)
        t0 = time.perf_counter()
        poisson.reconstruct(c, nrm, popts)
        row["poisson_call"] = round((time.perf_counter() - t0) * 1e3, 3)
        r = mesh.SUPPORT_CELLS * ps.cell
        opts = mesh.default_opts(support_radius=r)
        row.update(vertices_in=len(v), triangles_in=len(t), radius=round(r, 6), upload_bytes=int(v.nbytes + t.nbytes + rgb.nbytes))
        got = mesh.finish(c, v, t, rgb, opts)                    # warm-up: the grid, the handle's blocks
        mesh.finish(c, v, t, rgb, opts)
        free0 = torch.cuda.mem_get_info()[0]
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            mesh.finish(c, v, t, rgb, opts)
            walls.append((time.perf_counter() - t0) * 1e3)
        row["finish_call"] = round(float(np.median(walls)), 3)
        ctx.set_timing(True)
        stages = []
        for _ in range(reps):
            mesh.finish(c, v, t, rgb, opts)
            stages.append(mesh.last_timing(c))
        ctx.set_timing(False)
        row["repeat_call_allocates_bytes"] = int(free0 - torch.cuda.mem_get_info()[0])
        stages.sort(key=lambda s: s["total"])
        mid = stages[len(stages) // 2]
        row["stages"] = {k: round(val, 3) for k, val in mid.items()}
        row["upload"] = round(mid["total"] - mid["search"] - mid["components"] - mid["compaction"], 3)
        s = got.summary
        row["summary"] = {k: int(getattr(s, k)) for k in COUNTS}
        row["summary"].update(area=float(s.area), volume=float(s.volume))
        row["mean_support"] = round(float(got.support.mean()), 1) if len(got.support) else 0.0
    if cpu:
        ms = build_stub(pathlib.Path(tempfile.mkdtemp()))
        t0 = time.perf_counter()
        rc, want = stub_finish(ms, xyz, rgb, v, t, r, search=2, threads=16)
        row["cpu_stub_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        row["equal_to_stub"] = bool(rc == 0 and all(np.array_equal(bits(getattr(got, k)), bits(want[k])) for k in ARRAYS) and
                                    row["summary"] == want["summary"])
    print("RESULT " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.points, a.depth, a.reps, not a.no_cpu)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--points", str(a.points), "--depth", str(a.depth), "--reps", str(a.reps)] + \
          (["--no-cpu"] if a.no_cpu else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        return 1                                                 # nothing more on the GPU after a failure
    result = {"device": "MI355X", "reps": a.reps}
    result.update(json.loads(line[0][7:]))
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
