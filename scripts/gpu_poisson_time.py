"""Host-clock time of the Poisson surface reconstruction on the GPU (sfmhip_cloud_poisson, poisson.py) at depth 7 on
surface_cloud of tests/test_cloud_cpu.py (a sphere, a plane, a wavy sheet, 5 % outliers) at 200 k and 1 M points, with
the normals of sfmhip_cloud_normals flipped as create_mesh flips them.  Prints one JSON line and, with --out, writes it
to a file: per size, the stages of one call as the library clocks them (of --reps calls after a warm-up, the call with
the median total), the CG iteration count, and beside them the g++ build of the same header (the test stub) on 16 threads.

Every size runs in a child process of its own under a time limit (--limit seconds); a child that fails or runs out of
time ends the script: nothing more is started on the GPU after it.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python scripts/gpu_poisson_time.py --child 200000 --no-cpu --reps 1`
in a run of its own, then `--kernel-stats DIR/.../kt_kernel_stats.csv` on the timing run: the psn_* rows of that table go
into the result as `kernel_trace` (calls, total and average time, share of the file's kernel time, and psn_apply's bytes
over its time).  Without --kernel-stats a `kernel_trace` block that the --out file already holds is kept.  The result
records the flags (depth, reps) and the device's name as the runtime gives it.

  stage        what it covers
  splat        upload of the normals, the samples' box, cell sort, V / W gather, right-hand side
  solve        conjugate gradients (4 launches per step, the record read every 32 steps)
  extraction   iso-value, classify / scan / emit, download of the mesh
  total        the whole sfmhip_cloud_poisson call
The stencil kernel (psn_apply) reads r, p and point_weight W and writes p and q once per step: 5 N^3 f64 = 84 MB at depth
7; psn_update reads chi, r, p, q and writes chi, r: 6 N^3 f64 = 101 MB.  The six vectors (101 MB) fit the 256 MiB last-level
cache, so the rate these give is a cache rate, not an HBM rate; `bytes_per_step` is printed for the division.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs)"
    except Exception:  # (no torch, or none with a device: the name is not known, the timing is still valid)
        return "unknown"


def kernel_trace(path, depth):
    """the psn_* rows of rocprofv3's kernel statistics table (Name, Calls, TotalDurationNs, AverageNs)"""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"].split("(")[0].strip()
            if name.startswith("psn_"):
                rows[name] = {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                              "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    whole = sum(v["total_ms"] for v in rows.values())
    for v in rows.values():
        v["share_of_psn_kernels_pct"] = round(100.0 * v["total_ms"] / whole, 1) if whole > 0 else 0.0
    out = {"source": "rocprofv3 --kernel-trace --stats, " + os.path.basename(path), "kernels": rows}
    if "psn_apply" in rows and rows["psn_apply"]["avg_us"] > 0:
        out["psn_apply_bytes_over_time_TBps"] = round(5 * 8 * (1 << depth) ** 3 / (rows["psn_apply"]["avg_us"] * 1e-6) / 1e12, 3)
    return out


def child(n, depth, reps, no_cpu):
    try:
        import torch  # noqa: F401  (load torch's ROCm runtime first, as bench.py does)
    except ImportError:
        pass
    from sfm_danpipeline_amd import _lib, cloud, poisson
    from tests.test_cloud_cpu import surface_cloud
    from tests.test_poisson_cpu import STUB, cg_cap, load_stub, stub_reconstruct
    ctx = _lib.default_context()
    xyz = surface_cloud(n, 21)
    out = {"n": n, "depth": depth, "reps": reps, "device": device_name()}
    opts = dict(depth=depth, cg_max_iter=cg_cap(depth))
    with cloud.Cloud(xyz, ctx=ctx) as c:
        nrm = c.normals()
        nrm[:, :3] *= -1.0
        v, t, s = poisson.reconstruct(c, nrm, poisson.default_opts(**opts))      # warm-up: code objects
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            v, t, s = poisson.reconstruct(c, nrm, poisson.default_opts(**opts))
            runs.append(dict(poisson.last_timing(c), call=(time.perf_counter() - t0) * 1e3))
        mid = sorted(runs, key=lambda r: r["total"])[len(runs) // 2]  # one call's figures, so that the stages add up
        for key in ("splat", "solve", "extraction", "total", "call"):
            out[key] = round(float(mid[key]), 3)
    n3 = (1 << depth) ** 3
    out.update(samples=s.n_samples, cg_iterations=s.cg_iterations, cg_relative_residual=s.cg_relative_residual,
               n_vertices=s.n_vertices, n_triangles=s.n_triangles,
               solve_ms_per_step=round(out["solve"] / max(s.cg_iterations, 1), 4),
               bytes_per_step={"psn_apply": 5 * 8 * n3, "psn_update": 6 * 8 * n3})
    if not no_cpu:
        so = os.path.join(tempfile.mkdtemp(), "libpoissoncapi.so")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
        ps = load_stub(so)
        t0 = time.perf_counter()
        ref = stub_reconstruct(ps, xyz, nrm, want_chi=False, **opts)
        out["cpu_stub_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["equal_to_stub"] = bool(v.tobytes() == ref.verts.tobytes() and t.tobytes() == ref.tris.tobytes())
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[200_000, 1_000_000])
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a size may take")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--child", type=int, help="run one size in this process")
    ap.add_argument("--kernel-stats", help="rocprofv3's *_kernel_stats.csv of a --child run, reported as kernel_trace")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.depth, a.reps, a.no_cpu)
    sizes = []
    for n in a.n:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--depth", str(a.depth), "--reps", str(a.reps)]
        r = subprocess.run(cmd + (["--no-cpu"] if a.no_cpu else []), capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit(f"size {n} failed with status {r.returncode}: nothing more is run")
        sizes.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = {"device": sizes[0]["device"] if sizes else device_name(), "depth": a.depth, "reps": a.reps, "sizes": sizes}
    if a.kernel_stats:
        res["kernel_trace"] = kernel_trace(a.kernel_stats, a.depth)
    elif a.out and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "kernel_trace" in old:
            res["kernel_trace"] = old["kernel_trace"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
