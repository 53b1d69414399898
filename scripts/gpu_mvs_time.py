"""Host-clock time of the dense multi-view stereo on the GPU (sfmhip_mvs_run, mvs.py) at the size the pipeline runs it:
10 views of 640 x 480 at level 1, 128 planes, 4 sources, on the sphere-and-plane scene of tests/test_mvs_cpu.py.
Prints one JSON line and, with --out, writes it to a file: the stages of one call as the library clocks them under
sfmhip_set_timing (of --reps calls after a warm-up, the call with the median total), the warped samples per second of
the sweep, and beside them the g++ build of the same header (the test stub) on 16 threads.

  stage       what it covers
  depthmaps   per view: homographies on the host, their upload, the sweep kernel
  fusion      flag, scan, emit, download of the points
  total       the whole sfmhip_mvs_run call
The sweep kernel warps (16 + 2w)^2 samples per 16 x 16 tile, plane and source (two f64 divisions and four byte gathers
each) and moves, per tile, plane and source, about (16 + 2w)^2 (2 + 2 (2w+1) 16 / (16 + 2w)) u16 and 4 (16 + 2w) 16 (1 +
(2w+1) 16 / (16 + 2w)) u32 words through LDS; `samples_per_s` is the first count over the depth-map time.

What the LDS traffic allows (`lds_cycles_per_round`, `lds_bound_samples_per_s`): per tile, plane and source the workgroup
issues, as wave64 instructions, T²/64 u16 stores of samples (4 cycles each), 2 (2w+1) 16 T / 64 u16 loads and 4 · 16 T / 64
stores for the row sums, and 4 (2w+1) 256 / 64 loads for the column sums (a load 2 cycles, a store 4, no bank conflict
counted), T = 16 + 2w.  T² samples per that many cycles, on every CU at the device's clock, is the bound.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_clock():
    """(compute units, clock in Hz) of device 0; the MI355X's 256 and 2.4 GHz where torch cannot say"""
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return int(p.multi_processor_count), float(p.clock_rate) * 1e3
    except Exception:
        return 256, 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (load torch's ROCm runtime first, as bench.py does)
    except ImportError:
        pass
    from scripts.gpu_poisson_time import device_name
    from sfm_danpipeline_amd import _lib, mvs
    from tests.test_mvs_cpu import StubMvs, build_stub, opts, timing_scene
    ctx = _lib.default_context()
    ctx.set_timing(True)
    gray, K, P = timing_scene()
    o = mvs.default_opts()
    out = {"device": device_name(), "views": len(gray), "rows": gray.shape[1], "cols": gray.shape[2], "level": 1,
           "n_planes": o.n_planes, "n_src": o.n_src, "window": o.window, "reps": a.reps}
    with mvs.Mvs(gray, K, P, level=1, ctx=ctx) as M:
        pts = M.run(1.2, 4.0, o)                                                  # warm-up: code objects
        runs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pts = M.run(1.2, 4.0, o)
            runs.append(dict(M.last_timing(), call=(time.perf_counter() - t0) * 1e3))
        mid = sorted(runs, key=lambda r: r["total"])[len(runs) // 2]              # one call's figures, so that the stages add up
        for key in ("depthmaps", "fusion", "total", "call"):
            out[key] = round(float(mid[key]), 3)
        t = 16 + 2 * o.window
        tiles = -(-M.rows // 16) * -(-M.cols // 16)
        out["points"] = len(pts[0])
        out["samples"] = len(gray) * tiles * o.n_planes * o.n_src * t * t
        out["samples_per_s"] = round(out["samples"] / (out["depthmaps"] * 1e-3), 0)
        w2 = 2 * o.window + 1
        out["lds_cycles_per_round"] = round(4 * t * t / 64 + 2 * (2 * w2 * 16 * t) / 64 + 4 * (4 * 16 * t) / 64 + 2 * (4 * w2 * 256) / 64, 1)
        cus, hz = device_clock()
        out["cus"], out["clock_mhz"] = cus, round(hz / 1e6)
        out["lds_bound_samples_per_s"] = round(t * t / out["lds_cycles_per_round"] * cus * hz, 0)
        out["lds_bound_fraction"] = round(out["samples_per_s"] / out["lds_bound_samples_per_s"], 4)
    if not a.no_cpu:
        ms = build_stub(os.path.join(tempfile.mkdtemp(), "libmvscapi.so"))
        with StubMvs(ms, gray, K, P, None, 1) as H:
            t0 = time.perf_counter()
            ref = H.run(1.2, 4.0, opts(ms))
            out["cpu_stub_16_threads"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["equal_to_stub"] = bool(all(x.tobytes() == y.tobytes() for x, y in zip(pts, ref)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
