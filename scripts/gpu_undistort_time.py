"""Time of the lens-distortion resampling on the GPU (sfmhip_image_undistort, undistort.py) at the size the
pipeline runs the dense stereo: the 10 views of 640 x 480 of tests/test_mvs_cpu.py's timing scene, gray and BGR.  Prints one
JSON line and, with --out, writes it to a file.

  map      the kernel that builds the packed map (device events under sfmhip_set_timing), once per call
  gather   the kernel that resamples every view and channel through it
  call     the whole sfmhip_image_undistort call on the host clock: uploads, both kernels, downloads
Of --reps calls after a warm-up the figures of the call with the median kernel time are reported.  `bytes` is what the
algorithm has to move (map: 9 bytes written per pixel; gather: the 8-byte map entry per pixel, every source byte once, every
destination byte once), `gb_per_s` that over the kernel time, `hbm_fraction` that against the 6.3 TB/s a streaming copy
reaches on the MI355X.  At 0.3 M pixels both kernels are a few microseconds long: the figures say how far a launch of this
size is from the memory system's rate, not what the kernel does on a large picture.

Beside them: sfmhip_mvs_run on the same scene (level 1, default options), and the creation of the handle with and without
`dist` (host clock), so that a reader sees the step's share of step 7."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12
DIST = (-0.25, 0.08, 0.002, -0.0015, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (load torch's ROCm runtime first, as bench.py does)
    except ImportError:
        pass
    from scripts.gpu_poisson_time import device_name
    from sfm_danpipeline_amd import _lib, mvs, undistort
    from tests.test_mvs_cpu import timing_scene
    from tests.test_undistort_cpu import build_stub, stub_undistort
    ctx = _lib.default_context()
    ctx.set_timing(True)
    gray, K, P = timing_scene()
    n, rows, cols = gray.shape
    px = rows * cols
    out = {"device": device_name(), "views": n, "rows": rows, "cols": cols, "dist": list(DIST), "reps": a.reps,
           "hbm_bytes_per_s": HBM_BYTES_PER_S}
    us = build_stub(os.path.join(tempfile.mkdtemp(), "libundcapi.so"))
    for name, images, ch in (("gray", gray, 1), ("bgr", np.stack([gray, 255 - gray, gray // 3], -1), 3)):
        got = undistort.undistort(images, K, DIST, ctx=ctx)                        # warm-up: code objects
        runs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = undistort.undistort(images, K, DIST, ctx=ctx)
            runs.append(dict(undistort.last_timing(ctx), call=(time.perf_counter() - t0) * 1e3))
        mid = sorted(runs, key=lambda r: r["map"] + r["gather"])[len(runs) // 2]
        bytes_map, bytes_gather = 9 * px, 8 * px + 2 * n * px * ch
        want = stub_undistort(us, images, K, DIST)
        out[name] = {"map_ms": round(mid["map"], 4), "gather_ms": round(mid["gather"], 4), "call_ms": round(mid["call"], 3),
                     "map_bytes": bytes_map, "gather_bytes": bytes_gather,
                     "map_gb_per_s": round(bytes_map / (mid["map"] * 1e-3) / 1e9, 1),
                     "gather_gb_per_s": round(bytes_gather / (mid["gather"] * 1e-3) / 1e9, 1),
                     "map_hbm_fraction": round(bytes_map / (mid["map"] * 1e-3) / HBM_BYTES_PER_S, 4),
                     "gather_hbm_fraction": round(bytes_gather / (mid["gather"] * 1e-3) / HBM_BYTES_PER_S, 4),
                     "valid_pixels": int(got[1].sum()),
                     "equal_to_stub": bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes())}
    o = mvs.default_opts()
    for name, dist in (("create_ms", None), ("create_distorted_ms", DIST)):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            M = mvs.Mvs(gray, K, P, level=1, ctx=ctx, dist=dist)
            times.append((time.perf_counter() - t0) * 1e3)
            if _ < 2:
                M.close()
        out[name] = round(sorted(times)[1], 3)
        M.run(1.2, 4.0, o)                                                        # warm-up
        runs = []
        for _ in range(3):
            M.run(1.2, 4.0, o)
            runs.append(M.last_timing()["total"])
        out["mvs_run_ms" if dist is None else "mvs_run_distorted_ms"] = round(sorted(runs)[1], 3)
        M.close()
    out["undistort_share_of_step7"] = round((out["create_distorted_ms"] - out["create_ms"]) / (out["create_distorted_ms"] + out["mvs_run_distorted_ms"]), 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
