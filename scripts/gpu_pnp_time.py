"""Where sfmhip_pnp_ransac's time goes on the GPU: 1, 8 and 64 views x 2 000 correspondences with 30 % outliers; the solver,
scoring and mask + refit kernels separately (HIP events on the context's stream, sfmhip_pnp_last_timing), the call's wall
clock, and beside them the single-thread wall clock of the CPU build of the same header (tests/stub/pnp_capi.cpp) on the
same inputs.  Reported, not gated.  Usage: python scripts/gpu_pnp_time.py [out.json]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from sfm_danpipeline_amd import _lib, pnp  # noqa: E402

K = np.array([[1520.4, 0.0, 302.32], [0.0, 1525.9, 246.87], [0.0, 0.0, 1.0]])
DIST = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])


def scene(seed, n):
    """n correspondences of a cloud in front of a camera: 0.5 px noise, 30 % of the pixels displaced by 100 to 200 px"""
    g = np.random.default_rng(seed)
    R = pnp.rodrigues(g.normal(0, 0.4, 3))
    t = np.array([0.0, 0.0, 6.0]) + g.normal(0, 0.5, 3)
    X = g.uniform(-0.6, 0.6, (n, 3))
    Xc = X @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    k1, k2, p1, p2, k3 = DIST
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xy = np.stack([(x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) * K[0, 0] + K[0, 2],
                   (y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) * K[1, 1] + K[1, 2]], 1) + g.normal(0, 0.5, (n, 2))
    idx = g.choice(n, int(0.3 * n), replace=False)
    ang, rad = g.uniform(0, 2 * np.pi, len(idx)), g.uniform(100, 200, len(idx))
    xy[idx] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    return X, xy


def cpu_twin():
    """the CPU build of csrc/pnp.h (tests/stub/pnp_capi.cpp) when the tests tree and g++ are at hand, else None"""
    try:
        from tests import pnp_scenes
        L = pnp_scenes.build_stub(tempfile.mkdtemp())
        return lambda X, xy, thr: pnp_scenes.stub_ransac(L, X, xy, K, DIST, thresholds=thr)
    except Exception as e:  # noqa: BLE001
        print(f"(no CPU twin: {e})", file=sys.stderr)
        return None


def main():
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    twin = cpu_twin()
    rows = []
    for n_views in (1, 8, 64):
        scs = [scene(9000 + v, 2000) for v in range(n_views)]
        X, xy = [s[0] for s in scs], [s[1] for s in scs]
        thr = [pnp.reference_threshold(b) for b in xy]
        pnp.pnp_ransac(X, xy, K, DIST, thresholds=thr, ctx=ctx)   # warm-up (module load, first allocations)
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            r = pnp.pnp_ransac(X, xy, K, DIST, thresholds=thr, ctx=ctx)
            wall = (time.perf_counter() - t0) * 1e3
            ms = pnp.last_timing(ctx)
            if best is None or wall < best["gpu_wall_ms"]:
                best = dict(gpu_wall_ms=wall, solver_ms=ms[0], scoring_ms=ms[1], mask_refit_ms=ms[2])
        cpu = same = None
        if twin:
            t0 = time.perf_counter()
            c = twin(X, xy, thr)
            cpu = (time.perf_counter() - t0) * 1e3
            same = bool((r["rvec"] == c["rvec"]).all() and (r["tvec"] == c["tvec"]).all())
        row = dict(views=n_views, correspondences=2000, iterations=[int(i) for i in r["iterations"]][:8],
                   cpu_stub_1thread_ms=cpu, equal_bits=same, **best)
        rows.append(row)
        print(json.dumps(row))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
