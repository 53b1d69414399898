"""Times the pose step on the 1225-pair batch (about 2000 matches per pair, each pair seeded separately):
sfmhip_essential_pose (RANSAC + recoverPose), sfmhip_recover_pose (recoverPose alone on the RANSAC's E and mask) and,
for comparison, sfmhip_score_essential (the RANSAC alone): host clock around the raw ABI call on buffers concatenated
beforehand, after a warm-up.  The pose kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/gpu_pose_time.py --reps 1` run.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (torch's ROCm runtime first, as bench.py does)
from sfm_danpipeline_amd import _lib, scoring, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1225)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
K = np.array([[1520.0, 0, 302.2], [0, 1520.0, 246.87], [0, 0, 1]])
rng = np.random.default_rng(77)
pairs = []
for p in range(args.pairs):
    sc = synth.two_view_scene(m=int(rng.integers(1800, 2200)), seed=1000 + p, K=K, outlier_frac=float(rng.uniform(0.05, 0.5)))
    pairs.append((sc["xy1"], sc["xy2"]))
ctx = _lib.Context(0)
L = _lib.lib()
# the concatenated buffers are built once: the timed region is the ABI call alone (uploads, kernels, downloads, host set-up)
n = len(pairs)
off = np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs])]).astype(np.int32)
left = np.ascontiguousarray(np.concatenate([a for a, _ in pairs]))
right = np.ascontiguousarray(np.concatenate([b for _, b in pairs]))
E, R, t = np.zeros((n, 9)), np.zeros((n, 9)), np.zeros((n, 3))
inl, ng = np.zeros(n, np.int32), np.zeros(n, np.int32)
out = np.zeros(int(off[-1]), np.uint8)
_, rmasks, _ = scoring.score_essential(pairs, K, want_mask=True, ctx=ctx)
m_in = np.ascontiguousarray(np.concatenate(rmasks))


def essential_pose():
    _lib.check(L.sfmhip_essential_pose(ctx.h, n, off.ctypes.data, left.ctypes.data, right.ctypes.data, K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                                       0.999, 1.0, E.ctypes.data, inl.ctypes.data, R.ctypes.data, t.ctypes.data, ng.ctypes.data,
                                       out.ctypes.data), "sfmhip_essential_pose")


def recover_pose():
    _lib.check(L.sfmhip_recover_pose(ctx.h, n, off.ctypes.data, left.ctypes.data, right.ctypes.data, E.ctypes.data, K[0, 0], K[0, 2],
                                     K[1, 2], 50.0, m_in.ctypes.data, R.ctypes.data, t.ctypes.data, ng.ctypes.data, out.ctypes.data),
               "sfmhip_recover_pose")


def score_essential():
    _lib.check(L.sfmhip_score_essential(ctx.h, n, off.ctypes.data, left.ctypes.data, right.ctypes.data, K[0, 0], K[1, 1], K[0, 2],
                                        K[1, 2], 0.999, 1.0, inl.ctypes.data, out.ctypes.data, None), "sfmhip_score_essential")


essential_pose()                                               # warm-up (and E for recover_pose)
recover_pose()
score_essential()
times = {"essential_pose_ms": [], "recover_pose_ms": [], "score_essential_ms": []}
for _ in range(args.reps):
    for k, f in (("essential_pose_ms", essential_pose), ("recover_pose_ms", recover_pose), ("score_essential_ms", score_essential)):
        t0 = time.perf_counter()
        f()                                                    # (each entry point ends with a stream synchronisation)
        times[k].append(time.perf_counter() - t0)
    essential_pose()                                           # (E of this batch again for the next recover_pose)
res = {"pairs": n, "matches": int(off[-1]), "reps": args.reps}
res.update({k: round(1e3 * float(np.median(v)), 3) for k, v in times.items()})
print(json.dumps(res))
