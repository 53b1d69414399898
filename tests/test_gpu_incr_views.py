"""GPU: the incremental loop of the C++ host mirror (csrc/host/SfmIncremental.cpp: addMoreViews, findCameraPosePNP over
sfmhip_pnp_ransac) through sfm_incr_selftest: (a) a synthetic ring of 8 cameras with exact correspondences handed in through
the mirror's setters, against ground truth up to the gauge of the base pair; (b) the ten temple frames end to end,
structure only.  (tests/test_gpu_incremental.py holds the tests of the incremental kernels; this file is the loop's.)"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import build, pose

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TEMPLE = os.path.join(HERE, "golden", "temple")

# (a) measured worst case over the 8 cameras after similarity alignment, recorded in DESIGN f-7; asserted at 10 x
RING_ANGLE_WORST, RING_CENTRE_WORST = 6.03e-8, 5.59e-8
RING_ANGLE_BOUND, RING_CENTRE_BOUND = 10 * RING_ANGLE_WORST, 10 * RING_CENTRE_WORST


@pytest.fixture(scope="module")
def exe():
    return build.build_incr_demo()


def _read_out(path):
    b = open(path, "rb").read()
    n_img, bq, bt = struct.unpack_from("<iii", b, 0)
    if bq < 0:
        return dict(n_img=n_img, base=None)
    o = 12
    (base_cloud,) = struct.unpack_from("<i", b, o)
    o += 4
    P = np.frombuffer(b, np.float64, 12 * n_img, o).reshape(n_img, 3, 4).copy()
    o += 96 * n_img
    K = np.frombuffer(b, np.float64, 9, o).reshape(3, 3).copy()
    o += 72
    sets = []
    for _ in range(2):
        (n,) = struct.unpack_from("<i", b, o)
        sets.append(set(struct.unpack_from(f"<{n}i", b, o + 4)))
        o += 4 + 4 * n
    (nc,) = struct.unpack_from("<i", b, o)
    o += 4
    xyz, tracks = np.zeros((nc, 3)), []
    for i in range(nc):
        xyz[i] = struct.unpack_from("<3d", b, o)
        (nt,) = struct.unpack_from("<i", b, o + 24)
        tr = struct.unpack_from(f"<{2 * nt}i", b, o + 28)
        tracks.append([(tr[2 * k], tr[2 * k + 1]) for k in range(nt)])
        o += 28 + 8 * nt
    assert o == len(b)
    return dict(n_img=n_img, base=(bq, bt), base_cloud=base_cloud, P=P, K=K, done=sets[0], good=sets[1], xyz=xyz, tracks=tracks)


def _look_at(c):
    z = -c / np.linalg.norm(c)
    x = np.cross([0.0, 1.0, 0.1], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ c


def _ring_scene(path, n_views=8, n_points=1600, seed=3):
    """cameras on an arc of radius 6 looking at the origin, a cloud in [-1, 1]^3; point j is seen by three consecutive
    views, so every view brings points the cloud does not have yet.  Features are listed per image in a shuffled order."""
    g = np.random.default_rng(seed)
    K = np.array([[800.0, 0, 320.0], [0, 800.0, 240.0], [0, 0, 1]])      # (one focal: the bundle adjustment has one)
    poses = []
    for v in range(n_views):
        a = np.deg2rad(-42 + 12 * v)
        c = np.array([6 * np.sin(a), 0.4 * np.cos(3 * a), -6 * np.cos(a)])
        poses.append(_look_at(c))
    X = g.uniform(-1, 1, (n_points, 3))
    first = np.arange(n_points) % (n_views + 2) - 2                       # first view of the point's window of three
    feats, index = [], []
    for v in range(n_views):
        ids = np.flatnonzero((first <= v) & (v <= first + 2))
        ids = ids[g.permutation(len(ids))]
        R, t = poses[v]
        Xc = X[ids] @ R.T + t
        feats.append(np.stack([800 * Xc[:, 0] / Xc[:, 2] + 320, 800 * Xc[:, 1] / Xc[:, 2] + 240], 1))
        index.append({int(p): k for k, p in enumerate(ids)})
    pairs = []
    for q in range(n_views):
        for t_ in range(q + 1, n_views):
            common = sorted(set(index[q]) & set(index[t_]), key=lambda p: index[q][p])
            pairs.append((q, t_, [(index[q][p], index[t_][p]) for p in common]))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", n_views) + K.tobytes() + np.zeros(5).tobytes())
        for xy in feats:
            f.write(struct.pack("<i", len(xy)) + np.ascontiguousarray(xy).tobytes())
        f.write(struct.pack("<i", len(pairs)))
        for q, t_, m in pairs:
            f.write(struct.pack("<iii", q, t_, len(m)) + np.asarray(m, np.int32).reshape(-1, 2).tobytes())
    return poses, X


def _similarity(A, B):
    """s, R, t with s R A_i + t ~ B_i (Umeyama)"""
    ma, mb = A.mean(0), B.mean(0)
    U, D, Vt = np.linalg.svd((B - mb).T @ (A - ma) / len(A))
    S = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / ((A - ma) ** 2).sum(1).mean()
    return s, R, mb - s * R @ ma


def _angle(Ra, Rb):
    E = Ra @ Rb.T
    s = 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.arctan2(s, 0.5 * (np.trace(E) - 1)))


def _ba_costs(stdout):
    return [(float(a), float(b)) for a, b in re.findall(r"Bundle adjustment: iterations \d+, cost (\S+) -> (\S+),", stdout)]


def test_ring_of_eight_cameras_registers_every_view(exe, tmp_path):
    """Measured worst case over the 8 cameras after similarity alignment of the camera centres: rotation 6.03e-8 rad, centre
    5.59e-8 of the ring's radius (exact correspondences; what is left is where the bundle adjustment stops); the assertion is
    10 x that: 6.03e-7 rad and 5.59e-7."""
    scene, out = str(tmp_path / "ring.bin"), str(tmp_path / "ring.out")
    poses, _ = _ring_scene(scene)
    r = subprocess.run([exe, "--scene", scene, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    o = _read_out(out)
    assert o["base"] is not None and o["done"] == set(range(8)) and o["good"] == set(range(8))
    # poses against ground truth up to the gauge of the base pair
    C_est = np.stack([-o["P"][v][:, :3].T @ o["P"][v][:, 3] for v in range(8)])
    C_gt = np.stack([-R.T @ t for R, t in poses])
    s, Rg, tg = _similarity(C_est, C_gt)
    worst_a = max(_angle(o["P"][v][:, :3] @ Rg.T, poses[v][0]) for v in range(8))
    worst_c = float(np.max(np.linalg.norm((s * C_est @ Rg.T + tg) - C_gt, axis=1)) / 6.0)
    print(f"MEASURE ring angle {worst_a:.3e} centre {worst_c:.3e}")
    assert worst_a <= RING_ANGLE_BOUND and worst_c <= RING_CENTRE_BOUND
    # the cloud grows with every view
    after = {}
    view = None
    for line in r.stdout.splitlines():
        m = re.match(r"Possible view: image --> (\d+)", line)
        if m:
            view = int(m.group(1))
        m = re.match(r"After triangulation: (\d+)", line)
        if m and view is not None:
            after[view] = int(m.group(1))
    assert len(after) == 6
    sizes = [o["base_cloud"]] + list(after.values())              # (dict order = the order the views were added in)
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    assert len(o["xyz"]) == sizes[-1]
    # bundle adjustment never raises its cost
    costs = _ba_costs(r.stdout)
    assert len(costs) == 6 and all(b <= a for a, b in costs), costs


def test_temple_frames_end_to_end(exe, tmp_path):
    """structure only: there is nothing here to measure the temple reconstruction against"""
    out = str(tmp_path / "temple.out")
    r = subprocess.run([exe, "--images", TEMPLE, os.path.join(TEMPLE, "camera_calibration_template.xml"), out],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    o = _read_out(out)
    assert o["n_img"] == 10 and o["base"] is not None
    assert set(o["base"]) <= o["good"] <= o["done"] <= set(range(10))
    for v in o["good"]:
        P = o["P"][v]
        assert np.linalg.norm(P[:, 3]) <= 200 and pose.check_coherent_rotation(P[:, :3]), v
    assert len(o["xyz"]) >= o["base_cloud"] > 0
    # measured values for DESIGN f-7 (no threshold on them)
    print(f"MEASURE temple registered {len(o['good'])} of 10, done {len(o['done'])}, cloud {o['base_cloud']} -> {len(o['xyz'])}")
    costs = _ba_costs(r.stdout)
    n_obs = sum(len(t) for t in o["tracks"])
    if costs:   # the last bundle adjustment's final cost is half the sum of squared residuals over every observation
        print(f"MEASURE temple reprojection RMS {np.sqrt(2 * costs[-1][1] / n_obs):.4f} px over {n_obs} observations")
