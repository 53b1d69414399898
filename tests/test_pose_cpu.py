"""The pose step of baseReconstruction (csrc/pose.h: getCameraPose's recoverPose and CheckCoherentRotation, reference
src/Sfm.cpp:713-799) on the CPU, through a g++ build of the header the device kernels compile: decomposeEssentialMat
against numpy's SVD, recoverPose against an independent numpy restatement (numpy SVD, a per-point numpy DLT), the edge
cases of the selection and the thresholds, the float-narrowed rotation check, and one shape under ASan / UBSan.  The
last section runs the scenes of tests/pose_scenes.py (every candidate a winner, ties, degenerate and scaled E, mask
bytes, thresholds): what it asserts here is what tests/test_gpu_pose.py relies on when it runs them on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import synth
from tests import pose_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "pose_capi.cpp")
K = np.array([[1520.0, 0, 302.2], [0, 1490.0, 246.87], [0, 0, 1]])   # fx != fy: recoverPose takes fx for both axes
W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pose") / "libposecapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.pose_decompose.argtypes = [vp] * 4
    lib.pose_normalize.argtypes = [C.c_double] * 5 + [vp]
    lib.pose_normalize.restype = None
    lib.pose_recover.argtypes = [C.c_int, vp, vp, vp] + [C.c_double] * 4 + [vp] * 6
    lib.pose_fullpivlu_det.argtypes = [vp]
    lib.pose_fullpivlu_det.restype = C.c_double
    lib.pose_coherent_det.argtypes = [C.c_double]
    lib.pose_check_rotation.argtypes = [vp]
    return lib


def _p(a):
    return a.ctypes.data if a is not None else None


def decompose(pc, E):
    E = np.ascontiguousarray(E, np.float64)
    R1, R2, t = np.zeros(9), np.zeros(9), np.zeros(3)
    fl = pc.pose_decompose(_p(E), _p(R1), _p(R2), _p(t))
    return R1.reshape(3, 3), R2.reshape(3, 3), t, fl


def recover(pc, a, b, E, f, ppx, ppy, dist=50.0, mask=None):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    E = np.ascontiguousarray(E, np.float64)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    R, t, out = np.zeros(9), np.zeros(3), np.zeros(max(len(a), 1), np.uint8)
    ng, cnt, fl = C.c_int32(0), np.zeros(4, np.int32), C.c_int32(0)
    sel = pc.pose_recover(len(a), _p(a), _p(b), _p(E), f, ppx, ppy, dist, _p(m), _p(R), _p(t), C.byref(ng), _p(out), _p(cnt),
                          C.byref(fl))
    return dict(sel=sel, R=R.reshape(3, 3), t=t, n_good=ng.value, mask=out[:len(a)], counts=cnt, flags=fl.value)


def _essential(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


def _rot(rng, scale=0.3):
    a = rng.normal(0, scale, 3)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


# ---------------------------------------------------------------- the numpy restatement
def np_decompose(E):
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2]


def np_recover(a, b, E, f, ppx, ppy, dist=50.0, mask=None):
    """recoverPose with numpy's SVD: (sel, R, t, counts, masks (4, n), near (n,) = a point within 1e-9 of a threshold)"""
    R1, R2, t = np_decompose(E)
    x1 = (np.asarray(a) - [ppx, ppy]) / f
    x2 = (np.asarray(b) - [ppx, ppy]) / f
    n = len(x1)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    masks, near = np.zeros((4, n), bool), np.zeros(n, bool)
    for c, (R, tt) in enumerate(cands):
        P = np.hstack([R, tt[:, None]])
        P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
        A = np.stack([x1[:, :1] * P0[2] - P0[0], x1[:, 1:] * P0[2] - P0[1], x2[:, :1] * P[2] - P[0], x2[:, 1:] * P[2] - P[1]], 1)
        Q = np.linalg.svd(A)[2][:, 3, :]
        ok = Q[:, 2] * Q[:, 3] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            X = Q / Q[:, 3:4]
        ok &= X[:, 2] < dist
        z = X @ P[2]
        ok &= (z > 0) & (z < dist)
        if mask is not None:
            ok &= np.asarray(mask) != 0
        masks[c] = ok
        nq = np.linalg.norm(Q, axis=1)
        with np.errstate(invalid="ignore"):
            near |= (np.abs(Q[:, 3]) < 1e-9 * nq) | (np.abs(Q[:, 2]) < 1e-9 * nq)
            near |= (np.abs(X[:, 2]) < 1e-9) | (np.abs(X[:, 2] - dist) < 1e-9 * dist)
            near |= (np.abs(z) < 1e-9) | (np.abs(z - dist) < 1e-9 * dist)
    g = masks.sum(1)
    sel = next(c for c in range(3) if all(g[c] >= g[k] for k in range(4))) if any(
        all(g[c] >= g[k] for k in range(4)) for c in range(3)) else 3
    return sel, cands[sel][0], cands[sel][1], g, masks, near


# ---------------------------------------------------------------- decomposition
def test_decomposition_matches_numpy(pc):
    rng = np.random.default_rng(5)
    for trial in range(60):
        R, t = _rot(rng), rng.normal(0, 1, 3)
        E = _essential(R, t)
        if trial % 2:
            E = E + rng.normal(0, 1e-3, (3, 3))       # noisy: no longer rank 2
        R1, R2, tt, fl = decompose(pc, E)
        nR1, nR2, nt = np_decompose(E)
        assert fl == 0
        for Rx in (R1, R2):
            assert abs(np.linalg.det(Rx) - 1) < 1e-12
            assert min(np.abs(Rx - nR1).max(), np.abs(Rx - nR2).max()) < 1e-12, trial
        assert not np.allclose(R1, R2, atol=1e-6)
        assert min(np.abs(tt - nt).max(), np.abs(tt + nt).max()) < 1e-12, trial
        assert abs(np.linalg.norm(tt) - 1) < 1e-12


def test_zero_essential_matrix_is_flagged(pc):
    assert decompose(pc, np.zeros((3, 3)))[3] == 1     # the random-vector branch of JacobiSVDImpl_: reported, not restated


# ---------------------------------------------------------------- recoverPose
def _scene(m, seed, outliers=0.1):
    sc = synth.two_view_scene(m=m, seed=seed, K=K, noise_px=0.3, outlier_frac=outliers)
    R, t = sc["P2"][:, :3], sc["P2"][:, 3]
    return sc["xy1"], sc["xy2"], _essential(R, t), R, t / np.linalg.norm(t)


@pytest.mark.parametrize("m,seed,with_mask", [(500, 99, True), (2000, 7, True), (300, 3, False), (1200, 21, False)])
def test_recover_pose_matches_the_numpy_restatement(pc, m, seed, with_mask):
    a, b, E, Rtrue, ttrue = _scene(m, seed)
    mask = (np.random.default_rng(seed).random(m) < 0.9).astype(np.uint8) if with_mask else None
    f, ppx, ppy = K[0, 0], K[0, 2], K[1, 2]
    got = recover(pc, a, b, E, f, ppx, ppy, mask=mask)
    sel, R, t, g, masks, near = np_recover(a, b, E, f, ppx, ppy, mask=mask)
    assert got["flags"] == 0
    assert np.abs(got["R"] - R).max() < 1e-9 and np.abs(got["t"] - t).max() < 1e-9
    assert np.abs(got["R"] - Rtrue).max() < 1e-2 and np.abs(got["t"] - ttrue).max() < 1e-1     # (and it is the scene's pose)
    assert near.sum() <= max(2, m // 200), near.sum()
    keep = ~near
    mine = got["mask"] != 0
    assert np.array_equal(mine[keep], masks[sel][keep])
    assert abs(got["n_good"] - int(g[sel])) <= near.sum() and got["n_good"] == int(mine.sum())
    # the four counts, candidate by candidate (numpy's SVD may order R1 / R2 and sign t the other way)
    R1, R2, tt, _ = decompose(pc, E)
    nR1, nR2, nt = np_decompose(E)
    ncands = [(nR1, nt), (nR2, nt), (nR1, -nt), (nR2, -nt)]
    for c, (Rc, tc) in enumerate([(R1, tt), (R2, tt), (R1, -tt), (R2, -tt)]):
        k = [i for i, (Rn, tn) in enumerate(ncands) if np.abs(Rn - Rc).max() < 1e-9 and np.abs(tn - tc).max() < 1e-9]
        assert len(k) == 1 and abs(int(got["counts"][c]) - int(g[k[0]])) <= near.sum(), (c, k)
    assert got["n_good"] > 0.6 * m
    want_byte = 1 if with_mask else 255                 # bitwise_and(mask, mask1): the input's byte, or 255 without one
    assert set(np.unique(got["mask"])) <= {0, want_byte}


def test_all_zero_mask_selects_the_first_candidate(pc):
    a, b, E, _, _ = _scene(400, 11)
    got = recover(pc, a, b, E, K[0, 0], K[0, 2], K[1, 2], mask=np.zeros(400, np.uint8))
    R1, _, t, _ = decompose(pc, E)
    assert list(got["counts"]) == [0, 0, 0, 0] and got["n_good"] == 0 and got["sel"] == 0
    assert np.array_equal(got["R"], R1) and np.array_equal(got["t"], t) and not got["mask"].any()


def test_empty_pair(pc):
    R1, _, t, _ = decompose(pc, _scene(10, 1)[2])
    got = recover(pc, np.zeros((0, 2)), np.zeros((0, 2)), _scene(10, 1)[2], K[0, 0], K[0, 2], K[1, 2])
    assert got["n_good"] == 0 and got["sel"] == 0 and np.array_equal(got["R"], R1)


def test_far_points_are_cut(pc):
    a, b, E, _, _ = _scene(500, 99, outliers=0.0)
    near = recover(pc, a, b, E, K[0, 0], K[0, 2], K[1, 2])
    # the scene's depths are 4..8 baselines (|t| ~ 1): a threshold of 6 cuts the far part, 3 cuts everything
    mid = recover(pc, a, b, E, K[0, 0], K[0, 2], K[1, 2], dist=6.0)
    none = recover(pc, a, b, E, K[0, 0], K[0, 2], K[1, 2], dist=3.0)
    assert near["n_good"] > 450 and 0 < mid["n_good"] < near["n_good"] and none["n_good"] == 0
    sel, _, _, g, _, _ = np_recover(a, b, E, K[0, 0], K[0, 2], K[1, 2], dist=6.0)
    assert abs(mid["n_good"] - int(g[sel])) <= 1
    # 50 baselines: the same scene scaled 10x in depth (points at 40..80) loses the part beyond 50
    sc = synth.two_view_scene(m=500, seed=99, K=K, noise_px=0.0, outlier_frac=0.0)
    X = sc["X_true"] * [1, 1, 10]
    P2 = sc["P2"]
    proj = lambda P: ((X @ P[:, :3].T + P[:, 3])[:, :2] / (X @ P[:, :3].T + P[:, 3])[:, 2:3]) @ K[:2, :2].T + K[:2, 2]
    a2, b2 = proj(sc["P1"]), proj(P2)
    far = recover(pc, a2, b2, _essential(P2[:, :3], P2[:, 3]), K[0, 0], K[0, 2], K[1, 2])
    t_norm = np.linalg.norm(P2[:, 3])
    depth = X[:, 2] / t_norm                               # in baselines (recoverPose's t has unit length)
    assert 50 < depth.max() and depth.min() < 50
    assert abs(far["n_good"] - int((depth < 50).sum())) <= 5, (far["n_good"], int((depth < 50).sum()))


def test_normalisation_uses_the_one_focal(pc):
    rng = np.random.default_rng(3)
    for u, v in rng.uniform(0, 640, (50, 2)):
        xy = np.zeros(2)
        pc.pose_normalize(u, v, K[0, 0], K[0, 2], K[1, 2], _p(xy))
        a = 1.0 / K[0, 0]
        assert xy[0] == u * a + (-K[0, 2] * a) and xy[1] == v * a + (-K[1, 2] * a)   # fx for y too, bit for bit
    # through recoverPose: the numpy restatement with fy in the y normalisation disagrees, with fx it agrees
    a, b, E, _, _ = _scene(800, 5)
    got = recover(pc, a, b, E, K[0, 0], K[0, 2], K[1, 2])
    sel, _, _, _, masks, near = np_recover(a, b, E, K[0, 0], K[0, 2], K[1, 2])
    assert np.array_equal((got["mask"] != 0)[~near], masks[sel][~near])


# ---------------------------------------------------------------- CheckCoherentRotation
def test_float_narrowed_rotation_check(pc):
    assert pc.pose_coherent_det(1.0) and pc.pose_coherent_det(-1.0)
    assert pc.pose_coherent_det(1 + 5e-8)                # rounds to 1.0f
    assert not pc.pose_coherent_det(1 + 1e-7)            # rounds to 1.0000001f
    assert pc.pose_coherent_det(float("nan"))            # NaN - 1.0 > 1e-7 is false
    assert pc.pose_coherent_det(0.5) and not pc.pose_coherent_det(2.0)   # one-sided: only |det| above 1 fails
    for d, ok in ((1 + 5e-8, 1), (1 + 1e-7, 0), (1.0, 1)):
        R = np.ascontiguousarray(np.diag([d, 1.0, 1.0]))
        assert pc.pose_fullpivlu_det(_p(R)) == d and pc.pose_check_rotation(_p(R)) == ok
    rng = np.random.default_rng(9)
    for _ in range(50):
        R = np.ascontiguousarray(_rot(rng, 1.0))
        d = pc.pose_fullpivlu_det(_p(R))
        assert abs(d - np.linalg.det(R)) < 1e-14 and pc.pose_check_rotation(_p(R)) == 1
        M = np.ascontiguousarray(rng.normal(0, 1, (3, 3)))
        assert abs(pc.pose_fullpivlu_det(_p(M)) - np.linalg.det(M)) < 1e-12 * max(1, abs(np.linalg.det(M)))
    Rn = np.ascontiguousarray(np.full((3, 3), np.nan))
    assert pc.pose_check_rotation(_p(Rn)) == 1


def test_python_rotation_check_matches_the_header(pc):
    from sfm_danpipeline_amd import pose
    rng = np.random.default_rng(2)
    mats = [np.diag([1 + 5e-8, 1, 1]), np.diag([1 + 1e-7, 1, 1]), np.full((3, 3), np.nan), np.zeros((3, 3))]
    mats += [_rot(rng, 1.0) for _ in range(20)] + [rng.normal(0, 1, (3, 3)) for _ in range(20)]
    for M in mats:
        M = np.ascontiguousarray(M, np.float64)
        d = pc.pose_fullpivlu_det(_p(M))
        assert np.array_equal(np.float64(pose.determinante(M)), np.float64(d), equal_nan=True)
        assert pose.check_coherent_rotation(M) == bool(pc.pose_check_rotation(_p(M)))


def test_python_pose_refusals_before_any_device_call():
    """getCameraPose's early exits (src/Sfm.cpp:720-739): an empty K, or 7 or fewer aligned points -- no device needed"""
    from sfm_danpipeline_amd import pose
    a, b, _, _, _ = _scene(50, 4)
    assert pose.get_camera_pose(np.zeros((0, 0)), a, b) is None
    assert pose.get_camera_pose(K, a[:7], b[:7]) is None
    pts = [a, b]
    assert pose.base_reconstruction([(0.5, (0, 1))], pts, {(0, 1): (np.arange(50), np.arange(50))}, np.zeros((0, 0))) is None
    assert pose.base_reconstruction([], pts, {}, K) is None


# ---------------------------------------------------------------- sanitizers
def test_recover_pose_under_asan_ubsan(pc, tmp_path):
    exe = str(tmp_path / "pose_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DPOSE_MAIN", "-o", exe, STUB])
    a, b, E, _, _ = _scene(700, 13)
    mask = (np.random.default_rng(13).random(700) < 0.9).astype(np.uint8)
    f, ppx, ppy = K[0, 0], K[0, 2], K[1, 2]
    with open(tmp_path / "in.bin", "wb") as fo:
        fo.write(np.array([700, 1], np.int32).tobytes() + np.array([f, ppx, ppy, 50.0], np.float64).tobytes())
        fo.write(np.ascontiguousarray(E, np.float64).tobytes() + np.ascontiguousarray(a, np.float64).tobytes())
        fo.write(np.ascontiguousarray(b, np.float64).tobytes() + mask.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300, env=env)
    bad = [m for m in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:") if m in r.stderr]
    assert r.returncode == 0 and not bad, r.stderr[-3000:]
    got = recover(pc, a, b, E, f, ppx, ppy, mask=mask)
    lines = r.stdout.split()
    assert lines[:11] == ["sel", str(got["sel"]), "n_good", str(got["n_good"]), "counts", *map(str, got["counts"]), "flags", "0"]
    words = np.array([int(w, 16) for w in lines[11:23]], np.uint64)
    assert np.array_equal(words, np.concatenate([got["R"].ravel(), got["t"]]).view(np.uint64))


# ---------------------------------------------------------------- every candidate, ties, degenerate E (tests/pose_scenes.py)
def _family_run(pc, R, sign, m=300, noise=0.3, seed=100):
    """recoverPose by the stub and by numpy on the four members of family(R) under sign * E: [(member's true R, true unit
    t, stub result, np_recover result)]"""
    E = sign * S.essential(R, S.T)
    out = []
    for k, (Rk, tk) in enumerate(S.family(R)):
        a, b = S.scene(Rk, tk, m, seed + k, noise)
        out.append((Rk, tk / np.linalg.norm(tk), recover(pc, a, b, E, S.F, S.PPX, S.PPY), np_recover(a, b, E, S.F, S.PPX, S.PPY)))
    return E, out


def test_every_candidate_wins_somewhere(pc):
    """The four poses that share one E land on four different candidates, and the three rotations permute which: the choice
    is the scene's true pose, numpy's restatement picks the same one and counts the same, candidate by candidate."""
    m, chosen = 300, set()
    for ri, R in enumerate(S.ROTATIONS):
        for sign in (1, -1):
            E, runs = _family_run(pc, R, sign, m=m, seed=100 + 10 * ri)
            sels = [got["sel"] for _, _, got, _ in runs]
            assert sorted(sels) == [0, 1, 2, 3], (ri, sign, sels)
            if ri == 0:
                assert sels == S.FAMILY_WINNERS, (sign, sels)
            chosen |= set(sels)
            R1, R2, tt, fl = decompose(pc, E)
            assert fl == 0
            cands = [(R1, tt), (R2, tt), (R1, -tt), (R2, -tt)]
            nR1, nR2, nt = np_decompose(E)
            ncands = [(nR1, nt), (nR2, nt), (nR1, -nt), (nR2, -nt)]
            for k, (Rk, tk, got, (sel, Rn, tn, g, masks, near)) in enumerate(runs):
                assert got["flags"] == 0
                assert np.array_equal(got["R"], cands[got["sel"]][0]) and np.array_equal(got["t"], cands[got["sel"]][1])
                assert np.abs(got["R"] - Rk).max() < 1e-2 and np.abs(got["t"] - tk).max() < 1e-1, (ri, sign, k)
                assert np.abs(got["R"] - Rn).max() < 1e-9 and np.abs(got["t"] - tn).max() < 1e-9, (ri, sign, k)
                assert near.sum() <= max(2, m // 200), near.sum()
                mine = got["mask"] != 0
                assert np.array_equal(mine[~near], masks[sel][~near])
                assert abs(got["n_good"] - int(g[sel])) <= near.sum() and got["n_good"] == int(mine.sum()) > 0.9 * m
                for c, (Rc, tc) in enumerate(cands):
                    j = [i for i, (Rx, tx) in enumerate(ncands) if np.abs(Rx - Rc).max() < 1e-9 and np.abs(tx - tc).max() < 1e-9]
                    assert len(j) == 1 and abs(int(got["counts"][c]) - int(g[j[0]])) <= near.sum(), (ri, sign, k, c, j)
    assert chosen == {0, 1, 2, 3}


@pytest.mark.parametrize("parts,counts,choice", S.TIES)
def test_tied_counts_take_the_first_candidate(pc, parts, counts, choice):
    a, b = S.mixture(parts)
    assert len(a) == sum(n for _, n in parts)
    got = recover(pc, a, b, S.E0, S.F, S.PPX, S.PPY)
    assert list(got["counts"]) == counts and got["sel"] == choice and got["n_good"] == counts[choice] == max(counts)
    R1, R2, t, _ = decompose(pc, S.E0)
    assert np.array_equal(got["R"], R2 if choice & 1 else R1) and np.array_equal(got["t"], -t if choice & 2 else t)
    assert int((got["mask"] != 0).sum()) == counts[choice]


def test_degenerate_and_scaled_essential_matrices(pc):
    """flags: 1 where a singular value is not above DBL_MIN (zero, rank 1, NaN, squares that underflow or overflow), else 0;
    an unflagged scaled E gives the unscaled pose and count (the candidate's index may move with the scale: the SVD's signs)"""
    fam = S.family()
    a, b = S.scene(*fam[0], 300, 100, 0.3)
    base = recover(pc, a, b, S.E0, S.F, S.PPX, S.PPY)
    assert base["flags"] == 0 and base["n_good"] == 300
    assert set(S.FLAGGED) == {"zero", "rank1", "nan", "1e-200", "1e200"} and set(S.UNFLAGGED) == {"1e-75", "1e-100", "1e-140", "1e60", "1e75"}
    for name, (E, flags) in S.DEGENERATE.items():
        got = recover(pc, a, b, E, S.F, S.PPX, S.PPY)
        assert got["flags"] == flags == decompose(pc, E)[3], name
        if not flags:
            worst = max(np.abs(got["R"] - base["R"]).max(), np.abs(got["t"] - base["t"]).max())
            assert worst < 1e-6 and got["n_good"] == base["n_good"], (name, worst)
            assert np.array_equal(got["mask"], base["mask"]), name
    assert not np.isfinite(recover(pc, a, b, S.DEGENERATE["1e200"][0], S.F, S.PPX, S.PPY)["R"]).all()
    assert np.isnan(recover(pc, a, b, S.DEGENERATE["nan"][0], S.F, S.PPX, S.PPY)["R"]).all()


def test_mask_bytes_pass_through(pc):
    """bitwise_and(mask, mask1): the output is the input BYTE where the candidate passes, whatever it is, and 0 elsewhere"""
    fam = S.family()
    a, b = S.scene(*fam[0], 300, 100, 0.3, outliers=0.2)
    mb = S.mask_bytes(300)
    assert set(np.unique(mb)) == set(S.MASK_BYTES.tolist())
    free = recover(pc, a, b, S.E0, S.F, S.PPX, S.PPY)
    got = recover(pc, a, b, S.E0, S.F, S.PPX, S.PPY, mask=mb)
    assert got["sel"] == free["sel"]
    passes = free["mask"] != 0
    assert 0 < passes.sum() < 300 and set(np.unique(mb[passes])) == set(S.MASK_BYTES.tolist())
    assert np.array_equal(got["mask"], np.where(passes, mb, 0).astype(np.uint8))
    assert got["n_good"] == int((passes & (mb != 0)).sum())
    assert set(np.unique(free["mask"])) == {0, 255}


def test_distance_thresholds(pc):
    """depths are 4 .. 8 baselines: 6 cuts a part, 3 and below everything, inf nothing, and a NaN compares false"""
    fam = S.family()
    a, b = S.scene(*fam[0], 300, 100, 0.3)
    ng = [recover(pc, a, b, S.E0, S.F, S.PPX, S.PPY, dist=d)["n_good"] for d in S.THRESHOLDS]
    assert S.THRESHOLDS[:5] == [50.0, 6.0, 3.0, 0.0, -1.0] and np.isinf(S.THRESHOLDS[5]) and np.isnan(S.THRESHOLDS[6])
    assert ng[0] == 300 and 0 < ng[1] < 300 and ng[2:5] == [0, 0, 0] and ng[5] == 300 and ng[6] == 0
