"""CPU: csrc/ransac_host.h's ransac_replay -- OpenCV 3.4.1's RANSACPointSetRegistrator::run replayed in chunks of 32, 64,
128, 256, 256, ... iterations, the one loop behind sfmhip_score_essential, sfmhip_score_homography and sfmhip_pnp_ransac --
against a one-iteration-at-a-time transcription of run(), through a g++ build (tests/stub/ransac_capi.cpp) whose backend
answers from tables: the test scripts how many models every iteration of every view gives, their inlier counts and flags,
and asserts that the chunked form ends where the plain loop ends.  Also the homography's rejection sampler
(csrc/score_host.h) against a transcription of getSubset + checkSubset, and RANSACUpdateNumIters against the oracle's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "ransac_capi.cpp")
ESSENTIAL, HOMOGRAPHY, PNP = 0, 1, 2
MP = {ESSENTIAL: 5, HOMOGRAPHY: 4, PNP: 5}           # model points
MM = {ESSENTIAL: 10, HOMOGRAPHY: 1, PNP: 1}          # models per sample
POLICIES = pytest.mark.parametrize("policy", [ESSENTIAL, HOMOGRAPHY, PNP], ids=["essential", "homography", "pnp"])
T = 1248                                             # the chunks end at 32, 96, 224, 480, 736, 992, 1248 iterations
CHUNK_ENDS = (32, 96, 224, 480, 736, 992)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("ransac")), "libransaccapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.ransac_update_num_iters_c.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int]
    lib.ransac_scripted.argtypes = [C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_double, C.c_int, C.c_int] + [vp] * 6
    lib.ransac_has_code.argtypes = [C.c_int] * 3
    lib.homography_samples.argtypes = [C.c_int, vp, vp, C.c_int, vp]
    lib.homography_samples.restype = None
    return lib


class Script:
    """what every iteration of every view gives: nm[v, i] models of cnt[v, i, m] inliers and flags[v, i]; by default one
    model that never raises (no inliers)"""

    def __init__(self, policy, n_corr):
        self.policy, self.n_corr = policy, np.asarray(n_corr, np.int32)
        v = len(n_corr)
        self.nm = np.ones((v, T), np.int32)
        self.cnt = np.zeros((v, T, MM[policy]), np.int32)
        self.flags = np.zeros((v, T), np.int32)
        self.dead_at = np.full(v, -1, np.int32)

    def only(self, v):
        s = Script(self.policy, self.n_corr[v:v + 1])
        s.nm, s.cnt, s.flags, s.dead_at = (np.ascontiguousarray(a[v:v + 1]) for a in (self.nm, self.cnt, self.flags, self.dead_at))
        return s


def replay(L, s, confidence=0.99, max_iters=1000, real_sampler=False):
    """the chunked loop; per view (best, iter, status, kept (iteration, m) or None), and the OR of the flags of all views"""
    v = len(s.n_corr)
    out = [np.zeros(v, np.int32) for _ in range(5)]
    fl = C.c_int32(0)
    rc = L.ransac_scripted(s.policy, v, s.n_corr.ctypes.data, T, s.nm.ctypes.data, s.cnt.ctypes.data, s.flags.ctypes.data,
                           s.dead_at.ctypes.data, float(confidence), int(max_iters), int(real_sampler),
                           *[a.ctypes.data for a in out], C.addressof(fl))
    assert rc == 0, f"the stub's backend refused the loop's calls: {rc} (71: sample rows, 72: keep list)"
    best, it, status, kit, km = out
    return [(int(best[i]), int(it[i]), int(status[i]), (int(kit[i]), int(km[i])) if kit[i] >= 0 else None) for i in range(v)], fl.value


def plain(L, s, v, confidence=0.99, max_iters=1000):
    """RANSACPointSetRegistrator::run (calib3d/ptsetreg.cpp) for view v, one iteration at a time:
    (best, iter, status, kept, flags)"""
    mp, count = MP[s.policy], int(s.n_corr[v])
    niters = 1000 if s.policy == ESSENTIAL else max(max_iters, 1) if s.policy == HOMOGRAPHY else max(max_iters, 0)
    if count < mp:
        return (0, 0, -1, None), 0
    if count == mp:                                   # runKernel on the points themselves; every point an inlier
        has = s.nm[v, 0] > 0
        return (mp if has else 0, 0, 1 if has else 0, (0, 0) if has else None), int(s.flags[v, 0])
    best, kept, flags, it = 0, None, 0, 0
    while it < niters:
        if 0 <= s.dead_at[v] <= it and s.policy == HOMOGRAPHY:   # getSubset found no sample: iteration 0 returns false, later ones break
            break
        flags |= int(s.flags[v, it])
        for m in range(int(s.nm[v, it])):             # (nmodels <= 0: continue)
            good = int(s.cnt[v, it, m])
            if good > max(best, mp - 1):
                best, kept = good, (it, m)
                niters = L.ransac_update_num_iters_c(confidence, (count - good) / count, mp, niters)
        it += 1
    return (best, it, 1 if kept else 0, kept), flags


def check(L, s, **kw):
    """the chunked replay of every view of the script equals the plain loop; returns the per-view results"""
    got, fl = replay(L, s, **kw)
    kw.pop("real_sampler", None)
    want = [plain(L, s, v, **kw) for v in range(len(s.n_corr))]
    assert got == [w[0] for w in want]
    f = 0
    for w in want:
        f |= w[1]
    assert fl == f
    return got, fl


def test_update_num_iters_equals_the_oracle(L):
    for p in (0.5, 0.9, 0.99, 0.995, 0.999, 1.0):
        for ep in (0.0, 1e-9, 0.01, 0.2, 0.5, 0.77, 0.9, 0.999, 1.0):
            for mp in (4, 5):
                for mx in (0, 1, 7, 100, 1000, 2000):
                    assert L.ransac_update_num_iters_c(p, ep, mp, mx) == orc.lib().orc_ransac_update_num_iters(p, ep, mp, mx)


@POLICIES
def test_has_code(L, policy):
    mp = MP[policy]
    assert [L.ransac_has_code(s, c, mp) for s, c in ((-1, mp - 1), (0, mp), (1, mp), (0, 50), (1, 50))] == [0, 0, 2, 0, 1]


@POLICIES
def test_counts_around_the_model_points(L, policy):
    mp = MP[policy]
    s = Script(policy, [mp - 1, mp, mp, mp + 1, mp + 1])
    s.nm[2, 0] = 0                                    # the minimal view whose one sample gives no model
    s.flags[1, 0], s.flags[2, 0] = 1, 2               # both are looked at
    s.flags[1, 1] = s.flags[2, 1] = 4                 # a second slot of such a view is not
    s.cnt[3, 3, 0] = mp + 1                           # every point an inlier at iteration 3: the limit drops to 0
    got, fl = check(L, s)
    assert got[0] == (0, 0, -1, None)
    assert got[1] == (mp, 0, 1, (0, 0)) and got[2] == (0, 0, 0, None)
    assert got[3] == (mp + 1, 4, 1, (3, 0)) and got[4] == (0, 1000, 0, None)
    assert fl == 3


CAPS = (1, 31, 32, 33, 95, 96, 97, 223, 224, 225, 479, 480, 481, 735, 736, 737, 991, 992, 993, 1000)


@pytest.mark.parametrize("policy", [HOMOGRAPHY, PNP], ids=["homography", "pnp"])
def test_caps_on_and_around_the_chunk_ends(L, policy):
    """counts that never raise: a view runs to max_iters, whichever chunk that falls in; the flag of the last iteration is
    seen and the one past it is not"""
    s = Script(policy, [50])
    s.nm[0, ::3] = 0                                  # (some samples without a model)
    for cap in CAPS:
        s.flags[:] = 0
        s.flags[0, cap - 1], s.flags[0, cap] = 1, 2
        got, fl = check(L, s, max_iters=cap)
        assert got[0] == (0, cap, 0, None) and fl == 1


def test_essential_runs_to_its_fixed_limit(L):
    s = Script(ESSENTIAL, [50])
    s.nm[:] = 10
    s.cnt[:] = 4                                      # ten models a sample, none above four inliers: nothing is kept
    s.flags[0, 999], s.flags[0, 1000] = 1, 2
    got, fl = check(L, s, max_iters=7)                # (max_iters is not the essential matrix's to set)
    assert got[0] == (0, 1000, 0, None) and fl == 1


@POLICIES
def test_a_raise_that_pulls_the_limit_below_the_current_iteration(L, policy):
    """iteration 40 (the second chunk: 32 .. 95) finds 95 of 100: the limit becomes a handful and the loop ends at 41; the
    chunk's later slots hold a better model and a flag, and neither may show"""
    s = Script(policy, [100])
    s.cnt[0, 40, 0] = 95
    s.cnt[0, 41:96, 0] = 99
    s.flags[0, 41:96] = 4
    s.flags[0, 40] = 1
    got, fl = check(L, s)
    assert L.ransac_update_num_iters_c(0.99, 0.05, MP[policy], 1000) < 40
    assert got[0] == (95, 41, 1, (40, 0)) and fl == 1


@POLICIES
def test_raises_in_the_last_slot_of_a_chunk_and_the_first_of_the_next(L, policy):
    """small raises (the limit stays at 1000) at iterations 31 | 32 and 95 | 96: each is kept from the chunk it is in"""
    s = Script(policy, [1000] * 5)
    s.cnt[0, 31, 0] = 6
    s.cnt[1, 32, 0] = 6
    s.cnt[2, 31, 0], s.cnt[2, 32, 0] = 6, 7
    s.cnt[3, 95, 0], s.cnt[3, 96, 0] = 6, 7
    s.cnt[4, 31, 0], s.cnt[4, 96, 0], s.cnt[4, 991, 0], s.cnt[4, 992, 0] = 6, 7, 8, 9
    got, _ = check(L, s)
    assert [g[3] for g in got] == [(31, 0), (32, 0), (32, 0), (96, 0), (992, 0)]
    assert all(g[1] == 1000 for g in got)


def test_essential_models_of_one_sample(L):
    s = Script(ESSENTIAL, [1000] * 4)
    s.nm[:] = 10
    s.cnt[:] = 4                                      # (four inliers never count: good > max(best, 4))
    s.cnt[0, 5, 3], s.cnt[0, 5, 7] = 20, 30           # two models of one sample raise: the later one stays
    s.cnt[1, 5, 3], s.cnt[1, 5, 7] = 30, 30           # a tie inside a sample: the first stays
    s.cnt[2, 5, 7], s.cnt[2, 40, 0] = 30, 30          # a tie with a later sample (the next chunk): the first stays
    s.cnt[3, 5, 7], s.nm[3, 5] = 30, 7                # a model past the sample's number of models is not one
    got, _ = check(L, s)
    assert [g[3] for g in got] == [(5, 7), (5, 3), (5, 7), None]
    assert [g[0] for g in got] == [30, 30, 30, 0]


def test_homography_dead_streams(L):
    """getSubset gives up: at iteration 0 there is no model at all, later the loop ends there with what it has -- in the
    middle of a chunk and exactly where a chunk starts"""
    dead = [0, 50, 32, 96, 31, -1]
    s = Script(HOMOGRAPHY, [1000] * len(dead))
    s.dead_at[:] = dead
    s.cnt[:, 10, 0] = 6                               # (a small raise before: kept by all but the first)
    s.flags[:, 0] = 1
    for v, d in enumerate(dead):
        if d >= 0:
            s.nm[v, d:], s.cnt[v, d:, 0], s.flags[v, d:] = 1, 999, 8   # (what a dead row would give if it were read)
    got, fl = check(L, s)
    assert got[0] == (0, 0, 0, None)
    assert [g[1] for g in got] == [0, 50, 32, 96, 31, 1000]
    assert all(g == (6, g[1], 1, (10, 0)) for g in got[1:]) and fl == 1


def test_pnp_without_iterations(L):
    s = Script(PNP, [4, 5, 6, 50])
    s.cnt[:, 0, 0] = 6
    got, _ = check(L, s, max_iters=0)
    assert got == [(0, 0, -1, None), (5, 0, 1, (0, 0)), (0, 0, 0, None), (0, 0, 0, None)]
    got, _ = check(L, s.only(3), max_iters=-3)        # (the C entry point refuses a negative limit; the loop reads it as 0)
    assert got == [(0, 0, 0, None)]
    got, _ = check(L, Script(HOMOGRAPHY, [50]), max_iters=0)   # (findHomography's limit is at least one iteration)
    assert got == [(0, 1, 0, None)]


@POLICIES
def test_views_of_a_batch_do_not_depend_on_each_other(L, policy):
    """eight views that leave the loop in different chunks (and two that never enter it), in one call and each alone: the
    job list shrinks from chunk to chunk, and with the per-count sampler of the essential-matrix and PnP uses (the stub
    checks every row it is handed against that count's stream) views of one count share a stream at different iterations"""
    mp = MP[policy]
    count = [200, 100, 200, 100, 200, 200, 100, 200, mp, mp - 1]
    share = [0.8, 0.7, 0.6, 0.5, 0.4, 0.35, 0.3, 0.0]            # of inliers at iteration 2 (the last view never raises)
    s = Script(policy, count)
    for v, w in enumerate(share):
        s.cnt[v, 2, -1] = round(w * count[v])
        s.nm[v, 2] = MM[policy]
        s.flags[v, 1] = 1 << v
    real = policy != HOMOGRAPHY
    got, fl = check(L, s, real_sampler=real)
    ends = [g[1] for g in got[:8]]
    assert ends == sorted(ends) and ends[0] < 32 and ends[-1] == 1000
    assert len({sum(e > c for c in CHUNK_ENDS) for e in ends}) >= 6   # (a condition on the script: the chunks the views leave in)
    assert fl == 255
    for v in range(len(count)):
        alone, fl1 = replay(L, s.only(v), real_sampler=real)
        assert alone[0] == got[v] and fl1 == (1 << v if v < 8 else 0)


# ---------------------------------------------------------------- the homography's sample stream
class _Rng:                                           # cv::RNG((uint64)-1)
    def __init__(self):
        self.state = 0xFFFFFFFFFFFFFFFF

    def uniform(self, a, b):
        if a == b:
            return a
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return (self.state & 0xFFFFFFFF) % (b - a) + a


def _have_collinear(p):
    """haveCollinearPoints(m, 4): the triples that hold the last point (differences in float, the rest in double)"""
    f = np.float32
    for j in range(3):
        dx1, dy1 = float(f(p[j][0]) - f(p[3][0])), float(f(p[j][1]) - f(p[3][1]))
        for k in range(j):
            dx2, dy2 = float(f(p[k][0]) - f(p[3][0])), float(f(p[k][1]) - f(p[3][1]))
            if abs(dx2 * dy1 - dy2 * dx1) <= float(np.finfo(f).eps) * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def _check_subset(a, b):
    """HomographyEstimatorCallback::checkSubset for four pairs: no collinear triple, the orientations of every triple kept"""
    if _have_collinear(a) or _have_collinear(b):
        return False

    def det(q, t):
        m = [float(q[t[0]][0]), float(q[t[0]][1]), 1.0, float(q[t[1]][0]), float(q[t[1]][1]), 1.0, float(q[t[2]][0]), float(q[t[2]][1]), 1.0]
        return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    negative = sum(det(a, t) * det(b, t) < 0 for t in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)))
    return negative in (0, 4)


def _subsets(m1, m2, n):
    """getSubset per iteration: distinct indices, drawn again (the RNG moves on) while checkSubset refuses; (rows, refused)"""
    rng, rows, refused = _Rng(), [], 0
    for _ in range(n):
        for _attempt in range(10000):
            idx = []
            while len(idx) < 4:
                v = rng.uniform(0, len(m1))
                if v not in idx:
                    idx.append(v)
            if _check_subset(m1[idx], m2[idx]):
                break
            refused += 1
        else:
            raise AssertionError("no acceptable sample")
        rows.append(idx)
    return np.array(rows, np.int32), refused


def test_homography_samples_redraw_after_a_refused_subset(L):
    """five points of which three lie on a line: the samples that hold the three (with the last drawn on the line) are
    refused and drawn again from the same RNG, so every later row depends on the refusals"""
    m1 = np.array([[0, 0], [10, 10], [20, 20], [30, 5], [7, 41]], np.float32)
    H = np.array([[1.1, 0.1, 3.0], [-0.05, 0.95, -2.0], [1e-4, 2e-4, 1.0]])
    q = np.c_[m1.astype(np.float64), np.ones(5)] @ H.T
    m2 = np.ascontiguousarray((q[:, :2] / q[:, 2:]).astype(np.float32))
    n = 64
    want, refused = _subsets(m1, m2, n)
    assert refused >= 10                              # a condition on the scene: the rejection path is taken
    got = np.zeros((n, 4), np.int32)
    L.homography_samples(5, m1.ctypes.data, m2.ctypes.data, n, got.ctypes.data)
    assert np.array_equal(got, want)


def test_homography_samples_go_dead_on_a_line(L):
    """every point on one line: no subset is ever accepted; the stream is -1 from its first row"""
    m1 = np.ascontiguousarray(np.c_[np.arange(6), 2 * np.arange(6)].astype(np.float32))
    got = np.zeros((3, 4), np.int32)
    L.homography_samples(6, m1.ctypes.data, m1.ctypes.data, 3, got.ctypes.data)
    assert np.all(got == -1)
