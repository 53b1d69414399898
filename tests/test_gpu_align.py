"""GPU: the coarse plot alignment (csrc/align.hip and register.hip's batch) against the g++ build of the same
headers (tests/stub/align_capi.cpp), byte for byte: the batch's results and idx rows against the stub's batch and against
sfmhip_cloud_register called per start on the device, for sources on both sides of a sum block and at the size where the
single call starts to walk the source in cell order, for 1 to 65 starts that converge, hit the limit, end FEW and end
DEGENERATE; the target handle reused around a single registration and a filter; the vote's candidates and stats for the CPU
file's shapes, for target samples on both sides of the kernel's tile and at the ceilings; the hand-made edges; the empty
cases and the refusals; the whole alignment on two planted motions; and the host mirror's self-test."""
import math
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, register
from sfm_danpipeline_amd.cloud import Cloud
from sfm_danpipeline_amd.register import DEGENERATE, EMPTY, FEW, NO_WINNER, Frame, Transform
from tests.test_align_cpu import (FULL_ICP, GOOD, LEVEL, MOTIONS, RECOVERY, al, fill_starts, mirrored_points, mixed_batch, recovery_scene,  # noqa: F401
                                  small_scene, struct_bytes, stub_align, stub_align_opts, stub_batch, stub_vote, yaw_motion)
from tests.test_register_cpu import motion_errors, moved_back, planted_plot, result_bytes

pytestmark = pytest.mark.gpu
TILE = 256   # aln_vote's target tile


def assert_batch(al, tc, sc, tgt, src, starts, singles=True, **kw):
    """One device batch against the stub's and against the device's single calls: the same bytes."""
    want, widx, _ = stub_batch(al, tgt, src, starts, **kw)
    got = register.icp_batch(tc, sc, starts, return_pairs=True, **kw)
    assert len(got) == len(starts)
    for b, (g, w) in enumerate(zip(got, want)):
        assert result_bytes(g) == result_bytes(w), b
        assert np.array_equal(g.idx, widx[b]), b
        if singles:
            one = register.icp(tc, sc, starts[b], return_pairs=True, **kw)
            assert result_bytes(one) == result_bytes(g) and np.array_equal(one.idx, g.idx), b
    return got


def assert_vote(al, tc, sc, tgt, src, ft, fs, o):
    want, wst = stub_vote(al, tgt, src, ft, fs, o)
    got, gst = register.align_vote(tc, sc, ft, fs, opts=o)
    assert [struct_bytes(c) for c in got] == [struct_bytes(c) for c in want]
    assert struct_bytes(gst) == struct_bytes(wst)
    return got, gst


def vote_equal(al, ctx, tgt, src, ft, fs, o):
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        return assert_vote(al, tc, sc, tgt, src, ft, fs, o)


# ---------------------------------------------------------------- the batch
@pytest.mark.parametrize("n_src,B", [(1, 1), (1, 65), (255, 2), (255, 64), (256, 1), (256, 65), (257, 2), (257, 64), (8192, 1), (8192, 2), (8192, 65)])
def test_batch_bytes(ctx, al, n_src, B):
    tgt, src, starts, kw = mixed_batch(n_src)
    starts = fill_starts(starts, B)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        res = assert_batch(al, tc, sc, tgt, src, starts, **kw)
    if n_src >= 255:
        assert (res[0].converged, res[0].flags, res[0].pairs) == (1, 0, n_src)
    if n_src >= 255 and B >= 64:
        assert (res[1].iterations, res[2].flags, res[3].flags) == (6, FEW, DEGENERATE)


def test_mixed_batch_and_its_timing(ctx, al):
    tgt, src, starts, kw = mixed_batch()
    starts = fill_starts(starts, 7)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        ctx.set_timing(True)
        try:
            res = assert_batch(al, tc, sc, tgt, src, starts, singles=False, **kw)
            t = register.batch_last_timing(tc)
        finally:
            ctx.set_timing(False)
        assert [r.flags for r in res[:4]] == [0, 0, FEW, DEGENERATE] and (res[0].converged, res[1].converged, res[1].iterations) == (1, 0, 6)
        assert t["iterations"] == max(r.iterations for r in res) == 6 and all(0 < t[k] < 5000 for k in ("search", "sums", "update"))
        assert_batch(al, tc, sc, tgt, src, starts, **kw)                                # and against the single calls
        assert register.batch_last_timing(tc) == dict(search=0.0, sums=0.0, update=0.0, iterations=6)
        line = np.outer(np.arange(40, dtype=np.float32), np.array([1.0, 2.0, -1.0], np.float32))
        with Cloud(line, ctx=ctx) as lc, Cloud(line + np.float32(0.01), ctx=ctx) as ls, Cloud(line[:0], ctx=ctx) as empty:
            starts3 = [Transform.make(), Transform.make(t=[500.0, 0, 0]), Transform.make(t=[0.01, 0, 0])]
            res = assert_batch(al, lc, ls, line, line + np.float32(0.01), starts3, max_dist=5.0)
            assert [r.flags for r in res] == [DEGENERATE, FEW, DEGENERATE]
            assert [r.flags for r in assert_batch(al, lc, empty, line, line[:0], starts3)] == [FEW] * 3
            assert [r.flags for r in assert_batch(al, empty, ls, line[:0], line, starts3)] == [FEW] * 3


def test_target_handle_reused_around_a_single_call_and_a_filter(ctx, al):
    tgt, src, starts, kw = mixed_batch()
    starts = fill_starts(starts, 9)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        first = assert_batch(al, tc, sc, tgt, src, starts, singles=False, **kw)      # builds the k-NN grid itself
        one = register.icp(tc, sc, starts[1], return_pairs=True, **kw)                # a single call shrinks nothing the batch owns
        thin = tc.voxel_grid(0.2)
        kept = tc.statistical_outlier(8)
        again = register.icp_batch(tc, sc, starts, return_pairs=True, **kw)
        for a, b in zip(first, again):
            assert result_bytes(a) == result_bytes(b) and np.array_equal(a.idx, b.idx)
        assert result_bytes(one) == result_bytes(first[1]) and np.array_equal(one.idx, first[1].idx)
        small = register.icp_batch(tc, sc, starts[:2], return_pairs=True, **kw)       # fewer starts in the larger block
        assert [result_bytes(r) for r in small] == [result_bytes(r) for r in first[:2]]
        assert np.array_equal(tc.voxel_grid(0.2)["xyz"], thin["xyz"]) and np.array_equal(tc.statistical_outlier(8), kept)
        assert_batch(al, sc, tc, src, tgt, [s.inverse() for s in starts[:2]], singles=False, **kw)   # the other way round


def test_batch_refusals(ctx):
    tgt, src, starts, kw = mixed_batch()
    other = _lib.Context(0)
    try:
        with Cloud(tgt[:100], ctx=ctx) as a, Cloud(src[:50], ctx=ctx) as s, Cloud(src[:50], ctx=other) as b:
            bad = list(starts)
            bad[2] = Transform.make(scale=0.0)
            for call in (lambda: register.icp_batch(a, s, bad), lambda: register.icp_batch(a, s, []), lambda: register.icp_batch(a, s, fill_starts(starts, 1025)),
                         lambda: register.icp_batch(a, b, starts), lambda: register.icp_batch(a, s, starts, max_dist=0.0),
                         lambda: register.icp_batch(a, s, starts, min_pairs=2), lambda: register.icp_batch(a, s, starts, max_iters=-1)):
                with pytest.raises(_lib.SfmHipError, match="status -"):
                    call()
            assert len(register.icp_batch(a, s, fill_starts(starts, 1024), max_iters=1)) == 1024
    finally:
        other.close()


# ---------------------------------------------------------------- the vote
@pytest.mark.parametrize("samples", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_scale,n_yaw,bins", [(1, 1, 4), (3, 4, 64), (1, 72, 128), (3, 72, 64)])
def test_vote_bytes_for_the_cpu_shapes(ctx, al, n_scale, n_yaw, bins, samples):
    tgt = planted_plot()[:3000]
    src = moved_back(tgt[1::2], yaw_motion(90.0 if n_yaw == 4 else 0.0 if n_yaw == 1 else 35.0, 2.0, (3.0, -2.0)))
    o = stub_align_opts(al, scale_lo=2.0 if n_scale == 1 else 1.5, scale_hi=3.0, h_tol=0.3, n_scale=n_scale, n_yaw=n_yaw, bins=bins,
                        src_samples=samples, tgt_samples=max(samples - 1, 1) if samples == 64 else samples, n_cand=16)
    cands, st = vote_equal(al, ctx, tgt, src, LEVEL, Frame.make((0, 0, 1), (0.3, 1, 0), 0.001), o)
    if samples >= 63:
        assert len(cands) == min(16, n_scale * n_yaw) and cands[0].votes > 0


@pytest.mark.parametrize("tgt_samples", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_vote_bytes_around_the_tile(ctx, al, tgt_samples):
    tgt, src = planted_plot(), moved_back(planted_plot()[::3], yaw_motion(137.0, 2.3))
    n_above = stub_vote(al, tgt, src, LEVEL, LEVEL, stub_align_opts(al, **dict(GOOD, tgt_samples=8192)))[1].n_above_tgt
    z = tgt[:, 2].astype(np.float64)                                                   # exactly that many above: the top point (hmax
    above, top = np.flatnonzero(z >= 0.1 * z.max()), int(np.argmax(z))                 # stays), the first others, and all that is below
    keep = z < 0.1 * z.max()
    keep[np.concatenate([[top], above[above != top][:tgt_samples - 1]])] = True
    tgt = tgt[keep]
    o = stub_align_opts(al, scale_lo=1.5, scale_hi=3.5, h_tol=0.3, n_scale=3, n_yaw=12, bins=37, src_samples=300, tgt_samples=8192, n_cand=36)
    cands, st = vote_equal(al, ctx, tgt, src, LEVEL, LEVEL, o)
    assert st.n_tgt == tgt_samples < n_above and 150 < st.n_src <= 300 and len(cands) == 36


def test_vote_bytes_at_the_ceilings(ctx, al):
    """8 192 samples a side, 128 bins (68 KB of LDS), tilted frames, a source with NaN rows."""
    rng = np.random.default_rng(3)
    big = np.concatenate([planted_plot()] * 3) + rng.normal(size=(25500, 3)).astype(np.float32) * np.float32(0.02)
    M = Transform.make(yaw_motion(200.0, 0.45).rotation() @ np.array([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]]), [1.0, 2.0, 3.0], 0.45)
    src = moved_back(big[::2], M)
    src[[5, 77], [0, 2]] = [np.nan, np.inf]
    up = tuple(M.rotation().T @ [0, 0, 1.0])
    fs = Frame.make(up, (0.0, 1.0, 0.2), float(np.dot(up, moved_back(np.zeros((1, 3)), M)[0])))
    o = stub_align_opts(al, scale_lo=0.3, scale_hi=0.7, h_tol=0.3, n_scale=2, n_yaw=4, bins=128, src_samples=8192, tgt_samples=8192, n_cand=8)
    cands, st = vote_equal(al, ctx, big, src, LEVEL, fs, o)
    assert st.n_src > 4096 and st.n_tgt > 4096 and len(cands) == 8


def test_vote_edges_on_hand_made_points(ctx, al):
    o = stub_align_opts(al, scale_lo=1.0, scale_hi=1.0, h_tol=0.25, n_scale=1, n_yaw=4, bins=64, clear_rel=0.0, n_cand=8)
    tgt, src = mirrored_points()
    cands, _ = vote_equal(al, ctx, tgt[:2], src, LEVEL, LEVEL, o)                     # ties of peaks and of candidates
    assert [(c.votes, c.m, c.bin) for c in cands] == [(1, m, 32 * 64 + 16) for m in range(4)]
    high = tgt.copy()
    high[:, 2] = 1.25
    assert [(c.votes, c.bin) for c in vote_equal(al, ctx, high, src, LEVEL, LEVEL, o)[0]] == [(2, 32 * 64 + 48)] * 4   # |dh| == h_tol
    assert vote_equal(al, ctx, high, src, Frame.make(offset=-math.ulp(1.25)), LEVEL, o)[0] == []                         # one double beyond
    o.window_rel, o.n_yaw = 0.5, 1
    below = float(np.nextafter(np.float32(2), np.float32(0)))
    tgt, src = mirrored_points(below)
    assert [(c.votes, c.bin) for c in vote_equal(al, ctx, tgt, src, LEVEL, LEVEL, o)[0]] == [(1, 32 * 64)]               # 2 is outside
    assert [(c.votes, c.bin) for c in vote_equal(al, ctx, np.concatenate([tgt, tgt[2:]]), src, LEVEL, LEVEL, o)[0]] == [(2, 32 * 64 + 63)]
    assert vote_equal(al, ctx, tgt[1:2], src, LEVEL, LEVEL, o)[0] == []                                                     # W = 0


def test_empty_cases_and_refusals(ctx, al):
    tgt, src, _ = small_scene()
    o = stub_align_opts(al, **GOOD)
    under = tgt.copy()
    under[:, 2] = -np.abs(under[:, 2]) - 1
    nan = np.full((5, 3), np.nan, np.float32)
    for t, s in ((under, src), (tgt, under), (tgt[:0], src), (tgt, src[:0]), (nan, src), (tgt, nan)):
        with Cloud(t, ctx=ctx) as tc, Cloud(s, ctx=ctx) as sc:
            cands, st = assert_vote(al, tc, sc, t, s, LEVEL, LEVEL, o)
            assert cands == [] and st.flags == EMPTY
            res = register.align(tc, sc, LEVEL, LEVEL, opts=o)
            assert struct_bytes(res) == struct_bytes(stub_align(al, t, s, LEVEL, LEVEL, o)) and res.flags == EMPTY | NO_WINNER
    other = _lib.Context(0)
    try:
        with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc, Cloud(src, ctx=other) as oc:
            o.icp_dist_bins = 1e-9                                                    # candidates, and every start ends FEW
            res = register.align(tc, sc, LEVEL, LEVEL, opts=o)
            assert struct_bytes(res) == struct_bytes(stub_align(al, tgt, src, LEVEL, LEVEL, o)) and res.flags == NO_WINNER and res.n_cand == 4
            for call in (lambda: register.align_vote(tc, oc, LEVEL, LEVEL, **GOOD), lambda: register.align_vote(tc, tc, LEVEL, LEVEL, **GOOD),
                         lambda: register.align_vote(tc, sc, LEVEL, LEVEL), lambda: register.align(tc, sc, LEVEL, LEVEL, **dict(GOOD, bins=129)),
                         lambda: register.align(tc, sc, LEVEL, LEVEL, **dict(GOOD, h_tol=math.nan)),
                         lambda: register.align(tc, sc, Frame.make((0, 0, 1.1)), LEVEL, **GOOD),
                         lambda: register.align_vote(tc, sc, LEVEL, Frame.make((0, 0, 1), (0, 0, 1)), **GOOD),
                         lambda: register.align_vote(tc, sc, LEVEL, Frame.make(offset=math.inf), **GOOD)):
                with pytest.raises(_lib.SfmHipError, match="status -"):
                    call()
    finally:
        other.close()


# ---------------------------------------------------------------- the whole alignment
@pytest.mark.parametrize("name,scale,partial", [("yaw137", 2.3, True), ("yaw310", 0.45, False)])
def test_align_on_planted_motions(ctx, al, name, scale, partial):
    M = MOTIONS[name](scale)
    tgt, src = recovery_scene(M, partial)
    o = stub_align_opts(al, scale_lo=0.65 * scale, scale_hi=1.52 * scale, **RECOVERY)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        res = register.align(tc, sc, LEVEL, LEVEL, opts=o)
        assert struct_bytes(res) == struct_bytes(stub_align(al, tgt, src, LEVEL, LEVEL, o))
        assert res.flags == 0 and res.reg.pairs == res.stats.n_src and res.n_same >= 2
        assert abs(register.scale_guess(res.stats) / scale - 1) < 0.02
        t = register.align_last_timing(tc)
        assert 0 < t["vote"] < 5000 and 0 < t["icp"] < 5000 and t["vote"] + t["icp"] <= t["total"] < 10000
        fine = register.icp(tc, sc, res.reg.T, **FULL_ICP)                             # the caller's next step, from the winner
        truth = register.icp(tc, sc, M, **FULL_ICP)
        assert all(g <= 2 * w for g, w in zip(motion_errors(fine.T, M), motion_errors(truth.T, M)))
        plain = register.icp(tc, sc, None, **FULL_ICP)                                 # without it: nowhere near
        assert plain.flags != 0 or motion_errors(plain.T, M)[1] > 10.0


# ---------------------------------------------------------------- the host mirror
def test_align_selftest(ctx):
    exe = build.build_align_demo()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    steps = ["plots", "ground A", "ground B", "align", "register", "scale"]
    lines = [line.split(": ", 1) for line in r.stdout.splitlines() if line.split(": ", 1)[0] in steps]
    assert [k for k, _ in lines] == steps, r.stdout
    out = dict(lines)
    assert out["align"].startswith("flags 0 ") and " converged 1 flags 0 " in out["register"]
    assert abs(float(out["scale"].split()[0]) / 2.3 - 1) <= 1e-3
