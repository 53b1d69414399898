"""GPU: the second registration entry (csrc/register.hip, DESIGN.md f-22: point-to-plane, trimmed and one-to-one ICP) against the
g++ build of the same header (tests/stub/register_icp_capi.cpp), byte for byte: the result struct and idx.  Source sizes on both
sides of a sum block and of the cell-order threshold, targets of 1, 3 and 8 500 points, both metrics with every rejector, metric
0 without rejectors against sfmhip_cloud_register on the device (single calls and batches), the four looping entries against the
bytes frozen from the commit before they shared one loop (tests/golden/register_parent.npz), batches with a start that stops at
once and one that runs to the limit, a target handle reused around the family's other calls, the timing call, and the host mirror's self-test."""
import math
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, register
from sfm_danpipeline_amd.cloud import Cloud
from sfm_danpipeline_amd.register import FEW, Transform
from tests.test_align_cpu import GOOD, LEVEL
from tests.test_register_cpu import icp_scene, motion, moved_back, planted_plot, result_bytes
from tests.test_register_icp_cpu import (batch_inits, frozen_cases, frozen_hash, frozen_mismatch, ig, plane_kw, plot_normals, stems_scene,  # noqa: F401
                                         stub_icp, stub_icp_batch, yaw_motion)

pytestmark = pytest.mark.gpu


def show(r):
    return dict(R=list(r.T.R), t=list(r.T.t), scale=r.T.scale, it=r.iterations, pairs=r.pairs, conv=r.converged, flags=r.flags, mse=r.mse,
                plane=r.plane_mse, tau=r.trim_d2)


def assert_icp(ig, tc, sc, tgt, src, nrm=None, init=None, **kw):
    """One device call against the stub: the same bytes.  Returns the device's result."""
    want, widx = stub_icp(ig, tgt, src, nrm, init, **kw)
    got = register.icp_ex(tc, sc, nrm, init, return_pairs=True, **kw)
    assert result_bytes(got) == result_bytes(want), (kw, show(got), show(want))
    assert np.array_equal(got.idx, widx), kw
    return got


def option_grid(n_live):
    """Both metrics, each with one-to-one on and off, trim 1 and 0.5, and trim 1 / N."""
    for metric in (0, 1):
        base = plane_kw(with_scale=1) if metric else dict(with_scale=1)
        for o2o in (0, 1):
            for trim in (1.0, 0.5):
                yield dict(base, one_to_one=o2o, trim=trim)
        yield dict(base, trim=1.0 / max(n_live, 1))
        yield dict(base, trim=1.0 / max(n_live, 1), one_to_one=1)


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("n_src", [1, 255, 256, 257, 8191, 8192, 20000])   # (the sum block's edges; from 8 192 on the source is walked in cell order)
def test_source_sizes(ctx, ig, n_src):
    tgt, nrm = planted_plot(), plot_normals()
    M = motion(2.0, 0.1, 1.04)
    rng = np.random.default_rng(n_src)
    pick = np.arange(0, 3 * n_src, 3) if 3 * n_src <= len(tgt) else rng.integers(0, len(tgt), n_src)
    src = moved_back(tgt[pick].astype(np.float64) + (rng.normal(size=(n_src, 3)) * 0.01 if n_src > 3000 else 0.0), M)
    if n_src >= 8191:
        src = src.copy()
        src[[5, 4000], [0, 2]] = [np.nan, np.inf]                  # points without an image
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        for kw in option_grid(n_src):
            res = assert_icp(ig, tc, sc, tgt, src, nrm, max_dist=1.0, max_iters=3, **kw)
            if n_src == 1:
                assert res.flags == FEW
            elif kw["trim"] == 0.5 and not kw.get("one_to_one"):
                assert res.flags == 0 and 0 < res.pairs < n_src and math.isfinite(res.trim_d2)   # (the trim cut something)
        if n_src >= 255:
            full = assert_icp(ig, tc, sc, tgt, src, nrm, **plane_kw(with_scale=1, max_dist=1.0))
            assert full.converged == 2 and abs(full.T.scale / 1.04 - 1) < 1e-3


@pytest.mark.parametrize("n", [1, 3, 8500])
def test_target_sizes(ctx, ig, n):
    tgt, nrm = planted_plot()[:n], plot_normals()[:n]
    src = moved_back(planted_plot()[:2000:2], motion(2.0, 0.1, 1.0))
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        for kw in option_grid(len(src)):
            res = assert_icp(ig, tc, sc, tgt, src, nrm, max_iters=3, **dict(kw, with_scale=0, min_pairs=6 if kw.get("metric") else 3))
            if kw.get("one_to_one"):
                assert res.pairs <= n
        assert_icp(ig, tc, sc, tgt, src, nrm[:, :3].copy(), **plane_kw(max_iters=2))     # stride 3


# ---------------------------------------------------------------- metric 0 without rejectors is sfmhip_cloud_register
@pytest.mark.parametrize("scene", ["planted", "partial", "edges"])
def test_metric_0_without_rejectors_equals_register_on_the_device(ctx, ig, scene):
    tgt, src, M = icp_scene(4.0, 0.3, 1.04)
    kw = dict(with_scale=1)
    if scene == "partial":
        src, kw = np.concatenate([src[tgt[::3, 0] < 1], np.float32([0, 0, 13]) + src[:300]]), dict(with_scale=1, max_dist=0.8)
    if scene == "edges":
        tgt, src = tgt.copy(), src.copy()
        tgt[[5, 600]] = np.nan
        src[[0, 77], [0, 1]] = np.nan
        kw = dict(eps=1e-2)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        for init in (None, motion(3.0, 0.2, 1.0)):
            for extra in (dict(), dict(max_iters=0), dict(max_iters=2)):
                old = register.icp(tc, sc, init, return_pairs=True, **kw, **extra)
                new = assert_icp(ig, tc, sc, tgt, src, None, init, **kw, **extra)
                assert result_bytes(new)[:len(result_bytes(old))] == result_bytes(old) and np.array_equal(new.idx, old.idx)
                assert math.isnan(new.plane_mse) and new.trim_d2 == math.inf
        big = np.concatenate([src] * 4)[:8192 + 100]               # the cell-ordered walk too
        with Cloud(big, ctx=ctx) as bc:
            old = register.icp(tc, bc, return_pairs=True, max_iters=2, **kw)
            new = register.icp_ex(tc, bc, return_pairs=True, max_iters=2, **kw)
            assert result_bytes(new)[:len(result_bytes(old))] == result_bytes(old) and np.array_equal(new.idx, old.idx)


def test_icp_batch_without_rejectors_equals_register_batch_on_the_device(ctx):
    """The batch form of the equality above: both are the one loop, the second narrowed to f-17's result."""
    tgt, nrm, src, M = stems_scene()
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        for n_init in (1, 2, 5):
            inits = batch_inits()[:n_init]                        # the second starts at t = (300, 0, 0): FEW at k = 0
            for kw in (dict(max_dist=1.0), dict(max_dist=1.0, with_scale=1, max_iters=3), dict(max_dist=1.0, eps=1e-3)):
                old = register.icp_batch(tc, sc, inits, return_pairs=True, **kw)
                new = register.icp_ex_batch(tc, sc, inits, return_pairs=True, **kw)
                assert len(old) == len(new) == n_init
                for b in range(n_init):
                    assert result_bytes(new[b])[:len(result_bytes(old[b]))] == result_bytes(old[b]), (n_init, kw, b, show(new[b]))
                    assert np.array_equal(new[b].idx, old[b].idx), (n_init, kw, b)
                    assert math.isnan(new[b].plane_mse) and new[b].trim_d2 == math.inf
                if n_init > 1:
                    assert old[1].flags == FEW and old[1].iterations == 0 and (old[1].idx == -1).all()


# ---------------------------------------------------------------- the frozen record
def device_run(tc, sc, entry, nrm, starts, kw):
    """One frozen case on the device: (the result structs' bytes, idx)."""
    if entry == "f17":
        res = register.icp(tc, sc, starts, return_pairs=True, **kw)
    elif entry == "icp":
        res = register.icp_ex(tc, sc, nrm, starts, return_pairs=True, **kw)
    else:
        rows = (register.icp_batch(tc, sc, starts, return_pairs=True, **kw) if entry == "f17_batch" else
                register.icp_ex_batch(tc, sc, starts, nrm, return_pairs=True, **kw))
        return b"".join(result_bytes(r) for r in rows), np.stack([r.idx for r in rows])
    return result_bytes(res), res.idx


def test_device_equals_the_frozen_record(ctx):
    """The device against the parent's bytes: one f-17 single call, the f-17 batch, every rejector combination at metric 0 and 1 and
    the two f-22 batches; each at most 6 iterations on a few thousand points."""
    chosen = [c for c in frozen_cases() if c[0] in ("f17 | icp_scene | no init | max_iters=2", "f17_batch | stems | short")
              or (c[1] == "icp" and c[0].endswith("| short")) or c[1] == "icp_batch"]
    assert len(chosen) == 11 and all(c[6].get("max_iters", 50) <= 6 for c in chosen)
    bad = []
    for name, entry, tgt, src, nrm, starts, kw in chosen:
        with Cloud(np.ascontiguousarray(tgt, np.float32), ctx=ctx) as tc, Cloud(np.ascontiguousarray(src, np.float32), ctx=ctx) as sc:
            res, idx = device_run(tc, sc, entry, nrm, starts, kw)
        bad.append(frozen_mismatch(name, frozen_hash(tgt, src, nrm, starts, kw), res, idx))
    assert not any(bad), [b for b in bad if b]


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("n_init", [1, 2, 5])
def test_batch_rows_equal_the_single_runs(ctx, ig, n_init):
    tgt, nrm, src, M = stems_scene()
    far = Transform.make(t=[300.0, 0, 0])                          # stops at k = 0: FEW
    inits = [Transform.make(), far, motion(1.0, 0.05), M, yaw_motion(2.0, (0.2, -0.1, 0.0))][:n_init]
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        for kw in (plane_kw(max_dist=1.0, trim=0.8, one_to_one=1, max_iters=6), dict(max_dist=1.0, trim=0.8, max_iters=4),
                   plane_kw(max_dist=1.0, eps=1e-3), dict(max_dist=1.0, one_to_one=1)):
            want, widx = stub_icp_batch(ig, tgt, src, inits, nrm, **kw)
            got = register.icp_ex_batch(tc, sc, inits, nrm, return_pairs=True, **kw)
            for b in range(n_init):
                assert result_bytes(got[b]) == result_bytes(want[b]) and np.array_equal(got[b].idx, widx[b]), (kw, b, show(got[b]), show(want[b]))
                one = register.icp_ex(tc, sc, nrm, inits[b], return_pairs=True, **kw)
                assert result_bytes(one) == result_bytes(got[b]) and np.array_equal(one.idx, got[b].idx), (kw, b)
            if "max_iters" in kw:
                assert got[0].iterations == kw["max_iters"] and got[0].converged == 0 and got[0].flags == 0   # ran to the limit
            if n_init > 1:
                assert got[1].flags == FEW and got[1].iterations == 0 and (got[1].idx == -1).all()
        plane = register.icp_plane_batch(tc, sc, inits, nrm, max_dist=1.0, eps=1e-6)
        assert [result_bytes(r) for r in plane] == [result_bytes(register.icp_plane(tc, sc, nrm, i, max_dist=1.0, eps=1e-6)) for i in inits]


# ---------------------------------------------------------------- the handle
def test_target_handle_reused_around_the_other_calls(ctx, ig):
    tgt, nrm, src, M = stems_scene()
    kw = plane_kw(max_dist=1.0, trim=0.9, one_to_one=1)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        first = assert_icp(ig, tc, sc, tgt, src, nrm, **kw)           # before them: builds the k-NN grid itself
        knn = tc.knn(4)
        old = register.icp(tc, sc, return_pairs=True, max_dist=1.0)
        vote = register.align_vote(tc, sc, LEVEL, LEVEL, **GOOD)
        again = assert_icp(ig, tc, sc, tgt, src, nrm, **kw)
        assert result_bytes(again) == result_bytes(first)
        assert np.array_equal(tc.knn(4)[0], knn[0])
        older = register.icp(tc, sc, return_pairs=True, max_dist=1.0)
        assert result_bytes(older) == result_bytes(old) and np.array_equal(older.idx, old.idx)
        assert len(register.align_vote(tc, sc, LEVEL, LEVEL, **GOOD)[0]) == len(vote[0])
        assert_icp(ig, tc, sc, tgt, src, nrm, **plane_kw(max_dist=1.0))                # a smaller state after a larger one
        own = tc.normals(10)                                           # normals=None: the cloud's own, [n, 4]
        assert result_bytes(register.icp_plane(tc, sc, max_dist=1.0, eps=1e-6, k=10)) == result_bytes(
            register.icp_plane(tc, sc, own, max_dist=1.0, eps=1e-6))
        assert_icp(ig, sc, tc, src, tgt, None, trim=0.5, max_dist=1.0, max_iters=3)    # the other way round: both hold a state


def test_bad_arguments_are_refused(ctx):
    tgt, nrm, src, M = stems_scene()
    other = _lib.Context(0)
    try:
        with Cloud(tgt[:100], ctx=ctx) as a, Cloud(src[:50], ctx=other) as b, Cloud(src[:50], ctx=ctx) as s:
            n = nrm[:100]
            for call in (lambda: register.icp_ex(a, b), lambda: register.icp_ex(a, s, trim=0.0), lambda: register.icp_ex(a, s, trim=1.5),
                         lambda: register.icp_ex(a, s, trim=math.nan), lambda: register.icp_ex(a, s, metric=2), lambda: register.icp_ex(a, s, one_to_one=2),
                         lambda: register.icp_ex(a, s, min_pairs=2), lambda: register.icp_ex(a, s, max_dist=0.0),
                         lambda: register.icp_plane(a, s, n, eps=0.0), lambda: register.icp_plane(a, s, n, min_pairs=5),
                         lambda: register.icp_plane(a, s, n, with_scale=1, min_pairs=6), lambda: register.icp_plane(a, s, n, init=Transform.make(scale=0.0)),
                         lambda: register.icp_plane_batch(a, s, [], n), lambda: register.icp_ex_batch(a, s, [Transform.make(t=[math.nan, 0, 0])])):
                with pytest.raises(_lib.SfmHipError, match="status -"):
                    call()
            assert register.icp_plane(a, s, n).flags in (0, FEW, 2)
    finally:
        other.close()


def test_timing_is_zero_while_off_and_reported_when_on(ctx):
    tgt, nrm, src, M = stems_scene()
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        assert register.icp_last_timing(tc) == dict(search=0.0, rejectors=0.0, sums=0.0, update=0.0, iterations=0)
        res = register.icp_plane(tc, sc, nrm, max_dist=1.0, eps=1e-6, trim=0.9)
        assert register.icp_last_timing(tc) == dict(search=0.0, rejectors=0.0, sums=0.0, update=0.0, iterations=res.iterations)
        ctx.set_timing(True)
        try:
            timed = register.icp_plane(tc, sc, nrm, max_dist=1.0, eps=1e-6, trim=0.9)
            t = register.icp_last_timing(tc)
        finally:
            ctx.set_timing(False)
        assert result_bytes(timed) == result_bytes(res)
        assert t["iterations"] == res.iterations and all(0 < t[k] < 5000 for k in ("search", "rejectors", "sums", "update"))


# ---------------------------------------------------------------- the host mirror
def test_registration_selftest_icp(ctx):
    exe = build.build_registration_demo()
    r = subprocess.run([exe, "--icp"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = dict(line.split(": ", 1) for line in r.stdout.splitlines() if ": " in line)
    assert out["plots"] == "A 82000 B 41000"
    for key in ("plane", "plane trimmed", "plane one-to-one", "registerCloud"):
        assert key in out, r.stdout
    assert " flags 0 " in out["plane"] and " converged 2 " in out["plane"]
    assert abs(float(out["registerCloud"].split()[0]) / 1.04 - 1) <= 1e-6
