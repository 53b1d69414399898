"""GPU: the cloud registration (csrc/register.hip) against the g++ build of the same header
(tests/stub/register_capi.cpp), byte for byte: the result struct, idx and d2.  Source sizes on both sides of a sum block and
over several, targets of 1 .. 200 000 points, the CPU file's scenes (nearest, the planted motions, the partial overlap, the
loop's edges), init given and not, NaN rows on both sides, a source farther away than max_dist, a target handle reused
around the family's other calls, two contexts, transform and concat against numpy and as inputs that never were on the host,
and the host mirror's self-test."""
import math
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, register
from sfm_danpipeline_amd.cloud import Cloud
from sfm_danpipeline_amd.register import DEGENERATE, FEW, Transform
from tests.test_register_cpu import (CENTRES, SCALE_ERR_MAX, icp_scene, least_max_dist, motion, moved_back, nearest_scene, partial_scene, planted_plot,  # noqa: F401
                                     result_bytes, rg, stub_nearest, stub_opts, stub_run)
from tests.test_trees_cpu import plot

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def show(r):
    return dict(R=list(r.T.R), t=list(r.T.t), scale=r.T.scale, it=r.iterations, pairs=r.pairs, conv=r.converged, flags=r.flags, mse=r.mse)


def assert_nearest(rg, tc, sc, tgt, src, T=None, max_dist=math.inf):
    want = stub_nearest(rg, tgt, src, T, max_dist)
    got = register.nearest(tc, sc, T, max_dist)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    return got


def assert_icp(rg, tc, sc, tgt, src, init=None, **kw):
    """One device call against the stub: the same bytes.  Returns the device's result."""
    want, widx = stub_run(rg, tgt, src, init, **kw)
    got = register.icp(tc, sc, init, return_pairs=True, **kw)
    assert result_bytes(got) == result_bytes(want), (show(got), show(want))
    assert np.array_equal(got.idx, widx)
    return got


def icp_equal(rg, ctx, tgt, src, init=None, **kw):
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        return assert_icp(rg, tc, sc, tgt, src, init, **kw)


@pytest.fixture(scope="module")
def big_plot():
    """200 000 points: the k-NN grid has several rows per ring."""
    xyz = plot(2, CENTRES, n_tree=40000, n_ground=80000)[0]
    xyz.setflags(write=False)
    return xyz


# ---------------------------------------------------------------- scene 1
@pytest.mark.parametrize("max_dist", [math.inf, 0.3])
@pytest.mark.parametrize("moved", [False, True])
def test_nearest_equals_the_stub(ctx, rg, max_dist, moved):
    tgt, src = nearest_scene()
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        idx, d2 = assert_nearest(rg, tc, sc, tgt, src, motion(5.0, 0.2, 1.1) if moved else None, max_dist)
        assert (idx[7:11] == -1).all() and np.isinf(d2[7:11]).all() and np.isfinite(d2[100:152]).all()
        if not moved and max_dist == math.inf:
            assert idx[200] == 450 and d2[200] == np.float32(0.0625)
            md = least_max_dist(d2[200])                            # kept at the bound, rejected one double below it, d2 kept
            assert register.nearest(tc, sc, None, md)[0][200] == 450
            assert_nearest(rg, tc, sc, tgt, src, None, math.nextafter(md, 0.0))
            assert register.nearest(tc, sc, None, math.nextafter(md, 0.0))[0][200] == -1
            same = assert_nearest(rg, tc, tc, tgt, tgt)              # source == target
            assert (same[0][np.isfinite(tgt).all(1)] >= 0).all()


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("n_src", [1, 255, 256, 257, 2834, 8191, 8192, 60000])   # (from 8 192 on the source is walked in cell order)
def test_source_sizes(ctx, rg, n_src):
    tgt = planted_plot()
    M = motion(4.0, 0.3, 1.04)
    rng = np.random.default_rng(n_src)
    pick = np.arange(0, 3 * n_src, 3) if 3 * n_src <= len(tgt) else rng.integers(0, len(tgt), n_src)
    src = moved_back(tgt[pick].astype(np.float64) + (rng.normal(size=(n_src, 3)) * 0.01 if n_src > 3000 else 0.0), M)
    res = icp_equal(rg, ctx, tgt, src, with_scale=1, max_dist=1.0)
    assert res.flags == (FEW if n_src == 1 else 0)
    if n_src >= 255:
        assert res.pairs == n_src and abs(res.T.scale / 1.04 - 1) < 1e-3 and (res.converged == 1 or n_src > 3000)
    icp_equal(rg, ctx, tgt, src, init=motion(3.5, 0.25, 1.04), max_iters=3)
    if n_src >= 8191:
        src = src.copy()
        src[[5, 4000], [0, 2]] = [np.nan, np.inf]                  # points without an image sort behind every cell
        with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
            assert_nearest(rg, tc, sc, tgt, src, M, 0.05)
            assert_nearest(rg, tc, sc, tgt, src)
            assert_icp(rg, tc, sc, tgt, src, with_scale=1, max_dist=1.0, max_iters=4)


@pytest.mark.parametrize("n", [1, 2, 3, 8500, 200000])
def test_target_sizes(ctx, rg, big_plot, n):
    tgt = big_plot if n == 200000 else planted_plot()[:n]
    M = motion(4.0, 0.3, 0.95)
    src = moved_back(big_plot[::70] if n == 200000 else planted_plot()[:2000:2], M)
    res = icp_equal(rg, ctx, tgt, src, with_scale=1)
    if n < 3:
        assert res.flags == DEGENERATE and res.iterations == 0 and res.pairs == len(src)   # every pair at one point, or on a line
    if n >= 8500:
        assert res.flags == 0 and res.converged == 1 and res.pairs == len(src) and abs(res.T.scale / 0.95 - 1) < 10 * SCALE_ERR_MAX
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        assert_nearest(rg, tc, sc, tgt, src, M, 0.5)
        assert_nearest(rg, tc, sc, tgt, src)


# ---------------------------------------------------------------- scenes 3, 4, 5
@pytest.mark.parametrize("deg,tr,scale,max_dist", [(2.0, 0.1, None, 1.0), (4.0, 0.3, 1.04, math.inf), (8.0, 0.5, 0.95, 1.0)])
def test_planted_motions(ctx, rg, deg, tr, scale, max_dist):
    tgt, src, M = icp_scene(deg, tr, scale or 1.0)
    res = icp_equal(rg, ctx, tgt, src, with_scale=int(scale is not None), max_dist=max_dist)
    assert res.converged == 1 and res.pairs == len(src) and res.iterations <= 30 and abs(res.T.scale / M.scale - 1) <= SCALE_ERR_MAX


@pytest.mark.parametrize("scale,max_dist", [(None, 0.5), (1.04, 1.0)])
def test_partial_overlap(ctx, rg, scale, max_dist):
    tgt, src, M, n_own = partial_scene(4.0, 0.3, scale or 1.0)
    res = icp_equal(rg, ctx, tgt, src, with_scale=int(scale is not None), max_dist=max_dist)
    assert res.converged == 1 and res.pairs == n_own == 1541


def test_loop_edges_init_and_nan_rows(ctx, rg):
    tgt, src, M = icp_scene(4.0, 0.3, 1.0)
    tgt, src = tgt.copy(), src.copy()
    tgt[[5, 600, 8499]] = np.nan                                   # NaN rows on both sides
    src[[0, 77, 2833], [0, 1, 2]] = np.nan
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        full = assert_icp(rg, tc, sc, tgt, src)
        assert full.converged == 1 and full.pairs == len(src) - 3
        assert assert_icp(rg, tc, sc, tgt, src, max_iters=0).iterations == 0
        assert assert_icp(rg, tc, sc, tgt, src, max_iters=1).iterations == 1
        assert assert_icp(rg, tc, sc, tgt, src, max_iters=full.iterations - 2).converged == 0
        assert assert_icp(rg, tc, sc, tgt, src, eps=1e-2).converged == 2
        assert assert_icp(rg, tc, sc, tgt, src, init=M).iterations <= 3            # init given
        assert assert_icp(rg, tc, sc, tgt, src, init=motion(3.0, 0.2, 1.0), with_scale=1, max_dist=0.8).flags == 0
        same = assert_icp(rg, tc, tc, tgt, tgt)                                       # source == target
        assert (same.iterations, same.converged, same.pairs) == (1, 1, len(tgt) - 3)
        with Cloud(src[:0], ctx=ctx) as empty, Cloud(np.full((3, 3), np.nan, np.float32), ctx=ctx) as nan3:
            for t, s, ta, sa in ((tc, empty, tgt, src[:0]), (empty, sc, tgt[:0], src), (nan3, sc, np.full((3, 3), np.nan), src),
                                 (tc, nan3, tgt, np.full((3, 3), np.nan))):
                res = assert_icp(rg, t, s, ta, sa)
                assert res.flags == FEW and res.pairs == 0 and math.isnan(res.mse)
                assert register.nearest(t, s)[0].tolist() == [-1] * s.n
        line = np.outer(np.arange(40, dtype=np.float32), np.array([1.0, 2.0, -1.0], np.float32))
    assert icp_equal(rg, ctx, line, line + np.float32(0.01)).flags == DEGENERATE


def test_source_beyond_max_dist_has_no_pairs(ctx, rg, big_plot):
    src = planted_plot()[::3] + np.array([60.0, 0.0, 0.0], np.float32)    # the gap to the target's box: over 30
    for tgt in (planted_plot(), big_plot):
        res = icp_equal(rg, ctx, tgt, src, max_dist=0.5)
        assert res.flags == FEW and res.pairs == 0 and res.iterations == 0 and math.isnan(res.mse)


# ---------------------------------------------------------------- the handle
def test_target_handle_reused_around_the_other_calls(ctx, rg):
    tgt, src, M = icp_scene(2.0, 0.1, 1.04)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        first = assert_icp(rg, tc, sc, tgt, src, with_scale=1)                       # before them: builds the k-NN grid itself
        knn = tc.knn(4)
        thin = tc.voxel_grid(0.2)
        kept = tc.statistical_outlier(8)
        again = assert_icp(rg, tc, sc, tgt, src, with_scale=1)
        assert result_bytes(again) == result_bytes(first)
        assert_nearest(rg, tc, sc, tgt, src, M)
        assert np.array_equal(tc.knn(4)[0], knn[0]) and np.array_equal(tc.voxel_grid(0.2)["xyz"], thin["xyz"])
        assert np.array_equal(tc.statistical_outlier(8), kept)
        assert_icp(rg, sc, tc, src, tgt, with_scale=1, max_dist=1.0)                 # and the other way round: both hold a state


def test_two_contexts_and_bad_arguments_are_refused(ctx, rg):
    tgt, src, _ = icp_scene(2.0, 0.1, 1.0)
    other = _lib.Context(0)
    try:
        with Cloud(tgt[:100], ctx=ctx) as a, Cloud(src[:50], ctx=other) as b, Cloud(src[:50], ctx=ctx) as s:
            for call in (lambda: register.icp(a, b), lambda: register.nearest(a, b), lambda: register.concat(a, b),
                         lambda: register.icp(a, s, max_dist=0.0), lambda: register.icp(a, s, max_dist=math.nan),
                         lambda: register.icp(a, s, eps=-1.0), lambda: register.icp(a, s, max_iters=-1), lambda: register.icp(a, s, min_pairs=2),
                         lambda: register.icp(a, s, init=Transform.make(scale=0.0)), lambda: register.nearest(a, s, Transform.make(t=[0, math.nan, 0])),
                         lambda: register.nearest(a, s, None, -1.0), lambda: register.transform(a, Transform.make(scale=math.inf))):
                with pytest.raises(_lib.SfmHipError, match="status -"):
                    call()
            assert register.icp(a, s).flags in (0, FEW)
    finally:
        other.close()


# ---------------------------------------------------------------- transform and concat
def test_transform_and_concat_stay_on_the_device(ctx, rg):
    tgt, src, M = icp_scene(4.0, 0.3, 1.04)
    src = src.copy()
    src[[3, 9], [1, 2]] = [np.nan, np.inf]
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        moved = register.transform(sc, M)
        want = M.apply(src)
        want[[3, 9]] = src[[3, 9]]                                                   # a non-finite point stays as it is
        assert moved.xyz is None and np.array_equal(bits(moved.download()), bits(want))
        both = register.concat(tc, register.transform(sc, M))
        assert both.xyz is None and both.n == len(tgt) + len(src)
        cat = np.concatenate([tgt, want])
        with Cloud(cat, ctx=ctx) as up:                                              # the same calls on an uploaded copy
            a, b = both.voxel_grid(0.25, return_cloud=True), up.voxel_grid(0.25, return_cloud=True)
            assert np.array_equal(bits(a["xyz"]), bits(b["xyz"])) and np.array_equal(a["voxel_of"], b["voxel_of"])
            ra = register.icp(both, a["cloud"], return_pairs=True, max_iters=2)
            rb = register.icp(up, b["cloud"], return_pairs=True, max_iters=2)
            assert result_bytes(ra) == result_bytes(rb) and np.array_equal(ra.idx, rb.idx)
            assert_icp(rg, both, a["cloud"], cat, a["xyz"], max_iters=2)
        assert np.array_equal(bits(both.download()), bits(cat))
        with Cloud(src[:0], ctx=ctx) as empty:
            assert register.concat(empty, empty).n == 0 and register.transform(empty, M).n == 0
            assert np.array_equal(bits(register.concat(empty, sc).download()), bits(src))


def test_timing_is_reported_when_on(ctx):
    tgt, src, _ = icp_scene(2.0, 0.1, 1.0)
    with Cloud(tgt, ctx=ctx) as tc, Cloud(src, ctx=ctx) as sc:
        ctx.set_timing(True)
        try:
            res = register.icp(tc, sc)
            t = register.last_timing(tc)
        finally:
            ctx.set_timing(False)
        assert t["iterations"] == res.iterations and all(0 < t[k] < 5000 for k in ("search", "sums", "update"))
        register.icp(tc, sc, max_iters=1)
        assert register.last_timing(tc) == dict(search=0.0, sums=0.0, update=0.0, iterations=1)


# ---------------------------------------------------------------- the host mirror
def test_registration_selftest(ctx):
    exe = build.build_registration_demo()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    steps = ["plots", "register", "scale", "transform", "concat", "voxel grid", "estimatePlot"]
    lines = [line.split(": ", 1) for line in r.stdout.splitlines() if line.split(": ", 1)[0] in steps]
    assert [k for k, _ in lines] == steps, r.stdout
    out = dict(lines)
    assert abs(float(out["scale"].split()[0]) / 1.04 - 1) <= SCALE_ERR_MAX
    assert " converged 1 flags 0 " in out["register"] and out["plots"] == "A 82000 B 41000" and out["concat"] == "123000 points"
    assert out["estimatePlot"].startswith("status 0 trees ")
