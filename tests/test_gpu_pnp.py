"""GPU: sfmhip_pnp_ransac and sfmhip_pnp_epnp (csrc/pnp.hip) against the CPU build of the same header
(tests/stub/pnp_capi.cpp), bit for bit on every output: models, masks, iteration counts, flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pnp_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return S.build_stub(tmp_path_factory.mktemp("pnp"))


@pytest.fixture(scope="module")
def ctx():
    from sfm_danpipeline_amd import _lib
    return _lib.Context(0)


def _views(n_views, sizes, seed0):
    scs = [S.ransac_scene(seed0 + v, sizes[v % len(sizes)], S.DIST1) for v in range(n_views)]
    return [s["X"] for s in scs], [s["xy"] for s in scs], [s["thr"] for s in scs]


def _same(a, b):
    for k in ("rvec", "tvec", "rvec_ransac", "tvec_ransac", "rvec_refit", "tvec_refit"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    for k in ("status", "inliers", "iterations"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["masks"], b["masks"]))
    assert a["flags"] == b["flags"]


@pytest.mark.parametrize("n_views,sizes", [(1, [2000]), (8, [8, 40, 333, 1000, 5000, 5, 64, 257]), (64, [8, 50, 200, 700, 13, 256, 300])],
                         ids=["1view", "8views", "64views"])
def test_ransac_equals_the_cpu_build_bit_for_bit(L, ctx, n_views, sizes):
    from sfm_danpipeline_amd import pnp
    X, xy, thr = _views(n_views, sizes, 1000 * n_views)
    dev = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx)
    cpu = S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr)
    assert np.all(dev["status"] == 1)
    _same(dev, cpu)


def test_ransac_without_distortion_and_edges(L, ctx):
    from sfm_danpipeline_amd import pnp
    scs = [S.ransac_scene(50 + v, 900 if v != 3 else 120, S.DIST0) for v in range(5)]
    for v, n in enumerate([4, 0, 5]):                                   # too few, none, exactly the model's five
        scs[v] = dict(scs[v], X=scs[v]["X"][scs[v]["truth"] == 1][:n], xy=scs[v]["xy"][scs[v]["truth"] == 1][:n])
    plane = scs[3]["X"].copy()
    plane[:, 2] = 0.1                                                   # a coplanar view: every hypothesis is skipped
    X = [s["X"] for s in scs] + [plane]
    xy = [s["xy"] for s in scs] + [S.project(plane, scs[3]["R"], scs[3]["t"], S.K, S.DIST0)]
    thr = [3.0, 3.0, 3.0, scs[3]["thr"], scs[4]["thr"], 3.0]
    dev = pnp.pnp_ransac(X, xy, S.K, S.DIST0, thresholds=thr, max_iters=200, ctx=ctx)
    cpu = S.stub_ransac(L, X, xy, S.K, S.DIST0, thresholds=thr, max_iters=200)
    _same(dev, cpu)
    assert list(dev["status"]) == [-1, -1, 1, 1, 1, 0] and dev["flags"] & pnp.FLAG_RANK_DEFICIENT


def test_epnp_equals_the_cpu_build_bit_for_bit(L, ctx):
    from sfm_danpipeline_amd import pnp
    X, xyn = [], []
    for v, n in enumerate([5, 6, 10, 100, 255, 256, 257, 2000, 5000]):
        sc = S.scene(300 + v, n, S.DIST1, noise=0.3)
        X.append(sc["X"])
        xyn.append(S.normalise(sc["xy"], S.K, S.DIST1))
    plane = X[3].copy()
    plane[:, 0] = 0.0
    X.append(plane)
    xyn.append(xyn[3])
    R, t, fl = pnp.epnp(X, xyn, ctx=ctx)
    Rc, tc, flc = S.stub_epnp(L, X, xyn)
    assert np.array_equal(R.view(np.uint64), Rc.view(np.uint64)) and np.array_equal(t.view(np.uint64), tc.view(np.uint64))
    assert fl == flc and fl & pnp.FLAG_RANK_DEFICIENT and not np.any(R[-1])


def test_batch_independence_and_repeatability(ctx):
    from sfm_danpipeline_amd import pnp
    X, xy, thr = _views(7, [40, 77, 114, 600, 1500], 7000)
    batch = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx)
    again = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx)      # two consecutive calls on one context
    _same(batch, again)
    for v in range(7):
        alone = pnp.pnp_ransac([X[v]], [xy[v]], S.K, S.DIST1, thresholds=[thr[v]], ctx=ctx)
        for k in ("rvec", "tvec", "rvec_refit", "tvec_refit", "status", "inliers", "iterations"):
            assert np.array_equal(alone[k][0], batch[k][v]), (k, v)
        assert np.array_equal(alone["masks"][0], batch["masks"][v])


_POISON = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests import pnp_scenes as S
from sfm_danpipeline_amd import pnp
scs = [S.ransac_scene(7000 + v, [40, 77, 114, 600, 1500][v % 5], S.DIST1) for v in range(7)]
r = pnp.pnp_ransac([s["X"] for s in scs], [s["xy"] for s in scs], S.K, S.DIST1, thresholds=[s["thr"] for s in scs])
np.savez(sys.argv[2], **{k: r[k] for k in ("rvec", "tvec", "rvec_refit", "tvec_refit", "status", "inliers", "iterations")},
         mask=np.concatenate(r["masks"]), flags=r["flags"])
"""


def test_poisoned_allocations_give_equal_bits(ctx, tmp_path):
    """SFMHIP_POISON=1 fills fresh device memory with 0xFF: a kernel that read before it wrote would show"""
    from sfm_danpipeline_amd import pnp
    X, xy, thr = _views(7, [40, 77, 114, 600, 1500], 7000)
    ref = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx)
    script, out = tmp_path / "poison.py", tmp_path / "poison.npz"
    script.write_text(_POISON)
    subprocess.run([sys.executable, str(script), ROOT, str(out)], check=True, timeout=300, env=dict(os.environ, SFMHIP_POISON="1"))
    got = np.load(out)
    for k in ("rvec", "tvec", "rvec_refit", "tvec_refit", "status", "inliers", "iterations"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["mask"], np.concatenate(ref["masks"])) and int(got["flags"]) == ref["flags"]


# ---------------------------------------------------------------- the chunks, the job list, the keep batches, the edges
LONG_SHARES = [0.3, 0.65, 0.0, 0.5, 0.8, 0.55, 0.3, 0.6, 0.45, 0.7]
LONG_SIZES = [200, 300, 64, 257, 120, 200, 9, 513, 200, 150]
_ROWS = ("rvec", "tvec", "rvec_ransac", "tvec_ransac", "rvec_refit", "tvec_refit", "status", "inliers", "iterations")


@pytest.fixture(scope="module")
def long_batch(L):
    """ten views that leave ransac_replay in different chunks, and the stub's result for them (computed once)"""
    scs = [S.outlier_scene(2000 + v, LONG_SIZES[v], LONG_SHARES[v], S.DIST1) for v in range(10)]
    X, xy, thr = [s["X"] for s in scs], [s["xy"] for s in scs], [s["thr"] for s in scs]
    return X, xy, thr, S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr)


def _covers_every_chunk(its):
    """a condition on the inputs: the stub's iteration counts leave in each chunk of ransac_replay and reach the cap"""
    its = [int(i) for i in its]
    for lo, hi in ((0, 32), (32, 96), (96, 224), (224, 480)):
        assert any(lo < i <= hi for i in its), (lo, hi, its)
    assert any(480 < i < 992 for i in its) and any(i == 1000 for i in its), its


def _row_equals(alone, batch, v):
    for k in _ROWS:
        a, b = alone[k][0], batch[k][v]
        assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8)), (k, v)
    assert np.array_equal(alone["masks"][0], batch["masks"][v]), v


def test_long_runs_leave_in_every_chunk(L, ctx, long_batch):
    """Outlier shares of 0 to 80 % in one batch (stub: 25, 875, 2, 142, 1000, 247, 33, 450, 89, 1000 iterations): views
    leave after the 32-, 64-, 128- and each 256-chunk and two run to the 1000-iteration cap, which overshoots the sample
    table (992 -> 1248 drawn).  This runs, on the device, pnp_solve's t / chunk and the interleaved Mem<64> work area over
    many waves per job (chunk 64, 128, 256), pnp_count's jobs[slot / chunk], the Keep slot arithmetic at chunk > 64 and
    the shrinking job list, where job index != view index (thr2[jb.view], Keep{slot, view}, jb.samp).  Then every view
    alone against its row of the batch: batch independence with job != view."""
    from sfm_danpipeline_amd import pnp
    X, xy, thr, cpu = long_batch
    _covers_every_chunk(cpu["iterations"])
    assert sorted(set(cpu["status"].tolist())) == [0, 1]
    dev = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx)
    _same(dev, cpu)
    for v in range(10):
        alone = pnp.pnp_ransac([X[v]], [xy[v]], S.K, S.DIST1, thresholds=[thr[v]], ctx=ctx)
        _row_equals(alone, dev, v)


def test_long_runs_with_a_threshold_of_its_own_per_view(L, ctx, long_batch):
    """the same batch with view v's threshold times 1 + 0.1 v, and then with thresholds of 0.75 (1 + 0.1 v) px.  The first
    set stays seven noise sigmas above the inliers and twenty thresholds below the outliers, so no count depends on which
    view's threshold is read (a stub built with thr2[job] gave the same bits); the second lies inside the 0.5 px noise:
    once the job list has shrunk, thr2[job] instead of thr2[jb.view] in pnp_count scores a view against another view's
    threshold and changes its counts (the same mutant stub differed, and a library built with that mistake fails here).
    Asserted on the inputs: the tight set still leaves in every chunk, and the final model of at least five views counts
    differently under its neighbour's threshold."""
    from sfm_danpipeline_amd import pnp
    X, xy, thr, _ = long_batch
    for thr_v in ([t * (1 + 0.1 * v) for v, t in enumerate(thr)], [0.75 * (1 + 0.1 * v) for v in range(10)]):
        cpu = S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr_v)
        _covers_every_chunk(cpu["iterations"])
        _same(pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr_v, ctx=ctx), cpu)
    Kc, dc = np.ascontiguousarray(S.K.reshape(9)), np.ascontiguousarray(S.DIST1)
    sensitive = 0
    for v in range(1, 10):
        if cpu["status"][v] != 1:
            continue
        fx, fy = np.ascontiguousarray(X[v], np.float32), np.ascontiguousarray(xy[v], np.float32)
        model = np.ascontiguousarray(np.concatenate([cpu["rvec"][v], cpu["tvec"][v]]))
        own, other = (L.pnp_count(len(fx), fx.ctypes.data, fy.ctypes.data, Kc.ctypes.data, dc.ctypes.data, model.ctypes.data, t, None)
                      for t in (thr_v[v], thr_v[v - 1]))
        assert own == cpu["inliers"][v]
        sensitive += own != other
    assert sensitive >= 5


@pytest.mark.parametrize("n_views", [130, 65])
def test_more_keeps_than_one_launch_holds(L, ctx, n_views):
    """noise-free, outlier-free views of 6 to 45 points with a 3 px threshold: every view's first sample takes every point,
    so the first chunk carries one keep per view: 130 keeps go to pnp_keep_best as KeepBatch launches of 64 + 64 + 2, 65 as
    64 + 1 (DeviceBackend::keep_best's first = 64, 128)"""
    from sfm_danpipeline_amd import pnp
    scs = [S.scene(5000 + v, 6 + v % 40, S.DIST1) for v in range(n_views)]
    X, xy, thr = [s["X"] for s in scs], [s["xy"] for s in scs], [3.0] * n_views
    cpu = S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr)
    assert np.all(cpu["iterations"] == 1) and np.all(cpu["status"] == 1)
    assert cpu["inliers"].tolist() == [6 + v % 40 for v in range(n_views)]
    dev = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx)
    _same(dev, cpu)
    assert np.all(dev["iterations"] == 1)
    assert len({r.tobytes() for r in dev["rvec"]}) == n_views               # (every view kept its own model)


def _family_views(noise):
    views = []
    for name, f in list(S.FAMILIES.items()) + [("slab_1e-6", S.slab(1e-6)), ("slab_1e-7", S.slab(1e-7))]:
        for k, n in enumerate((5, 64, 257)):
            views.append((name, f(700 + k, n, S.DIST1, noise)))
    return views


def test_ransac_over_the_geometry_families(L, ctx):
    """one batch over tests/pnp_scenes.py's FAMILIES (a rotation of exactly pi and of pi - 1e-7, so rodrigues_to_vector's
    half-turn branch runs in pnp_solve and in the refit; R = I; near and far cameras; slabs down to 1e-5, solved but
    ill-conditioned, where a contracted FMA on one side would show) and the slabs 1e-6 (on the rank limit) and 1e-7 (past
    it), n in (5, 64, 257), 0.3 px noise.  The flags must be equal too: host and device must agree on which side of
    FLAG_RANK_DEFICIENT every sample falls."""
    from sfm_danpipeline_amd import pnp
    views = _family_views(0.3)
    X, xy = [s["X"] for _, s in views], [s["xy"] for _, s in views]
    cpu = S.stub_ransac(L, X, xy, S.K, S.DIST1)
    status = {(name, len(s["X"])): int(cpu["status"][i]) for i, (name, s) in enumerate(views)}
    assert all(status[(name, n)] == 1 for name in S.FAMILIES for n in (64, 257)), status
    assert status[("slab_1e-7", 257)] == 0 and cpu["flags"] & pnp.FLAG_RANK_DEFICIENT
    _same(pnp.pnp_ransac(X, xy, S.K, S.DIST1, ctx=ctx), cpu)


def test_epnp_over_the_geometry_families(L, ctx):
    """sfmhip_pnp_epnp (pnp_epnp_group) on the same families without noise, and on twenty 1e-6 slabs: the stub solves
    some and refuses others (asserted), and the device must refuse the same ones"""
    from sfm_danpipeline_amd import pnp
    scs = [s for _, s in _family_views(0.0)] + [S.slab(1e-6)(seed, 5 + seed, S.DIST1) for seed in range(20)]
    X, xyn = [s["X"] for s in scs], [S.normalise(s["xy"], S.K, S.DIST1) for s in scs]
    Rc, tc, flc = S.stub_epnp(L, X, xyn)
    refused = [not np.any(R) for R in Rc]
    n_fam = 3 * len(S.FAMILIES)
    assert not any(refused[:n_fam]) and all(refused[n_fam + 3:n_fam + 6]) and 0 < sum(refused[n_fam + 6:]) < 20
    assert flc == pnp.FLAG_RANK_DEFICIENT
    R, t, fl = pnp.epnp(X, xyn, ctx=ctx)
    assert np.array_equal(R.view(np.uint64), Rc.view(np.uint64)) and np.array_equal(t.view(np.uint64), tc.view(np.uint64))
    assert fl == flc


def test_options_off_their_defaults(L, ctx):
    """max_iters 0, 1, 2 and inside / at the edges of the first chunks, on a batch whose views would run 25 and 145
    iterations and one of exactly five points; every side of the confidence clamp; thresholds 0, 1e-6 and 1e6 as three
    views of one batch"""
    from sfm_danpipeline_amd import pnp
    scs = [S.ransac_scene(3, 300, S.DIST1), S.outlier_scene(0, 200, 0.5, S.DIST1), S.scene(9, 5, S.DIST1)]
    X, xy, thr = [s["X"] for s in scs], [s["xy"] for s in scs], [scs[0]["thr"], scs[1]["thr"], 3.0]
    for mi in (0, 1, 2, 31, 32, 33, 96, 97):
        cpu = S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr, max_iters=mi)
        assert cpu["iterations"].tolist() == [min(mi, 25), min(mi, 145), 0] and cpu["status"][2] == 1, mi
        _same(pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, max_iters=mi, ctx=ctx), cpu)
    its = []
    for conf in (-1.0, 0.0, 0.5, 0.9, 0.999, 1.0, 2.0):
        cpu = S.stub_ransac(L, X[:2], xy[:2], S.K, S.DIST1, thresholds=thr[:2], confidence=conf)
        its.append(int(cpu["iterations"][0]))
        _same(pnp.pnp_ransac(X[:2], xy[:2], S.K, S.DIST1, thresholds=thr[:2], confidence=conf, ctx=ctx), cpu)
    assert its[0] == its[1] == its[2] < its[3] < 25 < its[4] < its[5] == its[6] == 1000
    thr3 = [0.0, 1e-6, 1e6]
    cpu = S.stub_ransac(L, [X[0]] * 3, [xy[0]] * 3, S.K, S.DIST1, thresholds=thr3)
    assert cpu["status"].tolist() == [0, 0, 1] and cpu["iterations"].tolist() == [1000, 1000, 1] and cpu["inliers"][2] == 300
    _same(pnp.pnp_ransac([X[0]] * 3, [xy[0]] * 3, S.K, S.DIST1, thresholds=thr3, ctx=ctx), cpu)


def test_nonfinite_points(L, ctx):
    """a NaN, an Inf and a -Inf coordinate in rows that the first two samples draw, a view of nothing but NaN and a clean
    view in one batch: the device returns, refuses the same samples (flags 3) and gives the stub's bits"""
    from sfm_danpipeline_amd import pnp
    scs = [S.nonfinite_scene(L, bad)[0] for bad in (np.nan, np.inf, -np.inf)] + [S.ransac_scene(3, 300, S.DIST1)]
    X = [s["X"] for s in scs] + [np.full((300, 3), np.nan)]
    xy = [s["xy"] for s in scs] + [np.full((300, 2), np.nan)]
    thr = [s["thr"] for s in scs] + [3.0]
    cpu = S.stub_ransac(L, X, xy, S.K, S.DIST1, thresholds=thr)
    assert cpu["status"].tolist() == [1, 1, 1, 1, 0] and cpu["iterations"][4] == 1000
    assert cpu["flags"] == pnp.FLAG_RANK_DEFICIENT | pnp.FLAG_SVD_RANDOM
    _same(pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=ctx), cpu)


ERR_ARG = -3   # include/sfmhip.h: SFMHIP_ERR_ARG


class _Raw:
    """sfmhip_pnp_ransac through ctypes with every pointer in the caller's hand"""

    def __init__(self, X, xy, thr):
        from sfm_danpipeline_amd import pnp
        self.n, self.off, self.xyz, self.xy = pnp._pack(X, xy)
        self.thr = np.ascontiguousarray(thr, np.float64)
        self.K, self.dist = np.ascontiguousarray(S.K.reshape(9)), np.ascontiguousarray(S.DIST1)
        self.fresh()

    def fresh(self):
        m, total = max(self.n, 1), max(int(self.off[-1]), 1)
        self.out = dict(status=np.full(m, 77, np.int32), rvec=np.full((m, 3), 7.0), tvec=np.full((m, 3), 7.0),
                        rvec_ransac=np.full((m, 3), 7.0), tvec_ransac=np.full((m, 3), 7.0), rvec_refit=np.full((m, 3), 7.0),
                        tvec_refit=np.full((m, 3), 7.0), inliers=np.full(m, 77, np.int32), mask=np.full(total, 77, np.uint8),
                        iterations=np.full(m, 77, np.int32))
        return self

    def untouched(self):
        return all(np.all(a == (7.0 if a.dtype == np.float64 else 77)) for a in self.out.values())

    def call(self, ctx, null=(), **over):
        from sfm_danpipeline_amd._lib import lib
        a = dict(ctx=ctx.h, n_views=self.n, offsets=self.off.ctypes.data, xyz=self.xyz.ctypes.data, xy=self.xy.ctypes.data,
                 K=self.K.ctypes.data, dist=self.dist.ctypes.data, thresholds=self.thr.ctypes.data, confidence=0.99, max_iters=1000)
        a.update({k: v.ctypes.data for k, v in self.out.items()})
        a.update(over)
        a.update({k: None for k in null})
        order = ("ctx", "n_views", "offsets", "xyz", "xy", "K", "dist", "thresholds", "confidence", "max_iters", "status", "rvec", "tvec",
                 "rvec_ransac", "tvec_ransac", "rvec_refit", "tvec_refit", "inliers", "mask", "iterations")
        return lib().sfmhip_pnp_ransac(*[a[k] for k in order])


def test_c_abi_nullable_outputs_and_refusals(L, ctx):
    """sfmhip_pnp_ransac with each and all of the nullable outputs NULL (rvec_ransac, tvec_ransac, rvec_refit, tvec_refit,
    mask, iterations): the mandatory outputs are those of the full call.  SFMHIP_ERR_ARG, with nothing written, for
    n_views < 0, offsets[0] != 0, decreasing offsets, points NULL with a non-zero total, max_iters < 0 and each mandatory
    pointer NULL; sfmhip_pnp_epnp refuses a problem of 4 points, decreasing offsets and its NULL pointers; n_views == 0
    and n_problems == 0 are OK and write nothing."""
    from sfm_danpipeline_amd._lib import lib
    scs = [S.ransac_scene(60 + v, n, S.DIST1) for v, n in enumerate((120, 40, 5))]
    raw = _Raw([s["X"] for s in scs], [s["xy"] for s in scs], [s["thr"] for s in scs])
    assert raw.call(ctx) == 0
    full = {k: v.copy() for k, v in raw.out.items()}
    cpu = S.stub_ransac(L, [s["X"] for s in scs], [s["xy"] for s in scs], S.K, S.DIST1, thresholds=[s["thr"] for s in scs])
    assert np.array_equal(full["rvec"], cpu["rvec"]) and np.array_equal(full["mask"], np.concatenate(cpu["masks"]))
    optional = ("rvec_ransac", "tvec_ransac", "rvec_refit", "tvec_refit", "mask", "iterations")
    for null in [(k,) for k in optional] + [optional]:
        assert raw.fresh().call(ctx, null=null) == 0, null
        for k, v in raw.out.items():
            if k in null:
                assert np.all(v == (7.0 if v.dtype == np.float64 else 77)), (null, k)
            else:
                assert np.array_equal(v.view(np.uint8), full[k].view(np.uint8)), (null, k)
    bad_first, decreasing = raw.off.copy(), raw.off.copy()
    bad_first[0] = 1
    decreasing[1], decreasing[2] = raw.off[2], raw.off[1]
    refusals = [dict(n_views=-1), dict(offsets=bad_first.ctypes.data), dict(offsets=decreasing.ctypes.data), dict(max_iters=-1),
                dict(null=("xyz",)), dict(null=("xy",))]
    refusals += [dict(null=(k,)) for k in ("ctx", "offsets", "K", "dist", "thresholds", "status", "rvec", "tvec", "inliers")]
    for kw in refusals:
        assert raw.fresh().call(ctx, **kw) == ERR_ARG, kw
        assert raw.untouched(), kw
    assert raw.fresh().call(ctx, n_views=0) == 0 and raw.untouched()
    assert raw.fresh().call(ctx, n_views=0, null=("xyz", "xy")) == 0 and raw.untouched()
    # sfmhip_pnp_epnp
    X = [s["X"][s["truth"] == 1][:n] for s, n in zip(scs, (30, 4, 5))]
    xyn = [S.normalise(s["xy"][s["truth"] == 1][:n], S.K, S.DIST1) for s, n in zip(scs, (30, 4, 5))]
    off = np.array([0, 30, 34, 39], np.int32)
    xyz, uv = np.ascontiguousarray(np.concatenate(X)), np.ascontiguousarray(np.concatenate(xyn))
    R, t = np.full((3, 9), 7.0), np.full((3, 3), 7.0)

    def epnp(n=3, off=off, xyz=xyz.ctypes.data, uv=uv.ctypes.data, R=R.ctypes.data, t=t.ctypes.data, h=ctx.h):
        return lib().sfmhip_pnp_epnp(h, n, None if off is None else off.ctypes.data, xyz, uv, R, t)
    swapped = np.array([0, 34, 30, 39], np.int32)
    for kw in (dict(), dict(off=swapped), dict(n=-1), dict(off=None), dict(xyz=None), dict(uv=None), dict(R=None), dict(t=None), dict(h=None)):
        assert epnp(**kw) == ERR_ARG, kw                                     # (dict(): the middle problem has 4 points)
        assert np.all(R == 7.0) and np.all(t == 7.0)
    assert epnp(n=0) == 0 and np.all(R == 7.0) and np.all(t == 7.0)
    ok_off = np.array([0, 30], np.int32)
    assert epnp(n=1, off=ok_off) == 0 and not np.any(R[0] == 7.0) and np.all(R[1:] == 7.0)
    Rc, tc, _ = S.stub_epnp(L, X[:1], xyn[:1])
    assert np.array_equal(R[0], Rc[0].reshape(9)) and np.array_equal(t[0], tc[0])


def test_timing_on_gives_the_same_bits(ctx, long_batch):
    """with sfmhip_set_timing on, the events recorded around every chunk's kernels change nothing: the long batch gives
    the stub's bits, and sfmhip_pnp_last_timing three finite, non-negative numbers, the solver's above zero"""
    from sfm_danpipeline_amd import _lib, pnp
    X, xy, thr, cpu = long_batch
    timed = _lib.Context(0)
    try:
        timed.set_timing(True)
        dev = pnp.pnp_ransac(X, xy, S.K, S.DIST1, thresholds=thr, ctx=timed)
        ms = pnp.last_timing(timed)
    finally:
        timed.close()
    _same(dev, cpu)
    assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms) and ms[0] > 0
