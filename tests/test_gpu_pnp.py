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
