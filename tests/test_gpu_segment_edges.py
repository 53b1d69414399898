"""GPU: csrc/segment.hip at the smallest shapes its kernels can break at (the scenes: tests/segment_scenes.py) -- every parity of k
and of the list length in seg_knn's two-slots-per-lane list, exact ties, rings that stay empty and a grid one cell thick, labels
that travel a whole chain against index order, the rule scenes built by hand, the segment tables' sort widths, cap and truncated
means, and the lists with no or one finite point.  Every case is compared bit for bit with the CPU build of the same header
(tests/stub/segment_capi.cpp) AND with the independent reference tests/test_segment_cpu.py checks that stub against (the literal
twin on untied scenes, numpy's brute force on tied ones); the propagation rounds, which the atomics' order decides, only have to
lie in 1 .. m + 1."""
import functools
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import cloud, segment
from tests import segment_scenes as scenes
from tests.test_segment_cpu import (K_GROW, K_SWEEP, STUB, brute_knn, check_expectation, check_knn, load_stub, ref_opts,
                                    reference_segmentation, stub_grow, stub_segment, stub_subset_knn, sweep_lengths, twin_knn, ubits,
                                    with_holes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("segment_edges") / "libsegmentcapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


@functools.lru_cache(maxsize=None)
def built(name, *args):
    """A scene of tests/segment_scenes.py, built once for the module."""
    return getattr(scenes, name)(*args)


def device_knn_equals(c, sc, xyz, ind, k, knn=twin_knn):
    idx, d2 = segment.subset_knn(c, ind, k)
    si, sd = stub_subset_knn(sc, xyz, ind, k)
    assert np.array_equal(idx, si) and np.array_equal(ubits(d2), ubits(sd))          # the stub, bit for bit
    check_knn((idx, d2), xyz, ind, k, knn)                                           # the independent reference
    return idx, d2


def device_whole(c, rgb, ind, kw):
    seg, ns, rounds = segment.grow(c, rgb, ind, segment.default_opts(**kw))
    labels, nc, st = segment.segment_rgb(c, rgb, ind, segment.default_opts(**kw))
    assert 1 <= rounds <= len(ind) + 1 and 1 <= st.rounds <= len(ind) + 1
    return dict(seg=seg, ns=ns, labels=labels, nc=nc, stats=[st.n_idx, st.n_segments, st.n_regions])


def same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("seg", "ns", "labels", "nc", "stats"))


def device_equals(c, sc, xyz, rgb, ind, kw, tied=False, ref=None):
    """The subset k-NN, the growth and the whole call on handle `c` against the stub and against the reference (`ref`: one that
    was computed before, for the same scene and options)."""
    o = ref_opts(**kw)
    device_knn_equals(c, sc, xyz, ind, o["region_neighbour_number"], brute_knn if tied else twin_knn)
    got = device_whole(c, rgb, ind, kw)
    sseg, sns = stub_grow(sc, xyz, rgb, ind, o)
    slabels, snc, sstats, _ = stub_segment(sc, xyz, rgb, ind, o)
    assert same(got, dict(seg=sseg, ns=sns, labels=slabels, nc=snc, stats=list(sstats[:3])))
    ref = ref or reference_segmentation(xyz, rgb, ind, o, tied)
    assert got["ns"] == ref[1] and np.array_equal(got["seg"], ref[0]) and got["nc"] == ref[3] and np.array_equal(got["labels"], ref[2])
    return got


# ---------------------------------------------------------------- 1. every parity of k and of the list length
@pytest.mark.parametrize("k", K_SWEEP)
def test_k_sweep(ctx, sc, k):
    xyz, rgb, ind, kw = built("untied_sheet", 300)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        for m in sweep_lengths(k):
            idx, d2 = device_knn_equals(c, sc, xyz, ind[:m], k)
            assert (idx[:, :min(k, m)] >= 0).all() and (idx[:, min(k, m):] == -1).all() and np.isinf(d2[:, min(k, m):]).all()
        if k in K_GROW:
            got = device_equals(c, sc, xyz, rgb, ind, dict(kw, region_neighbour_number=k, neighbour_number=min(30, k)))
            assert got["ns"] > 7


# ---------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("k", [3, 27, 64, 101])
def test_ties_on_a_lattice(ctx, sc, k):
    xyz, rgb, ind, kw = built("lattice", 6, 6, 3)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        idx, d2 = device_knn_equals(c, sc, xyz, ind, k, brute_knn)
    assert (np.diff(d2, axis=1) == 0).any(1).all()


# ---------------------------------------------------------------- 3. rings
RINGS = [("far_clusters", 5, 5), ("far_clusters", 100, 100), ("far_clusters", 127, 127), ("line", 5000, 3), ("line", 5000, 100)]


@pytest.mark.parametrize("name,arg,k", RINGS)
def test_rings(ctx, sc, name, arg, k):
    xyz, rgb, ind = built(name, arg)[:3]
    with cloud.Cloud(xyz, ctx=ctx) as c:
        device_knn_equals(c, sc, xyz, ind, k)
        device_knn_equals(c, sc, xyz, ind[::3], k)
    holed, rows = with_holes(xyz, ind)                                              # a few indexed rows made non-finite
    with cloud.Cloud(holed, ctx=ctx) as c:
        for sub in (ind, ind[::3]):
            idx, d2 = device_knn_equals(c, sc, holed, sub, k)
            gone = np.isin(sub, rows)
            assert gone.any() and (idx[gone] == -1).all() and np.isinf(d2[gone]).all() and not np.isin(idx, rows).any()
            assert (idx[~gone, 0] == sub[~gone]).all()


@pytest.mark.parametrize("k", [5, 100, 127])
def test_far_clusters_whole_call(ctx, sc, k):
    xyz, rgb, ind, kw, _ = built("far_clusters", k)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        device_equals(c, sc, xyz, rgb, ind, kw)


# ---------------------------------------------------------------- 4. chains
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("nn", [2, 3])
def test_chains(ctx, sc, order, nn):
    m = 4097
    xyz, rgb, ind, kw = built("snake", m, order)
    kw = dict(kw, neighbour_number=nn)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        got = device_equals(c, sc, xyz, rgb, ind, kw)
        assert got["ns"] == 1 and (got["seg"] == 0).all() and got["nc"] == 1 and (got["labels"] == 0).all()
        if order == "descending":                                                   # the atomics race: only the rounds may differ
            for _ in range(5):
                again = device_whole(c, rgb, ind, kw)
                assert same(again, got)
                assert again["seg"].tobytes() == got["seg"].tobytes() and again["labels"].tobytes() == got["labels"].tobytes()


# ---------------------------------------------------------------- 5. the rule scenes built by hand
@pytest.mark.parametrize("name,scene,want", scenes.rule_scenes(), ids=[r[0] for r in scenes.rule_scenes()])
def test_rule_scenes(ctx, sc, name, scene, want):
    xyz, rgb, ind, kw = scene
    o = ref_opts(**kw)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        device_knn_equals(c, sc, xyz, ind, o["region_neighbour_number"], brute_knn)
        got = device_whole(c, rgb, ind, kw)
    check_expectation(want, (got["seg"], got["ns"]), (got["labels"], got["nc"], got["stats"][2]))
    sseg, sns = stub_grow(sc, xyz, rgb, ind, o)
    slabels, snc, sstats, _ = stub_segment(sc, xyz, rgb, ind, o)
    assert same(got, dict(seg=sseg, ns=sns, labels=slabels, nc=snc, stats=list(sstats[:3])))


# ---------------------------------------------------------------- 6. the segment tables' edges
def table_scenes():
    out = [("blobs_%d" % S, ("blobs", S), {}, False) for S in scenes.BLOB_SIZES]
    out += [("hub_12_%d" % keep, ("hub", 12, keep), {}, True) for keep in (1, 4, 5)]
    out += [("thirds", ("thirds",), {}, False)]
    out += [("own_segment_%d" % m, ("untied_sheet", m, m), dict(neighbour_number=1), False) for m in (257, 1025)]
    out += [("clamped_neighbour_number", ("untied_sheet", 300), dict(neighbour_number=200, region_neighbour_number=100), False),
            ("zero_point_threshold", ("untied_sheet", 300), dict(point_color_threshold=0.0), False)]
    return out


@pytest.mark.parametrize("name,build,extra,tied", table_scenes(), ids=[t[0] for t in table_scenes()])
def test_table_edges(ctx, sc, name, build, extra, tied):
    xyz, rgb, ind, kw = built(*build)[:4]
    kw = dict(kw, **extra)
    ref = reference_segmentation(xyz, rgb, ind, ref_opts(**kw), tied)
    with cloud.Cloud(xyz, ctx=ctx) as c:
        got = device_equals(c, sc, xyz, rgb, ind, kw, tied, ref)
        alpha = device_equals(c, sc, xyz, rgb | np.uint32(0xFF000000), ind, kw, tied, ref)    # the upper byte is no colour
    assert same(alpha, got)
    if name.startswith("blobs"):
        assert got["ns"] == got["nc"] == got["stats"][2] == build[1]
    if name.startswith("own_segment"):
        assert got["ns"] == len(ind) and np.array_equal(got["seg"], np.arange(len(ind)))
    if name == "hub_12_1":
        assert got["ns"] == len(ind)
    if name in ("hub_12_4", "hub_12_5"):
        assert got["ns"] == 13 and got["stats"][2] == 13 - build[2]                 # the hub and the satellites its capped list keeps


# ---------------------------------------------------------------- 7. lists with no finite point, with one, a cloud of one point
def test_empty_cases(ctx, sc):
    xyz, rgb, ind, kw = built("untied_sheet", 300)
    sub = ind[:40]
    none = xyz.copy()
    none[sub, 0] = np.nan
    o = ref_opts(**kw)
    with cloud.Cloud(none, ctx=ctx) as c:
        labels, nc, st = segment.segment_rgb(c, rgb, sub, segment.default_opts(**kw))        # (status 0: a refusal raises)
        assert (labels == -1).all() and nc == 0 and [st.n_idx, st.n_segments, st.n_regions] == [0, 0, 0] and st.rounds >= 1
        seg, ns, rounds = segment.grow(c, rgb, sub, segment.default_opts(**kw))
        assert (seg == -1).all() and ns == 0 and rounds >= 1
        idx, d2 = segment.subset_knn(c, sub, 5)
        assert (idx == -1).all() and np.isinf(d2).all()
        slabels, snc, sstats, _ = stub_segment(sc, none, rgb, sub, o)
        sseg, sns = stub_grow(sc, none, rgb, sub, o)
        assert np.array_equal(labels, slabels) and nc == snc and list(sstats[:3]) == [0, 0, 0] and np.array_equal(seg, sseg) and ns == sns
    one = none.copy()
    one[17] = xyz[17]
    kw1 = dict(min_cluster_size=1)
    with cloud.Cloud(one, ctx=ctx) as c:
        device_knn_equals(c, sc, one, sub, 3)
        got = device_whole(c, rgb, sub, kw1)
        sseg, sns = stub_grow(sc, one, rgb, sub, ref_opts(**kw1))
        slabels, snc, sstats, _ = stub_segment(sc, one, rgb, sub, ref_opts(**kw1))
        assert same(got, dict(seg=sseg, ns=sns, labels=slabels, nc=snc, stats=list(sstats[:3])))
        assert got["ns"] == got["nc"] == 1 and list(np.nonzero(got["labels"] == 0)[0]) == [17] and got["stats"] == [1, 1, 1]
    with cloud.Cloud(xyz[:1], ctx=ctx) as c:
        device_equals(c, sc, xyz[:1], rgb[:1], ind[:1], kw1)
        got = device_whole(c, rgb[:1], ind[:1], kw1)
        assert got["ns"] == got["nc"] == 1 and list(got["labels"]) == [0] and got["stats"] == [1, 1, 1]
