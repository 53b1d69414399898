"""GPU: dendrometry (csrc/dendro.hip) against the g++ build of the same header (tests/stub/dendro_capi.cpp),
bit for bit: the whole slice table, every scalar and the flags, on planted trees of 3 k, 60 k and 200 k points in every
scene variant (the three sizes x the seven scenes), the rule cases, the handle reused after the colour segmentation and with two labels, a warm call against
the stub on 16 threads, and the host mirror's self-test."""
import os
import re
import struct
import subprocess
import time

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, dendro, segment
from sfm_danpipeline_amd.cloud import Cloud
from tests.test_dendro_cpu import (DBH_NONE, EMPTY, NO_CROWN, RULE_SLICES, dn, planted, pole, result_bytes, scenes, stub_opts,  # noqa: F401
                                   stub_run)
from tests.test_gpu_segment import _write_pcd, scene

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(build.__file__))


def dev_run(xyz, labels=None, label=0, opts=None, cloud=None, both=False):
    """(result, rows) of one sfmhip_cloud_dendro_profile call; with `both`, sfmhip_cloud_dendrometry must give the same scalars."""
    if cloud is None:
        with Cloud(xyz) as c:
            return dev_run(xyz, labels, label, opts, c, both)
    res, rows = dendro.measure_profile(cloud, labels, label, opts)
    if both:
        assert result_bytes(dendro.measure(cloud, labels, label, opts)) == result_bytes(res)
    return res, rows


def assert_equal(dn, xyz, labels=None, label=0, opts=None, cloud=None, both=False):
    res, rows, _ = stub_run(dn, xyz, labels, label, opts)
    dres, drows = dev_run(xyz, labels, label, opts, cloud, both)
    assert drows.tobytes() == rows.tobytes()
    assert result_bytes(dres) == result_bytes(res)
    return dres, drows


@pytest.mark.parametrize("n", [3000, 60000, 200000])
@pytest.mark.parametrize("name", ["ring", "arc200", "arc200_clutter", "taper", "rotated", "scaled", "labels"])
def test_device_equals_the_stub(ctx, dn, name, n):
    xyz, lab, label, o, _, _ = scenes(lambda **kw: stub_opts(dn, **kw), n)[name]
    res, rows = assert_equal(dn, xyz, lab, label, o, both=n == 3000)
    assert res.n_slices == 91
    if n >= 60000:                      # 500 trunk points a slice and more; at 3 000 a slice holds about 25, around min_inliers = 20
        assert rows["stem"][:30].all()
    if n == 200000:                     # slices beyond one LDS chunk of dnd_ransac (1 024 pairs) and one pass of dnd_refit's threads
        assert rows["count"].max() > 2048 and rows["count"][:30].min() > 1024


def test_device_equals_the_stub_at_200k_and_is_faster_warm(ctx, dn):
    xyz, _ = planted(21, 200000)
    with Cloud(xyz) as c:
        assert_equal(dn, xyz, cloud=c, both=True)
        t0 = time.perf_counter()
        dendro.measure(c)
        dev = time.perf_counter() - t0
        stages = dendro.last_timing(c)
    t0 = time.perf_counter()
    stub_run(dn, xyz, threads=16)
    cpu = time.perf_counter() - t0
    print(f"200 k points: device {dev * 1e3:.2f} ms, stub on 16 threads {cpu * 1e3:.2f} ms, stages {stages}")
    assert dev < cpu


@pytest.mark.parametrize("iters", [1, 65, 4096])
def test_iteration_counts(ctx, dn, iters):
    xyz, _ = planted(22, 3000)
    assert_equal(dn, xyz, opts=stub_opts(dn, ransac_iters=iters))


def test_rule_cases_on_the_device(ctx, dn):
    # the hand-made slices, one per 0.1 of height in one cloud (the empty ones leave their slice empty)
    parts = [np.concatenate([en, np.full((len(en), 1), 0.05 + 0.1 * k, np.float32)], 1) for k, en in enumerate(RULE_SLICES.values())]
    xyz = np.concatenate(parts).astype(np.float32)
    res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, ground=0.0))
    assert rows["count"].tolist()[:len(parts)] == [len(p) for p in parts]
    assert_equal(dn, xyz, opts=stub_opts(dn, ground=0.0, min_sectors=4))
    # flag bits 1, 2, 3, 0; NaN points; one slice that holds every point
    g = stub_opts(dn, ground=0.0)
    assert assert_equal(dn, pole(), opts=g)[0].flags == NO_CROWN
    assert assert_equal(dn, pole(drop=(12,)), opts=g)[0].flags == NO_CROWN | 2
    assert assert_equal(dn, pole(drop=(12, 13)), opts=g)[0].flags == NO_CROWN | DBH_NONE
    assert assert_equal(dn, pole(), np.zeros(len(pole()), np.int32), 3)[0].flags == EMPTY
    assert assert_equal(dn, np.full((5, 3), np.nan, np.float32))[0].flags == EMPTY
    assert assert_equal(dn, pole(), opts=stub_opts(dn, ground=10.0))[0].flags == EMPTY
    xyz, _ = planted(23, 3000)
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 2], [3e38, 3e38, 3e38]], np.float32)
    assert_equal(dn, np.concatenate([bad, xyz]), opts=stub_opts(dn, up=(0.6, 0.0, 0.8)))
    res, rows = assert_equal(dn, xyz, opts=stub_opts(dn, slice=20.0))
    assert res.n_slices == 1 and rows[0]["count"] == 3000
    with pytest.raises(_lib.SfmHipError), Cloud(xyz) as c:
        dendro.measure(c, opts=dendro.default_opts(up=(0, 0, 2)))
    with pytest.raises(_lib.SfmHipError), Cloud(xyz) as c:
        dendro.measure(c, opts=dendro.default_opts(north=(0, 0, 1)))
    with pytest.raises(_lib.SfmHipError), Cloud(xyz) as c:
        dendro.measure(c, opts=dendro.default_opts(ransac_iters=4097))
    assert result_bytes(dendro.default_opts()) == result_bytes(stub_opts(dn))


def test_handle_reuse_after_the_segmentation_and_with_two_labels(ctx, dn):
    xyz, rgb = scene(8000, 3)
    o = stub_opts(dn, up=(1, 0, 0), slice=0.02, scale=0.2, min_slice_pts=5)         # (the patches lie flat: 40 slices along x)
    with Cloud(xyz) as c:
        labels, nc, _ = segment.segment_rgb(c, rgb, c.passthrough(2, 0.0, 14.0), segment.default_opts(min_cluster_size=100))
        assert nc >= 2
        for label in (0, 1, 0, -1):
            assert_equal(dn, xyz, labels, label, o, cloud=c)
        labels2, nc2, _ = segment.segment_rgb(c, rgb, c.passthrough(2, 0.0, 14.0), segment.default_opts(min_cluster_size=100))
        assert nc2 == nc and np.array_equal(labels, labels2)


STARS = "************************************************"


def _g(v):
    """A float or double as std::ostream prints it by default (%g, six significant digits)."""
    return "%g" % float(v)


def _result_and_rows(blob, res):
    nres = len(result_bytes(res))
    m = struct.unpack_from("<i", blob, nres)[0]
    return blob[:nres], m, blob[nres + 4:]


def test_host_mirror_selftest(ctx, dn, tmp_path):
    exe = build.build_dendro_demo()
    xyz, _ = planted(24, 20000)
    rgb = np.full(len(xyz), 0x00406020, np.uint32)
    pcd, out = str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, rgb)
    r = subprocess.run([exe, pcd, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res, rows = dev_run(xyz)
    head, m, tail = _result_and_rows(open(out, "rb").read(), res)
    assert head == result_bytes(res) and m == len(rows) and tail == rows.tobytes()
    lines = {ln.split("=")[0]: ln.split("=")[1] for ln in r.stdout.splitlines() if "=" in ln}
    for key in ("Total Height ", "Altura copa viva", "Altura base de copa", "DAP", "Amplitud N-S", "Amplitud E-W"):
        assert re.fullmatch(r"-?\d+(\.\d+)?(e-?\d+)?", lines[key]), (key, lines[key])
    assert abs(float(lines["DAP"]) - 0.3) < 0.002 and lines["Altura DAP"] == "1.3"
    assert r.stdout == "\n".join([STARS, "              DENDROMETRY ESTIMATION            ", STARS, "*** Measurements ***",
                                  "Total Height =" + _g(res.total_height), "Altura copa viva=" + _g(res.live_crown),
                                  "Altura base de copa=" + _g(res.crown_base_height), "Altura DAP=1.3", "DAP=" + _g(res.dbh),
                                  "Amplitud N-S=" + _g(res.spread_ns), "Amplitud E-W=" + _g(res.spread_ew), STARS, STARS, ""])


def _segment_stdout(n, nc):
    return [STARS, "    COLOR BASE GROWING SEGMENTATION             ", STARS, "Preparing options for segmentation...",
            "Input cloud:%d" % n, "Distance threshold:10", "Point color threshold:6", "Region color threshold:5", "Clusters size:600",
            "Extracting clusters...", "Extract:%d clusters" % nc, STARS, STARS]


def test_host_mirror_selftest_on_one_cluster(ctx, dn, tmp_path):
    """The [label] form: the colour segmentation, then estimateTree on that cluster."""
    exe = build.build_dendro_demo()
    xyz, rgb = scene(8000, 6)
    xyz[np.isnan(xyz[:, 0]), 0] = 0.5                                                        # (a binary PCD of finite points)
    pcd, out = str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, rgb)
    labels, nc, _ = segment.color_based_growing_segmentation(xyz, rgb, ctx=ctx)
    assert nc >= 2
    for label in (1, 0):
        r = subprocess.run([exe, pcd, out, str(label)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        res, rows = dev_run(xyz, labels, label)
        assert res.n_selected == int((labels == label).sum()) > 0
        head, m, tail = _result_and_rows(open(out, "rb").read(), res)
        assert head == result_bytes(res) and m == len(rows) and tail == rows.tobytes()
        assert r.stdout.startswith("\n".join(_segment_stdout(len(xyz), nc)) + "\n" + STARS + "\n              DENDROMETRY ESTIMATION")
        assert ("\nTotal Height =" + _g(res.total_height) + "\n") in r.stdout


def test_segment_selftest_prints_what_it_printed(ctx, tmp_path):
    """Dendrometry::estimate is untouched: sfm_segment_selftest's whole output, byte for byte -- the segmentation's block, then the
    reference's dendrometry block with its bounds, the bounding-box "Total Height" and the blanks left blank."""
    exe = build.build_segment_demo()
    xyz, rgb = scene(8000, 6)
    xyz[np.isnan(xyz[:, 0]), 0] = 0.5
    pcd, out = str(tmp_path / "MAP3D.pcd"), str(tmp_path / "out.bin")
    _write_pcd(tmp_path / "MAP3D.pcd", xyz, rgb)
    r = subprocess.run([exe, pcd, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    labels, nc, _ = segment.color_based_growing_segmentation(xyz, rgb, ctx=ctx)
    with Cloud(xyz, ctx=ctx) as c:
        mn, mx, h = segment.minmax(c)
    want = _segment_stdout(len(xyz), nc) + [
        STARS, "              DENDROMETRY ESTIMATION            ", STARS,
        "Max: [%s, %s, %s]" % tuple(_g(v) for v in mx), "Min: [%s, %s, %s]" % tuple(_g(v) for v in mn),
        "*** Measurements ***", "Total Height =" + _g(h), "Altura copa viva=", "Altura base de copa=", "Altura DAP=1.3", "DAP=",
        "Amplitud N-S=", "Amplitud E-W=", STARS, STARS, ""]
    assert r.stdout == "\n".join(want)
