"""GPU: the dense multi-view stereo (sfmhip_mvs_*, csrc/mvs.hip) against the g++ build of the same header
(tests/stub/mvs_capi.cpp), compared as bytes: pyramid, index map, depth, score, point count, xyz, normals, rgb; then the
fusion cases and the analytic assertions of tests/test_mvs_cpu.py on the device's output.

The second half runs the cases S1 - S14 of tests/test_mvs_reference_cpu.py (its docstring has the table and the measured
figures; the preconditions that keep a case from going vacuous are asserted there, on the CPU): rotated views (a vertical
weight on 97 % of S1's samples, c <= 0 and all four borders in S4, a source that looks away), exact ties, the u32 ceiling of the LDS sums, a tile
that leaves early beside one that does not, images smaller than a tile or a window, 256 planes with 8 sources, pyramid
levels 2 and 3, a short source choice, per-view ranges, one handle at 9, 256 and 9 planes, and the fusion under rotation,
at half-pixel projections and on non-finite depths.  Each is compared as bytes with the stub and with the numpy reference
of tests/mvs_reference.py, which shares no code with either (a NaN must meet a NaN: the host's and the device's differ in
sign).  No test provokes a fault: every input is one the ABI accepts."""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from sfm_danpipeline_amd import build, mvs
from tests import mvs_reference as R
from tests.test_gpu_incr_views import _read_out
from tests.test_host_io import TEMPLE, _png_bytes
from tests.test_mvs_cpu import (D, DMAX, DMIN, K0, SLANT_BOUND, SPHERE_BOUND, StubMvs, build_stub, check_edge, check_fronto,
                                check_fusion, check_refusals, check_surface, hit_depth, opts, plane_inv, scene, timing_scene)
from tests.test_mvs_reference_cpu import (check_s3, check_s11_pyramid, check_s11_tiny, check_s12_reuse, check_s13,
                                          check_s14_half_pixel, check_s14_odd_depths)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("mvs") / "libmvscapi.so"))


@pytest.fixture(scope="module")
def scenes():
    """rendered once, shared, never written to"""
    out = {(k, l): scene(k, l) for k, l in (("fronto", 0), ("slanted", 0), ("sphere", 0), ("edge", 0), ("sphere", 1))}
    for v in out.values():
        v[0].setflags(write=False)
    return out


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _both(ms, o):
    """the same options for the device and for the stub"""
    kw = {f: getattr(o, f) for f, _ in o._fields_ if f != "pad"}
    return mvs.default_opts(**kw), opts(ms, **kw)


def _compare(ctx, ms, gray, K, P, level, kw, src=(1, 3, 0, 4), bgr=None, ref=2, dmin=DMIN, dmax=DMAX, maps=False):
    """device against stub, bytes; dmin / dmax: one range or one per view; maps: return the whole (index, depth, score)"""
    od, oh = _both(ms, opts(ms, **kw))
    zlo, zhi = (float(np.broadcast_to(a, (len(gray),))[ref]) for a in (dmin, dmax))     # the reference view's range
    with mvs.Mvs(gray, K, P, bgr=bgr, level=level, ctx=ctx) as G, StubMvs(ms, gray, K, P, bgr, level) as H:
        assert (G.rows, G.cols) == (H.rows, H.cols) and _same(G.K, H.K)
        for v in range(len(gray)):
            assert all(a is None and b is None or _same(a, b) for a, b in zip(G.level_image(v), H.level_image(v)))
        src = list(src)[:od.n_src]
        gi, gd, gs = G.depthmap(ref, src, zlo, zhi, od)
        hi, hd, hs = H.depthmap(ref, src, zlo, zhi, oh)
        print(f"{G.cols} x {G.rows}, {kw}: {int((gi >= 0).sum())} pixels with depth; index / depth / score differ at "
              f"{int((gi != hi).sum())} / {int((gd != hd).sum())} / {int((gs != hs).sum())}")
        assert _same(gi, hi) and _same(gd, hd) and _same(gs, hs)
        gi2, gd2, gs2 = G.depthmap(ref, src, zlo, zhi, od)                     # a repeat on the handle: the same bytes
        assert _same(gi, gi2) and _same(gd, gd2) and _same(gs, gs2)
        g, h = G.run(dmin, dmax, od), H.run(dmin, dmax, oh)
        print(f"    run: {len(g[0])} points on the device, {len(h[0])} with the host build")
        assert all(_same(a, b) for a, b in zip(g, h))
        assert all(_same(a, b) for a, b in zip(g, G.run(dmin, dmax, od)))
        return ((gi, gd, gs) if maps else gi), g


CASES = [  # every path of the sweep kernel: edge tiles in both directions, D, n_src, window, n_best, level
    ("sphere", 0, (64, 96), dict(n_planes=33)),
    ("sphere", 0, (45, 70), dict(n_planes=33)),
    ("sphere", 0, (45, 70), dict(n_planes=3, n_src=2, window=1)),
    ("slanted", 0, (45, 70), dict(n_planes=128, n_src=1, n_best=1)),
    ("edge", 0, (64, 96), dict(n_planes=128, window=1, n_src=4, n_best=3, min_views=2)),
    ("sphere", 1, (90, 141), dict(n_planes=33, n_src=2)),
    ("sphere", 1, (128, 192), dict(n_planes=33, window=7, n_best=4)),
    ("fronto", 0, (64, 96), dict(n_planes=33, var_min=0.0, ncc_min=-1.0, eps=0.05)),
]


@pytest.mark.parametrize("kind,level,size,kw", CASES)
def test_device_equals_the_header_build(ctx, ms, scenes, kind, level, size, kw):
    gray, depth, K, P = scenes[(kind, level)]
    gray = gray[:, :size[0], :size[1]]
    bgr = np.stack([gray, 255 - gray, gray // 3], -1) if level else None
    gi, pts = _compare(ctx, ms, gray, K, P, level, kw, bgr=bgr)
    assert (gi >= 0).sum() > 100 and len(pts[0]) > 100


def test_a_view_outside_its_sources_frustum(ctx, ms, scenes):
    gray, depth, K, P = scenes[("sphere", 0)]
    P = P.copy()
    P[4, 0, 3] = -50.0                                                           # view 4 looks at nothing the others see
    gi, pts = _compare(ctx, ms, gray, K, P, 0, dict(n_planes=33), src=(3, 2, 1, 0), ref=4)
    assert (gi == -1).all() and len(pts[0]) > 100


def test_fusion_on_hand_made_maps(ctx):
    check_fusion(lambda g, K, P, b, level: mvs.Mvs(g, K, P, bgr=b, level=level, ctx=ctx), mvs.default_opts)


def test_analytic_scenes_on_the_device(ctx, scenes):
    for kind, check in (("fronto", lambda M, o, z: check_fronto(M, o)),
                        ("slanted", lambda M, o, z: check_surface(M, o, z, "slanted plane", SLANT_BOUND)),
                        ("sphere", lambda M, o, z: check_surface(M, o, z, "sphere", SPHERE_BOUND)),
                        ("edge", lambda M, o, z: check_edge(M, mvs.default_opts(n_planes=D, min_views=5)))):
        gray, depth, K, P = scenes[(kind, 0)]
        with mvs.Mvs(gray, K, P, level=0, ctx=ctx) as M:
            check(M, mvs.default_opts(n_planes=D), depth)


def test_refusals(ctx, scenes):
    gray, depth, K, P = scenes[("fronto", 0)]
    for bad in (lambda: mvs.Mvs(gray[:1], K, P[:1], level=0, ctx=ctx), lambda: mvs.Mvs(gray[:, :1, :1], K, P, level=1, ctx=ctx),
                lambda: mvs.Mvs(gray[:, :0], K, P, level=0, ctx=ctx)):
        with pytest.raises(Exception, match="status -3"):
            bad()
    with mvs.Mvs(gray, K, P, level=0, ctx=ctx) as M:
        check_refusals(M, mvs.default_opts)


def test_run_is_faster_than_the_host_build_on_16_threads(ctx, ms):
    """the size the pipeline runs at: 10 views of 640 x 480 at level 1, 128 planes, 4 sources"""
    gray, K, P = timing_scene()
    od, oh = _both(ms, opts(ms))
    with mvs.Mvs(gray, K, P, level=1, ctx=ctx) as G, StubMvs(ms, gray, K, P, None, 1) as H:
        g = G.run(1.2, 4.0, od)
        t0 = time.perf_counter()
        g2 = G.run(1.2, 4.0, od)
        gpu_s = time.perf_counter() - t0                                          # (the timed call is the warm one)
        t0 = time.perf_counter()
        h = H.run(1.2, 4.0, oh)
        cpu_s = time.perf_counter() - t0
        print(f"10 x 640 x 480 at level 1: {len(g[0])} points; device {gpu_s:.3f} s {G.last_timing()}, host build {cpu_s:.3f} s")
        assert len(g[0]) > 10000 and all(_same(a, b) for a, b in zip(g, h)) and all(_same(a, b) for a, b in zip(g, g2))
        assert gpu_s < cpu_s, "the device call is slower than the header's host build on 16 threads"


# ---------------------------------------------------------------- the cases of tests/test_mvs_reference_cpu.py
def _device(ctx):
    return lambda g, K, P, b, level: mvs.Mvs(g, K, P, bgr=b, level=level, ctx=ctx)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_equals_the_header_build_and_the_reference(ctx, ms, name):
    c, r = R.case(name), R.reference(name)
    (gi, gd, gs), pts = _compare(ctx, ms, c.gray, c.K, c.poses, c.level, c.kw, src=c.src, bgr=c.bgr, ref=c.ref, dmin=c.dmin,
                                 dmax=c.dmax, maps=True)
    assert _same(gi, r.idx) and _same(gd, r.depth) and _same(gs, r.score)
    if r.points is not None:
        assert all(_same(a, b) for a, b in zip(pts, r.points))


def test_s3_rendered_scene_under_rotation(ctx):
    check_s3(_device(ctx), mvs.default_opts)


def test_s11_pyramid_levels_two_and_three(ctx):
    check_s11_pyramid(_device(ctx))


def test_s11_images_of_one_and_two_pixels(ctx):
    check_s11_tiny(_device(ctx), mvs.default_opts)


def test_s12_one_handle_at_9_256_and_9_planes(ctx):
    check_s12_reuse(_device(ctx), mvs.default_opts)


def test_s13_fusion_under_rotation(ctx):
    check_s13(_device(ctx), mvs.default_opts)


def test_s14_fusion_where_the_rounding_decides(ctx):
    check_s14_half_pixel(_device(ctx), mvs.default_opts)


def test_s14_fusion_of_odd_depths(ctx):
    check_s14_odd_depths(_device(ctx), mvs.default_opts)


# ---------------------------------------------------------------- the host mirror: densify and its driver
XML = """<?xml version="1.0"?>
<opencv_storage>
<Camera_Matrix type_id="opencv-matrix"><rows>3</rows><cols>3</cols><dt>d</dt><data>
 {} {} {} {} {} {} {} {} {}</data></Camera_Matrix>
<Distortion_Coefficients type_id="opencv-matrix"><rows>1</rows><cols>5</cols><dt>d</dt><data>
 0. 0. 0. 0. 0.</data></Distortion_Coefficients>
</opencv_storage>
"""


def write_state(path, P, registered, xyz, views, K=None):
    """the driver's poses + cloud file: views[i] lists the views that observe point i"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(P)))
        f.write(np.asarray(K if K is not None else np.zeros(9), "<f8").tobytes())
        for v in range(len(P)):
            f.write(struct.pack("<i", int(v in registered)) + np.asarray(P[v], "<f8").tobytes())
        f.write(struct.pack("<i", len(xyz)))
        for X, vs in zip(xyz, views):
            f.write(np.asarray(X, "<f8").tobytes() + struct.pack(f"<i{len(vs)}i", len(vs), *vs))


def read_dense_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    assert head[1] == "format binary_little_endian 1.0"
    assert [h.split()[-1] for h in head if h.startswith("property")] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    n = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    rec = np.frombuffer(raw, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]), n, end)
    assert len(raw) == end + 27 * n
    return rec["p"].copy(), rec["n"].copy(), rec["c"].copy()


def depth_ranges(P, xyz, views, n):
    """densify's rule: per view the smallest and largest depth of the sparse points it observes, widened by 25 %"""
    lo, hi = np.zeros(n), np.zeros(n)
    for v in range(n):
        z = np.array([(P[v, 2, 0] * X[0] + P[v, 2, 1] * X[1]) + (P[v, 2, 2] * X[2] + P[v, 2, 3]) for X, vs in zip(xyz, views) if v in vs])
        lo[v], hi[v] = z.min() / 1.25, z.max() * 1.25
    return lo, hi


def test_cpp_driver_densify_then_ply_to_pcd(ctx, scenes, tmp_path):
    """sfm_dense_selftest on the sphere scene written as PNGs (level 1 of 192 x 128), then convertPLYtoPCD (through
    sfm_cloud_selftest, the next driver of the chain): the point counts agree with sfmhip_mvs_run's"""
    exe, cloud_exe = build.build_dense_demo(), build.build_cloud_demo()
    gray, depth, K, P = scenes[("sphere", 1)]
    img = tmp_path / "img"
    img.mkdir()
    for v, g in enumerate(gray):
        (img / f"v{v:02d}.png").write_bytes(_png_bytes(g, 0))
    (tmp_path / "calib.xml").write_text(XML.format(*K.ravel()))
    # sparse points: a grid of the middle view's pixels on the sphere's face, lifted with the analytic depth, seen by all
    ys, xs = np.meshgrid(np.arange(40, 90, 10), np.arange(60, 135, 10), indexing="ij")
    dx, dy = (xs.ravel() - K[0, 2]) / K[0, 0], (ys.ravel() - K[1, 2]) / K[1, 1]
    z = hit_depth([("sphere", (0, 0, 1 / plane_inv(16) + 0.9), 1.0)], -P[2, :, 3], dx, dy)
    keep = np.isfinite(z)
    xyz = np.stack([-P[2, 0, 3] + z * dx, z * dy, z], 1)[keep]
    views = [list(range(5))] * len(xyz)
    assert len(xyz) >= 8
    write_state(tmp_path / "state.bin", P, set(range(5)), xyz, views)
    r = subprocess.run([exe, str(img), str(tmp_path / "calib.xml"), str(tmp_path / "state.bin"), str(tmp_path / "dense")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    p, nrm, c = read_dense_ply(tmp_path / "dense" / "models" / "options.txt.ply")
    lo, hi = depth_ranges(P, xyz, views, 5)
    with mvs.Mvs(gray, K, P, bgr=np.stack([gray] * 3, -1), level=1, ctx=ctx) as M:
        gx, gn, gc = M.run(lo, hi, mvs.default_opts(min_views=5))
    print(f"densify: {len(p)} points in the PLY, {len(gx)} from sfmhip_mvs_run")
    assert len(p) == len(gx) > 100 and _same(p, gx) and _same(nrm, gn)
    assert np.array_equal(c.astype(np.uint32) @ np.array([65536, 256, 1], np.uint32), gc)
    r = subprocess.run([cloud_exe, str(tmp_path / "dense" / "models" / "options.txt.ply"), str(tmp_path), str(tmp_path / "cloud.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"points {len(p)} " in r.stdout


def test_temple_frames(tmp_path):
    """the ten temple frames after the incremental driver's poses: structure only (DESIGN f-10 records the count)"""
    incr, exe = build.build_incr_demo(), build.build_dense_demo()
    xml = os.path.join(TEMPLE, "camera_calibration_template.xml")
    r = subprocess.run([incr, "--images", TEMPLE, xml, str(tmp_path / "incr.out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    o = _read_out(str(tmp_path / "incr.out"))
    views = [[v for v, _ in t] for t in o["tracks"]]
    write_state(tmp_path / "state.bin", o["P"], o["good"], o["xyz"], views, K=o["K"].ravel())
    r = subprocess.run([exe, TEMPLE, xml, str(tmp_path / "state.bin"), str(tmp_path / "dense")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    p, nrm, c = read_dense_ply(tmp_path / "dense" / "models" / "options.txt.ply")
    print(f"MEASURE temple dense cloud: {len(p)} points from {len(o['good'])} registered views, sparse cloud {len(o['xyz'])}")
    assert len(p) > 0 and np.isfinite(p).all() and np.isfinite(nrm).all()
    seen = np.zeros(len(p), int)
    for v in o["good"]:
        q = p.astype(np.float64) @ o["P"][v][:, :3].T + o["P"][v][:, 3]
        u = q[:, :2] / q[:, 2:] * [o["K"][0, 0], o["K"][1, 1]] + [o["K"][0, 2], o["K"][1, 2]]
        seen += (q[:, 2] > 0) & (u[:, 0] >= -0.5) & (u[:, 0] <= 639.5) & (u[:, 1] >= -0.5) & (u[:, 1] <= 479.5)
    assert (seen >= 5).all()
    lo, hi = o["xyz"].min(0), o["xyz"].max(0)
    ext = 0.25 * (hi - lo)
    assert ((p >= lo - ext) & (p <= hi + ext)).all()
