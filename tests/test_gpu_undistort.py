"""GPU: the lens-distortion resampling in front of the dense stereo (sfmhip_image_undistort, sfmhip_mvs_create_distorted,
sfmhip_mvs_valid; csrc/undistort.hip) against the g++ build of the same header
(tests/stub/undistort_capi.cpp), compared as bytes: pictures, masks, and the stereo's index, depth and score maps under
"no depth at the seam"; then the analytic assertions of tests/test_undistort_cpu.py on the device's output, and the C++
driver on pictures of a distorted camera.  No test provokes a fault.

The driver's cloud (five 64 x 96 renders of the slanted plane, so 32 x 48 at the driver's level 1, all five views agreeing):
relative depth offset from the plane along the owner's ray, measured on an MI355X: with the calibration's coefficients 461
points, median 0.0031, 95th percentile 0.0091, largest 0.0131; with the coefficients zeroed 35 points, median 0.0189.  The fusion's eps (0.01) bounds the disagreement BETWEEN views, so a kept point can sit a little beyond eps of the truth
when every view errs the same way: the test holds the project's two statistics, median and 95th percentile, to eps and
prints the largest."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, build, mvs, undistort
from tests.test_gpu_mvs import depth_ranges, read_dense_ply, write_state
from tests.test_host_io import _png_bytes
from tests.test_mvs_cpu import COLS, D, DMAX, DMIN, ROWS, SLANT_BOUND, SPHERE_BOUND, StubMvs, opts, plane_inv, scene
from tests.test_mvs_cpu import build_stub as build_mvs_stub
from tests.test_undistort_cpu import (K_ODD, SET_A, SET_B, build_stub, check_undistorted_surface, distorted_scene, rule_level_mask,
                                      stub_level_mask, stub_run, stub_seam, stub_undistort)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def us(tmp_path_factory):
    return build_stub(str(tmp_path_factory.mktemp("und") / "libundcapi.so"))


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_mvs_stub(str(tmp_path_factory.mktemp("mvs") / "libmvscapi.so"))


@pytest.fixture(scope="module")
def slanted():
    """the slanted plane through set A's lens at levels 0 and 1: rendered once, shared, never written to"""
    out = {level: distorted_scene("slanted", SET_A, level) for level in (0, 1)}
    for v in out.values():
        v[0].setflags(write=False)
    return out


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("rows,cols,ch,n", [(9, 11, 1, 1), (37, 53, 3, 3), (64, 96, 1, 5), (48, 64, 3, 2)])
def test_device_equals_the_header_build(ctx, us, rows, cols, ch, n):
    """sizes below one wave, no multiple of the gather's four pixels or of a block (37 x 53 = 1961), and multiples of four
    (the word stores): pictures and mask, both coefficient sets"""
    rng = np.random.RandomState(rows * ch)
    img = rng.randint(0, 256, (n, rows, cols) + ((3,) if ch == 3 else ())).astype(np.uint8)
    K = np.array([[0.9 * cols, 0, cols / 2 - 0.3], [0, 0.95 * cols, rows / 2 - 0.8], [0, 0, 1]])
    for dist in (SET_A, SET_B):
        got, gv = undistort.undistort(img, K, dist, ctx=ctx)
        want, wv = stub_undistort(us, img, K, dist)
        print(f"{n} x {rows} x {cols} x {ch} {dist}: {int(gv.sum())} valid; pictures differ at {int((got != want).sum())} bytes, "
              f"masks at {int((gv != wv).sum())}")
        assert _same(gv, wv) and _same(got, want)
        assert _same(got, undistort.undistort(img, K, dist, ctx=ctx)[0])           # a repeat: the same bytes


def test_zero_coefficients_copy_the_picture(ctx):
    rng = np.random.RandomState(5)
    for shape in ((48, 64), (48, 64, 3), (37, 53)):
        img = rng.randint(0, 256, (2,) + shape).astype(np.uint8)
        got, valid = undistort.undistort(img, K_ODD, np.zeros(5), ctx=ctx)
        assert _same(got, img) and (valid == 1).all()


def test_zero_coefficients_leave_the_stereo_as_it_was(ctx):
    for level in (0, 1):
        gray, depth, K, P = scene("fronto", level)
        bgr = np.stack([gray, 255 - gray, gray // 3], -1)
        o = mvs.default_opts(n_planes=D)
        with mvs.Mvs(gray, K, P, bgr=bgr, level=level, ctx=ctx) as A, mvs.Mvs(gray, K, P, bgr=bgr, level=level, ctx=ctx, dist=np.zeros(5)) as B:
            assert (A.rows, A.cols) == (B.rows, B.cols) == (ROWS, COLS) and _same(A.K, B.K)
            assert (A.valid() == 1).all() and (B.valid() == 1).all()
            for v in range(len(gray)):
                assert all(_same(a, b) for a, b in zip(A.level_image(v), B.level_image(v)))
            a, b = A.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, o), B.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, o)
            assert all(_same(x, y) for x, y in zip(a, b)) and (a[0] >= 0).sum() > 1000
            a, b = A.run(DMIN, DMAX, o), B.run(DMIN, DMAX, o)
            assert all(_same(x, y) for x, y in zip(a, b)) and len(a[0]) > 1000


@pytest.mark.parametrize("level,dist", [(0, SET_A), (1, SET_A), (1, SET_B)])
def test_distorted_handle_equals_the_header_builds(ctx, us, ms, slanted, level, dist):
    """Mvs(dist=...) against stub undistortion + halving + the stereo's host build + rule 7, bit for bit (set B on set A's
    pictures is as good a byte comparison as any, and has the invalid margin)"""
    gray, truth, K, P = slanted[level]
    bgr = np.stack([gray, 255 - gray, gray // 3], -1)
    und, valid0 = stub_undistort(us, gray, K, dist)
    und3, _ = stub_undistort(us, bgr, K, dist)
    valid = stub_level_mask(us, valid0, level)
    assert _same(valid, rule_level_mask(valid0, level)) and (dist is SET_A or (valid == 0).sum() > 100)
    kw = dict(n_planes=D)
    od, oh = mvs.default_opts(**kw), opts(ms, **kw)
    with mvs.Mvs(gray, K, P, bgr=bgr, level=level, ctx=ctx, dist=dist) as G, StubMvs(ms, und, K, P, und3, level) as H:
        assert (G.rows, G.cols) == (H.rows, H.cols) and _same(G.K, H.K)
        for v in range(len(gray)):
            assert all(_same(a, b) for a, b in zip(G.level_image(v), H.level_image(v)))
        assert _same(G.valid(), valid)
        g = G.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, od)
        raw = H.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, oh)
        h = stub_seam(us, valid, oh.window, *raw)
        print(f"level {level} {dist}: {int((g[0] >= 0).sum())} pixels with depth, {int((raw[0] >= 0).sum())} before rule 7; index / "
              f"depth / score differ at {[int((a != b).sum()) for a, b in zip(g, h)]}")
        assert all(_same(a, b) for a, b in zip(g, h)) and (g[0] >= 0).sum() > 1000
        pts, want = G.run(DMIN, DMAX, od), stub_run(us, ms, H, P, valid, DMIN, DMAX, oh)
        print(f"    run: {len(pts[0])} points on the device, {len(want[0])} with the host builds")
        assert all(_same(a, b) for a, b in zip(pts, want)) and len(pts[0]) > 100


class Device:
    """the device behind depthmap_of of check_undistorted_surface"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __call__(self, gray, K, P, dist):
        with mvs.Mvs(gray, K, P, level=0, ctx=self.ctx, dist=dist) as M:
            return M.depthmap(2, [1, 3, 0, 4], DMIN, DMAX, mvs.default_opts(n_planes=D))


@pytest.mark.parametrize("kind,bound", [("slanted", SLANT_BOUND), ("sphere", SPHERE_BOUND)])
@pytest.mark.parametrize("dist", [SET_A, SET_B])
def test_analytic_bounds_on_the_device(ctx, kind, bound, dist):
    check_undistorted_surface(kind, dist, bound, Device(ctx), mvs.default_opts(n_planes=D))


def test_refusals(ctx, slanted):
    gray, truth, K, P = slanted[0]
    L, img = _lib.lib(), np.ascontiguousarray(gray[0])
    out, valid = np.zeros_like(img), np.zeros(img.shape, np.uint8)
    sp, dp, null = (C.c_void_p * 1)(img.ctypes.data), (C.c_void_p * 1)(out.ctypes.data), (C.c_void_p * 1)(None)
    Kc, d = np.ascontiguousarray(K.reshape(9)), np.array(SET_A)
    Kf, dn = Kc.copy(), d.copy()
    Kf[4], dn[1] = 0.0, np.nan
    p = lambda a: a.ctypes.data
    und = lambda n=1, r=ROWS, c=COLS, ch=1, s=sp, k=p(Kc), dd=p(d), o=dp: L.sfmhip_image_undistort(ctx.h, n, r, c, ch, s, k, dd, o, p(valid))
    assert und() == 0
    for rc in (und(n=0), und(r=0), und(c=0), und(ch=2), und(ch=4), und(s=None), und(o=None), und(s=null), und(o=null), und(k=None),
               und(dd=None), und(k=p(Kf)), und(dd=p(dn)), L.sfmhip_image_undistort(None, 1, ROWS, COLS, 1, sp, p(Kc), p(d), dp, None)):
        assert rc == -3
    assert L.sfmhip_image_undistort(ctx.h, 1, ROWS, COLS, 1, sp, p(Kc), p(d), dp, None) == 0          # the mask is nullable
    gp = (C.c_void_p * 5)(*[g.ctypes.data for g in [np.ascontiguousarray(g) for g in gray]])
    Pc = np.ascontiguousarray(P.reshape(-1))
    for args in ((5, ROWS, COLS, gp, None, p(Kf), p(d), p(Pc), 0), (5, ROWS, COLS, gp, None, p(Kc), p(dn), p(Pc), 0),
                 (5, ROWS, COLS, gp, None, p(Kc), None, p(Pc), 0), (1, ROWS, COLS, gp, None, p(Kc), p(d), p(Pc), 0),
                 (5, 0, COLS, gp, None, p(Kc), p(d), p(Pc), 0), (5, 1, 1, gp, None, p(Kc), p(d), p(Pc), 1)):
        h = C.c_void_p(1)                                                            # (never dereferenced: set to null by the call)
        assert L.sfmhip_mvs_create_distorted(ctx.h, *args, C.byref(h)) == -3 and not h.value
    with pytest.raises(Exception, match="status -3"):
        mvs.Mvs(gray, K, P, level=0, ctx=ctx, dist=(np.inf, 0, 0, 0, 0))
    with pytest.raises(ValueError):
        mvs.Mvs(gray, K, P, level=0, ctx=ctx, dist=(0.1, 0, 0, 0))
    assert L.sfmhip_mvs_valid(None, p(valid)) == -3
    with mvs.Mvs(gray, K, P, level=0, ctx=ctx, dist=SET_A) as M:
        assert L.sfmhip_mvs_valid(M.h, None) == -3


XML = """<?xml version="1.0"?>
<opencv_storage>
<Camera_Matrix type_id="opencv-matrix"><rows>3</rows><cols>3</cols><dt>d</dt><data>
 {} {} {} {} {} {} {} {} {}</data></Camera_Matrix>
<Distortion_Coefficients type_id="opencv-matrix"><rows>1</rows><cols>5</cols><dt>d</dt><data>
 {} {} {} {} {}</data></Distortion_Coefficients>
</opencv_storage>
"""


def plane_offsets(p, nrm):
    """relative depth offset of the cloud's points from the slanted plane, each along the ray of the view that emitted it (the
    normal points at that view's centre; every view has the identity rotation, so a ray's z is its depth)"""
    n, d = np.array([-np.sin(np.pi / 6), 0, np.cos(np.pi / 6)]), np.cos(np.pi / 6) / plane_inv(16)
    X, N = p.astype(np.float64), nrm.astype(np.float64)
    C = X - (X[:, 2] / N[:, 2])[:, None] * N
    t = (d - C @ n) / ((X - C) @ n)                   # the plane lies at t times the point's depth
    return np.abs(1 / t - 1)


def test_cpp_driver_undistorts_by_the_calibration_file(ctx, slanted, tmp_path):
    """sfm_dense_selftest on five 64 x 96 pictures of the slanted plane through set A's lens: with the coefficients in the
    calibration file the cloud lies on the plane (median and 95th percentile within the fusion's eps; docstring of this file),
    with the coefficients zeroed the same pictures give a cloud that does not"""
    exe = build.build_dense_demo()
    gray, truth, K, P = slanted[0]
    img = tmp_path / "img"
    img.mkdir()
    for v, g in enumerate(gray):
        (img / f"v{v:02d}.png").write_bytes(_png_bytes(g, 0))
    # sparse points: a grid of the middle view's pinhole pixels lifted with the analytic depth, seen by all
    ys, xs = np.meshgrid(np.arange(8, 60, 8), np.arange(8, 92, 8), indexing="ij")
    z = truth[2][ys.ravel(), xs.ravel()]
    xyz = np.stack([(xs.ravel() - K[0, 2]) / K[0, 0] * z, (ys.ravel() - K[1, 2]) / K[1, 1] * z, z], 1)
    views = [list(range(5))] * len(xyz)
    write_state(tmp_path / "state.bin", P, set(range(5)), xyz, views)
    eps, clouds = mvs.default_opts().eps, {}
    for name, dist in (("set", SET_A), ("zero", (0.0,) * 5)):
        (tmp_path / f"{name}.xml").write_text(XML.format(*K.ravel(), *dist))
        r = subprocess.run([exe, str(img), str(tmp_path / f"{name}.xml"), str(tmp_path / "state.bin"), str(tmp_path / name)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("(undistorted)" in r.stdout) == (name == "set")
        p, nrm, c = clouds[name] = read_dense_ply(tmp_path / name / "models" / "options.txt.ply")
        off = plane_offsets(p, nrm)
        print(f"driver, coefficients {name}: {len(p)} points, relative offset from the plane median {np.median(off):.4f} "
              f"p95 {np.percentile(off, 95):.4f} max {off.max():.4f} (eps {eps})")
        if name == "set":
            assert len(p) > 100 and np.median(off) <= eps and np.percentile(off, 95) <= eps
        else:
            assert len(p) > 0 and np.median(off) > eps
    lo, hi = depth_ranges(P, xyz, views, 5)
    with mvs.Mvs(gray, K, P, bgr=np.stack([gray] * 3, -1), level=1, ctx=ctx, dist=SET_A) as M:     # the driver is the ABI's call
        gx, gn, gc = M.run(lo, hi, mvs.default_opts(min_views=5))
    p, nrm, c = clouds["set"]
    assert _same(p, gx) and _same(nrm, gn) and np.array_equal(c.astype(np.uint32) @ np.array([65536, 256, 1], np.uint32), gc)
