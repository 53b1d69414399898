"""The moving-least-squares smoothing (csrc/mls.h, include/sfmhip.h rules M1-M7) on the CPU, through a g++
build of the header the device kernel compiles (tests/stub/mls_capi.cpp): against a numpy float64 restatement of the rules on
a noisy plane and a noisy sphere cap, the restated exp against libm, the hash-grid search against brute force, M2's grid
against the arithmetic written out, what the smoothing does to the distance from the true surface and to the normals, the
documented edge cases and the refusals.  No GPU.  PARITY UNPINNED: PCL is not in the image."""
import math

import numpy as np
import pytest

from tests.mls_scenes import (ERR_ARG, NAN_BITS, OK, bits, build_stub, noisy_plane, radius_for, reference_mls, sphere_cap, stub_exp,
                              stub_grid, stub_mls, surface_cloud)

N = 2000
CAP_HALF_ANGLE = 0.5
# the largest |stub - restatement| seen on the two scenes below at orders 0, 1 and 2: 5.96e-8 in a coordinate, 2.98e-8 in a
# normal's component, 9.25e-10 in the curvature.  All three are the rounding of the stub's float32 output (half an ulp of a
# coordinate up to 1.3, of a component up to 0.5..1, of a curvature near 0.01): what libm's exp and numpy's summation order
# change in the doubles is below that.  The bounds are four times the figures.
TOL_XYZ, TOL_NORMAL, TOL_CURVATURE = 4 * 5.96e-8, 4 * 2.98e-8, 4 * 9.25e-10
# the largest error of mls.h's exp against libm seen over the arguments of test_exp_against_libm (M6); the test allows one more
EXP_MAX_ULP = 1


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("mls"))


@pytest.fixture(scope="module")
def scenes(ms):
    """name -> (points, radius, {order: (stub, restatement)}), computed once"""
    plane, cap = noisy_plane(N, 1), sphere_cap(N, 2, half_angle=CAP_HALF_ANGLE)
    out = {}
    for name, sc, area in (("plane", plane, 1.0), ("cap", cap, 2 * math.pi * (1 - math.cos(CAP_HALF_ANGLE)))):
        r = radius_for(30, N, area)
        res = {}
        for order in (0, 1, 2):
            rc, got = stub_mls(ms, sc[0], r, order)
            assert rc == OK
            res[order] = (got, reference_mls(sc[0], r, order))
        out[name] = (sc, r, res)
    return out


@pytest.mark.parametrize("name", ["plane", "cap"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_stub_equals_the_numpy_restatement(scenes, name, order):
    got, want = scenes[name][2][order]
    assert got["stats"] == want["stats"] and 25 <= got["stats"]["max_neighbours"] <= 60
    assert np.array_equal(got["src_index"], want["src_index"]) and got["stats"]["n_out"] == N
    d_xyz = np.abs(got["xyz"] - want["xyz"]).max()
    d_n = np.abs(got["normals"][:, :3] - want["normals"][:, :3]).max()
    d_c = np.abs(got["normals"][:, 3] - want["normals"][:, 3]).max()
    print(f"{name} order {order}: max |d xyz| {d_xyz:.3e} |d normal| {d_n:.3e} |d curvature| {d_c:.3e}")
    assert d_xyz <= TOL_XYZ and d_n <= TOL_NORMAL and d_c <= TOL_CURVATURE
    assert np.allclose(np.linalg.norm(got["normals"][:, :3], axis=1), 1.0, atol=1e-6)


def test_exp_against_libm(ms):
    """M6: 350 001 arguments in [-50, 0] (a grid of 200 001 and random ones, some near 0) against math.exp, which is libm's"""
    rng = np.random.default_rng(3)
    x = np.concatenate([np.linspace(-50, 0, 200001), -rng.uniform(0, 50, 100000), -rng.uniform(0, 1, 50000)])
    y = stub_exp(ms, x)
    ref = np.array([math.exp(v) for v in x])
    ulp = int(np.abs(y.view(np.int64) - ref.view(np.int64)).max())
    print(f"exp: largest error {ulp} ulp over {len(x)} arguments")
    assert ulp <= EXP_MAX_ULP + 1
    edge = stub_exp(ms, np.array([0.0, -0.0, -708.0, -708.0000001, -1e9, -np.inf]))
    assert edge[0] == 1.0 and edge[1] == 1.0 and abs(edge[2] / math.exp(-708.0) - 1) < 1e-15 and (edge[3:] == 0.0).all()
    assert np.isnan(stub_exp(ms, np.array([np.nan]))[0])


@pytest.mark.parametrize("order", [0, 2])
def test_hash_grid_search_equals_brute_force(ms, order):
    xyz = surface_cloud(5000, 4)
    xyz[::97] = np.nan
    xyz[5::211, 1] = np.inf
    r = radius_for(30, 5000, 1.0)
    (ra, a), (rb, b) = stub_mls(ms, xyz, r, order, search=1), stub_mls(ms, xyz, r, order, search=2)
    assert ra == OK and rb == OK and a["stats"] == b["stats"] and np.array_equal(a["src_index"], b["src_index"])
    assert np.array_equal(bits(a["xyz"]), bits(b["xyz"])) and np.array_equal(bits(a["normals"]), bits(b["normals"]))
    assert not np.isin(a["src_index"], np.arange(0, 5000, 97)).any() and a["stats"]["n_out"] + a["stats"]["n_dropped"] == np.isfinite(xyz).all(1).sum()


def test_grid_geometry_is_the_written_rule(ms):
    """M2: origin, cell (doubled while the grid exceeds 2^22 cells), axes capped at 2^12, keys x-fastest"""
    rng = np.random.default_rng(6)
    xyz = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    xyz[7] = np.nan
    for r, far in ((0.05, None), (0.002, None), (0.05, [1000.0, 0.5, 0.5])):
        pts = xyz if far is None else np.concatenate([xyz, np.float32([far])])
        fin = np.isfinite(pts).all(1)
        lo, hi = pts[fin].min(0).astype(np.float64), pts[fin].max(0).astype(np.float64)
        cell = r * (1.0 + 1.0 / 1024.0)
        while True:
            D = np.minimum(np.floor((hi - lo) / cell) + 1.0, 4096.0).astype(np.int64)
            if D.prod() <= 1 << 22:
                break
            cell *= 2
        c = np.clip(np.floor((pts[fin].astype(np.float64) - lo) / cell), 0, D - 1).astype(np.int64)
        gcell, gD, keys = stub_grid(ms, pts, r)
        assert gcell == cell and np.array_equal(gD, D) and (keys[~fin] == -1).all()
        assert np.array_equal(keys[fin], (c[:, 2] * D[1] + c[:, 1]) * D[0] + c[:, 0])
        if r == 0.002:
            assert gcell == 4 * r * (1.0 + 1.0 / 1024.0)      # doubled twice
        if far is not None:
            assert gD[0] == 4096 and keys[-1] % 4096 == 4095     # the outlier clamped into the border cell


def test_smoothing_brings_a_noisy_plane_closer_to_the_plane(scenes):
    (xyz, nrm, off), _, res = scenes["plane"]
    before = np.sqrt(((xyz.astype(np.float64) @ nrm - off) ** 2).mean())
    for order in (0, 1, 2):
        after = np.sqrt(((res[order][0]["xyz"].astype(np.float64) @ nrm - off) ** 2).mean())
        print(f"plane order {order}: rms distance {before:.5f} -> {after:.5f}")
        assert after < before


def test_the_polynomial_follows_a_sphere_better_than_the_plane(scenes):
    (_, centre, R), r, res = scenes["cap"]
    rms, angle = {}, {}
    for order in (0, 2):
        got = res[order][0]
        d = got["xyz"].astype(np.float64) - centre
        rad = np.linalg.norm(d, axis=1)
        rms[order] = np.sqrt(((rad - R) ** 2).mean())
        # the points whose whole neighbourhood lies on the cap (a one-sided neighbourhood at the rim constrains neither fit)
        inner = np.arccos(np.clip(d[:, 2] / rad, -1, 1)) < CAP_HALF_ANGLE - r
        cosang = np.abs((got["normals"][:, :3].astype(np.float64) * (d / rad[:, None])).sum(1))   # (M7: the sign is eigen33's)
        angle[order] = np.arccos(np.clip(cosang, 0, 1))[inner].mean()
        print(f"cap order {order}: rms distance to the sphere {rms[order]:.6f}, mean normal error {angle[order]:.6f} rad over {inner.sum()} inner points")
    assert rms[2] < rms[0] and angle[2] < angle[0]


def test_edge_cases(ms):
    rng = np.random.default_rng(8)
    for n in (0, 1, 2):
        rc, got = stub_mls(ms, rng.uniform(0, 0.01, (n, 3)), 1.0)
        assert rc == OK and got["stats"]["n_out"] == 0 and got["stats"]["n_dropped"] == n
    tri = rng.uniform(0, 0.01, (3, 3)).astype(np.float32)
    for order, plane_only in ((0, 0), (1, 0), (2, 3)):      # 3 neighbours: order 1 fits, order 2 keeps the plane
        rc, got = stub_mls(ms, tri, 1.0, order)
        assert rc == OK and got["stats"]["n_out"] == 3 and got["stats"]["n_plane_only"] == plane_only
    same = np.tile(np.float32([[0.25, -0.5, 2.0]]), (70, 1))
    rc, got = stub_mls(ms, same, 0.1)
    assert rc == OK and got["stats"]["n_degenerate"] == 70 and np.array_equal(bits(got["xyz"]), bits(same))
    assert (bits(got["normals"]) == NAN_BITS).all()
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = 0.01 * np.arange(40)
    rc, got = stub_mls(ms, line, 0.1)
    assert rc == OK and got["stats"]["n_degenerate"] == 40 and np.array_equal(bits(got["xyz"]), bits(line))
    k = np.arange(-4, 5, dtype=np.float32)                  # a cross in the plane z = 0: u v = 0 at every neighbour of its centre
    cross = np.concatenate([np.stack([0 * k, 0.01 * k, 0 * k], 1), np.stack([0.01 * k[k != 0], 0 * k[k != 0], 0 * k[k != 0]], 1)])
    rc, got = stub_mls(ms, cross, 1.0)
    assert rc == OK and got["stats"]["n_fit_failed"] >= 1 and got["stats"]["n_out"] == 17
    centre = got["src_index"].tolist().index(4)
    assert np.array_equal(got["xyz"][centre], [0, 0, 0]) and abs(got["normals"][centre, 2]) == 1.0      # M3's result stands
    rc, got = stub_mls(ms, tri, 1.0, normals=False)
    assert rc == OK and got["normals"] is None


def test_refusals(ms):
    xyz = np.random.default_rng(9).uniform(0, 1, (10, 3)).astype(np.float32)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(radius=0.5, order=3),
               dict(radius=0.5, order=-1), dict(radius=0.5, sqr_gauss=np.nan), dict(radius=0.5, sqr_gauss=np.inf)):
        rc, got = stub_mls(ms, xyz, **kw)
        assert rc == ERR_ARG and got["n_out"] == -9 and (got["xyz"] == 7.5).all() and (got["src_index"] == 77).all(), kw
