"""GPU: sfmhip_triangulate (csrc/triangulate.hip, the Jacobi of csrc/pose.h, the camera model of csrc/camera.h) off the
clean scene: the 256-thread block edge, degenerate rows next to healthy lanes of the same wave, degenerate calls, max_err
at a row's own error, and the err = NULL path.  X and err are compared with the oracle as bit patterns, keep with
array_equal; no tolerances.  Every case first asserts on the oracle's answer alone that it exercises what it is for."""
import ctypes as C

import numpy as np
import pytest

from sfm_danpipeline_amd import _lib, synth, triangulate

pytestmark = pytest.mark.gpu

ZERO = np.zeros(5)
MILD = np.array([-0.05, 0.01, 1e-4, -2e-4, 0.001])
STRONG = np.array([-0.9, 2.5, 0.05, -0.05, -3.0])        # the five undistortion iterations do not settle


def same_bits(got, ref, nan_rows=()):
    """Bit for bit, except on the rows listed: there a NaN must meet a NaN in the same entry (the host's and the device's
    default NaN differ in sign) and every entry that is not a NaN is still compared bit for bit."""
    (X, err, keep), (Xo, erro, keepo) = got, ref
    assert np.array_equal(keep, keepo)
    ok = np.ones(len(keepo), bool)
    ok[np.asarray(nan_rows, int)] = False
    assert np.array_equal(X[ok].view(np.uint64), Xo[ok].view(np.uint64))
    assert np.array_equal(err[ok].view(np.uint32), erro[ok].view(np.uint32))
    for a, b, bits in ((X[~ok], Xo[~ok], np.uint64), (err[~ok], erro[~ok], np.uint32)):
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb)
        assert np.array_equal(np.ascontiguousarray(a[~na]).view(bits), np.ascontiguousarray(b[~nb]).view(bits))


def nan_rows_of(X, err):
    return np.nonzero(np.isnan(X).any(1) | np.isnan(err).any(1))[0]


def both(ctx, orc, P1, P2, K, dist, xy1, xy2, max_err=6.0, check=None, nan_rows=()):
    ref = orc.triangulate(P1, P2, K, dist, xy1, xy2, max_err=max_err)
    if len(nan_rows) == 0:
        assert len(nan_rows_of(ref[0], ref[1])) == 0
    if check is not None:
        check(*ref)
    got = triangulate.triangulate_points(P1, P2, K, dist, xy1, xy2, max_err=max_err, ctx=ctx)
    same_bits(got, ref, nan_rows)
    return got, ref


@pytest.mark.parametrize("dist", [ZERO, MILD], ids=["zero", "mild"])
@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_triangulate_block_edge(ctx, orc, m, dist):
    """triangulate_kernel's `live = i < m` at the 256-thread block edge: one block short by a lane, full, one lane into a
    second block (whose 63 idle lanes of wave 0 run the Jacobi on zeros beside it), and into a third."""

    def check(Xo, erro, keepo):
        assert 0 < keepo.sum() < m and np.isfinite(Xo).all()

    sc = synth.two_view_scene(m, seed=m)
    both(ctx, orc, sc["P1"], sc["P2"], sc["K"], dist, sc["xy1"], sc["xy2"], check=check)


@pytest.mark.parametrize("dist", [ZERO, MILD], ids=["zero", "mild"])
@pytest.mark.parametrize("turn", range(4))
def test_triangulate_degenerate_rows_beside_healthy_lanes(ctx, orc, turn, dist):
    """dlt_null_vector's wave-uniform exit (pose.h, `if (!__any(changed)) break`): a NaN / inf / 1e300 observation makes
    its lane rotate through all 30 sweeps (`fabs(p) <= eps * sqrt(a * b)` is false on a NaN) while the 63 healthy lanes
    of its wave, long converged, must see no further rotation and stay bit-equal.  The rows sit at indices 0, 63, 64,
    255, 256 and m - 1; `turn` moves every kind through every place and both views.  Such a row gives a NaN point and NaN
    errors and is KEPT (`!(max_err < e1 || max_err < e2)` in triangulate_kernel, as src/Sfm.cpp:859).  A 1e12
    observation stays finite in the oracle and is dropped: it is compared bit for bit like any healthy row."""
    m = 513
    sc = synth.two_view_scene(m, seed=11)
    xy1, xy2 = sc["xy1"].copy(), sc["xy2"].copy()
    rows = [0, 63, 64, 255, 256, m - 1]
    kinds = [np.nan, np.inf, 1e12, 1e300, -np.inf, -1e300]
    kinds = kinds[turn:] + kinds[:turn]
    for k, (r, v) in enumerate(zip(rows, kinds)):
        (xy1 if (k + turn) % 2 == 0 else xy2)[r, (k + turn // 2) % 2] = v
    must_be_nan = [r for r, v in zip(rows, kinds) if not abs(v) == 1e12]
    ref = orc.triangulate(sc["P1"], sc["P2"], sc["K"], dist, xy1, xy2)
    nan_rows = nan_rows_of(ref[0], ref[1])

    def check(Xo, erro, keepo):
        assert set(must_be_nan) <= set(nan_rows.tolist()) <= set(rows)        # the planted rows and nothing else
        assert np.isnan(Xo[must_be_nan]).all() and np.isnan(erro[must_be_nan]).all() and keepo[must_be_nan].all()
        healthy = np.setdiff1d(np.arange(m), rows)
        assert np.isfinite(Xo[healthy]).all() and 0 < keepo[healthy].sum() < len(healthy)

    both(ctx, orc, sc["P1"], sc["P2"], sc["K"], dist, xy1, xy2, check=check, nan_rows=nan_rows)


def test_triangulate_identical_cameras(ctx, orc):
    """P1 == P2: rows 0, 2 and 1, 3 of every A are built from the same camera, the null space is not a point, and the Jacobi
    runs on a rank-deficient matrix in every lane (pose.h, the `beta < 0` / else branches with near-zero W).  The oracle
    answers with finite points and keeps none."""
    sc = synth.two_view_scene(300, seed=2)

    def check(Xo, erro, keepo):
        assert np.isfinite(Xo).all() and np.isfinite(erro).all() and keepo.sum() == 0

    both(ctx, orc, sc["P1"], sc["P1"], sc["K"], ZERO, sc["xy1"], sc["xy2"], check=check)
    both(ctx, orc, sc["P2"], sc["P2"], sc["K"], MILD, sc["xy1"], sc["xy2"], check=check)


def test_triangulate_epipole_of_a_forward_translation(ctx, orc):
    """A pure forward translation and an observation on the epipole (the principal point, in both views): two rows of A
    vanish identically, the selected singular vector has v[3] == 1 and X = 0 (triangulate_kernel's `scale`), the
    projection divides by z = 0 in the first view (`z ? 1. / z : 1`, camera.h).  Error 0, kept; planted at 0, 63 and 64
    of a batch of 130 ordinary points of the same pair."""
    rng = np.random.default_rng(5)
    K = np.array([[1520.0, 0, 302.2], [0, 1520.0, 246.87], [0, 0, 1]])
    P1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = np.hstack([np.eye(3), np.array([[0.0], [0.0], [-1.0]])])
    Xw = np.stack([rng.uniform(-1, 1, 130), rng.uniform(-1, 1, 130), rng.uniform(4, 8, 130)], 1)
    xy = []
    for P in (P1, P2):
        p = Xw @ P[:, :3].T + P[:, 3]
        xy.append((p[:, :2] / p[:, 2:3]) @ K[:2, :2].T + K[:2, 2] + rng.normal(0, 0.3, (130, 2)))
    rows = [0, 63, 64]
    for a in xy:
        a[rows] = [K[0, 2], K[1, 2]]

    def check(Xo, erro, keepo):
        assert np.all(Xo[rows] == 0) and np.all(erro[rows] == 0) and keepo[rows].all()
        assert np.isfinite(Xo).all() and keepo.sum() > 100

    both(ctx, orc, P1, P2, K, ZERO, xy[0], xy[1], check=check)


def test_triangulate_strong_distortion(ctx, orc):
    """undistort_point's five fixed-point iterations (camera.h) far from convergence and project_point's r^6 term with
    k3 = -3: whatever the iteration lands on, the device lands on the same bits.  300 finite points, 181 kept."""
    sc = synth.two_view_scene(300, seed=2)

    def check(Xo, erro, keepo):
        assert np.isfinite(Xo).all() and np.isfinite(erro).all() and keepo.sum() == 181

    both(ctx, orc, sc["P1"], sc["P2"], sc["K"], STRONG, sc["xy1"], sc["xy2"], check=check)


def test_triangulate_max_err_at_a_rows_own_error(ctx, orc):
    """`keep[i] = !(p.max_err < e1 || p.max_err < e2)` in float (triangulate_kernel; the reference's 6 px test is strict):
    with max_err equal to a row's larger error the row is kept, with the float just below it is dropped.  Then max_err
    of 0 (nothing of a noisy scene survives), +inf (everything does) and NaN (every comparison is false: everything
    does)."""
    sc = synth.two_view_scene(300, seed=8)
    args = (sc["P1"], sc["P2"], sc["K"], MILD, sc["xy1"], sc["xy2"])
    _, erro, keepo = orc.triangulate(*args)
    for row in (0, 64, 255, 256, 299):
        e = np.float32(erro[row].max())
        below = np.nextafter(e, np.float32(0))
        assert 0 < below < e

        def kept(Xo, erro2, keepo2):
            assert keepo2[row] == 1 and np.array_equal(erro2.view(np.uint32), erro.view(np.uint32))

        def dropped(Xo, erro2, keepo2):
            assert keepo2[row] == 0

        both(ctx, orc, *args, max_err=float(e), check=kept)
        both(ctx, orc, *args, max_err=float(below), check=dropped)

    def none(Xo, erro2, keepo2):
        assert keepo2.sum() == 0

    def every(Xo, erro2, keepo2):
        assert keepo2.all()

    both(ctx, orc, *args, max_err=0.0, check=none)
    both(ctx, orc, *args, max_err=float("inf"), check=every)
    both(ctx, orc, *args, max_err=float("nan"), check=every)


def test_triangulate_without_an_error_buffer(ctx, orc):
    """The documented err = NULL (include/sfmhip.h): triangulate_kernel's `if (err)` and the host's skipped copy, through
    a raw ctypes call.  Returns 0; X and keep are those of a call with the buffer."""
    sc = synth.two_view_scene(257, seed=4)
    (X, err, keep), _ = both(ctx, orc, sc["P1"], sc["P2"], sc["K"], MILD, sc["xy1"], sc["xy2"])
    m = 257
    a = [np.ascontiguousarray(v, np.float64) for v in (sc["P1"], sc["P2"], sc["K"], MILD, sc["xy1"], sc["xy2"])]
    X2 = np.full((m, 3), -7.0)
    keep2 = np.full(m, 9, np.uint8)
    rc = _lib.lib().sfmhip_triangulate(ctx.h, *[v.ctypes.data for v in a], m, C.c_float(6.0), X2.ctypes.data, None,
                                       keep2.ctypes.data)
    assert rc == 0
    assert np.array_equal(X2.view(np.uint64), X.view(np.uint64)) and np.array_equal(keep2, keep)
