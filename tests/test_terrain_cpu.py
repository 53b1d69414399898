"""The terrain model (csrc/terrain.h, DESIGN.md f-20: ground points, the terrain raster, height above ground) on the CPU, through
a g++ build of the header the device code compiles (tests/stub/terrain_capi.cpp): a literal Python transcription of rules 2-13
against the stub byte for byte; the opening against scipy.ndimage and by its properties; the window table and the rule cases
built by hand; on the planted terrain scenes the conditions the ground points must meet, the accuracy recorded in DESIGN.md
against the least-squares plane, and the chain into the trees and the dendrometry.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from sfm_danpipeline_amd.terrain import EMPTY, FILLED, GROUND, NO_WINDOW, NONE_SELECTED, TILE, UNFILLED, TerrainOpts, TerrainResult, set_opts
from tests.terrain_scenes import CENTRES, TABLE, plane_heights, scene, surface
from tests.test_dendro_cpu import TOP, dn, rotation, stub_opts as dendro_opts, stub_run as dendro_run  # noqa: F401
from tests.test_ground_cpu import gn, stub_opts as ground_opts, stub_run as ground_run  # noqa: F401
from tests.test_trees_cpu import py_frame_points, stub_opts as trees_opts, stub_run as trees_run, tr  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "terrain_capi.cpp")
RESULT_FIELDS = [f for f, _ in TerrainResult._fields_]
INF = np.float32(np.inf)
# measured on the stub on the two scenes of tests/terrain_scenes.TABLE (seed 1, cell 0.25; DESIGN.md f-20 records them): the RMS
# error of the height above ground over all points, and the worst error of a tree's height; the tests assert 1.25 x these
HAG_RMS = {"gentle": 0.0427, "steep": 0.0524}
TREE_WORST = {"gentle": 0.0708, "steep": 0.0466}


@pytest.fixture(scope="module")
def tn(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("terrain") / "libterraincapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.ter_default_opts.argtypes = [vp]
    lib.ter_default_opts.restype = None
    lib.ter_sizes.argtypes = [vp, vp]
    lib.ter_run.argtypes = [ci, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    lib.ter_raster.argtypes = [vp, vp, vp]
    lib.ter_windows.argtypes = [vp, vp, vp, vp]
    lib.ter_open.argtypes = [vp, ci, ci, ci, vp]
    lib.ter_open.restype = None
    lib.ter_opts_from_ground.argtypes = [vp, vp]
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_terrain.py)
def stub_opts(tn, **kw):
    o = TerrainOpts()
    tn.ter_default_opts(C.byref(o))
    return set_opts(o, **kw)


def result_bytes(r):
    return bytes(memoryview(r))


def stub_run(tn, xyz, labels=None, label=0, opts=None):
    """dict(is_ground, hag, norm, dtm, kind, chm, res); None when the call is refused."""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32))
    n, n1 = len(xyz), max(len(xyz), 1)
    is_ground, hag, norm, res = np.zeros(n1, np.int32), np.zeros(n1, np.float32), np.zeros((n1, 3), np.float32), TerrainResult()
    rc = tn.ter_run(n, xyz.ctypes.data, None if lab is None else lab.ctypes.data, label, C.byref(opts or stub_opts(tn)),
                    is_ground.ctypes.data, hag.ctypes.data, norm.ctypes.data, C.byref(res))
    if rc != 0:
        return None
    m = max(res.De * res.Dn, 1)
    dtm, kind, chm = np.empty(m, np.float32), np.empty(m, np.uint8), np.empty(m, np.float32)
    assert tn.ter_raster(dtm.ctypes.data, kind.ctypes.data, chm.ctypes.data) == res.De * res.Dn
    shape = (res.Dn, res.De)
    return dict(is_ground=is_ground[:n], hag=hag[:n], norm=norm[:n], dtm=dtm[:m if res.De else 0].reshape(shape).copy(),
                kind=kind[:m if res.De else 0].reshape(shape).copy(), chm=chm[:m if res.De else 0].reshape(shape).copy(), res=res)


ARRAYS = ("is_ground", "hag", "norm", "dtm", "kind", "chm")


def same_run(a, b):
    """Two runs hold the same bytes in every array and in the result."""
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in ARRAYS) and result_bytes(a["res"]) == result_bytes(b["res"])


def show(run):
    return {f: getattr(run["res"], f) for f in RESULT_FIELDS}, {k: int((run[k] != run[k]).sum()) for k in ("hag", "dtm", "chm")}


def stub_open(tn, Z, k):
    Z = np.ascontiguousarray(Z, np.float32)
    O = np.empty_like(Z)
    tn.ter_open(Z.ctypes.data, Z.shape[1], Z.shape[0], int(k), O.ctypes.data)
    return O


def stub_windows(tn, o):
    k, kd, dh = np.zeros(32, np.int32), np.zeros(32, np.float64), np.zeros(32, np.float64)
    m = tn.ter_windows(C.byref(o), k.ctypes.data, kd.ctypes.data, dh.ctypes.data)
    return None if m < 0 else (list(k[:m]), list(kd[:m]), list(dh[:m]))


def at(*pts):
    return np.array(pts, np.float32).reshape(-1, 3)


# ---------------------------------------------------------------- the transcription of rules 2-13
def py_windows(o):
    """Rule 5: (k_i, dh_i)."""
    c = o.cell / o.scale
    cells, d0, dmax = (o.max_window / o.scale) / c, o.initial_distance / o.scale, o.max_distance / o.scale
    ks, dhs = [], []
    for i in range(32):
        k = o.base ** i if o.exponential else (i + 1) * o.base
        if not float(2 * k + 1) <= cells:
            break
        dhs.append(d0 if i == 0 else min(dmax, o.slope * (float(2 * (k - ks[-1])) * c) + d0))
        ks.append(k)
    return ks, dhs


def py_extremum(A, k, axis, op, start):
    """The running extremum of half-width k along one axis, the window clipped at the raster's edge."""
    L = A.shape[axis]
    out = np.full_like(A, start)
    for s in range(-min(k, L - 1), min(k, L - 1) + 1):
        dst = [slice(None), slice(None)]
        src = [slice(None), slice(None)]
        dst[axis], src[axis] = slice(max(0, -s), L - max(0, s)), slice(max(0, s), L - max(0, -s))
        out[tuple(dst)] = op(out[tuple(dst)], A[tuple(src)])
    return out


def py_open(Z, k):
    """Rule 6 on a [Dn, De] raster whose empty cells are +inf."""
    E = py_extremum(py_extremum(Z, k, 1, np.minimum, INF), k, 0, np.minimum, INF)
    E = np.where(np.isposinf(E), -INF, E)
    O = py_extremum(py_extremum(E, k, 1, np.maximum, -INF), k, 0, np.maximum, -INF)
    return np.where(np.isneginf(O), INF, O)


def py_run(xyz, labels, label, o):
    """The arrays and the result's fields by rules 2-13, written from DESIGN.md f-20 with numpy and plain loops; None when the
    raster's cap refuses the call."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    nan32 = np.float32(np.nan)
    out = dict(is_ground=np.zeros(n, np.int32), hag=np.full(n, nan32), norm=np.full((n, 3), nan32), dtm=np.zeros((0, 0), np.float32),
               kind=np.zeros((0, 0), np.uint8), chm=np.zeros((0, 0), np.float32))
    c = o.cell / o.scale
    res = dict(c=c, e_min=0.0, n_min=0.0, t_min=nan32, t_max=nan32, hag_max=nan32, De=0, Dn=0, n_selected=0, n_ground=0, n_windows=0,
               n_kind1=0, n_kind2=0, n_kind0=0, fill_rounds=0, flags=NONE_SELECTED, pad=0)
    out["res"] = res
    fr, sel = py_frame_points(xyz, labels, label, o)
    res["n_selected"] = int(sel.sum())
    if not sel.any():
        return out
    res["flags"] = 0
    S = np.nonzero(sel)[0]
    e, nn, h = (fr[S, a].astype(np.float64) for a in range(3))
    # rule 3
    e_min, n_min, e_max, n_max = (float(v) for v in (fr[S, 0].min(), fr[S, 1].min(), fr[S, 0].max(), fr[S, 1].max()))
    De, Dn = math.floor((e_max - e_min) / c) + 1, math.floor((n_max - n_min) / c) + 1
    if float(De) * float(Dn) > 2.0 ** 24:
        return None
    res.update(e_min=e_min, n_min=n_min, De=De, Dn=Dn)
    ix, iy = np.floor((e - e_min) / c).astype(np.int64), np.floor((nn - n_min) / c).astype(np.int64)
    cell = iy * De + ix
    # rule 4
    Z = np.full(De * Dn, INF, np.float32)
    np.minimum.at(Z, cell, fr[S, 2])
    Z = Z.reshape(Dn, De)
    # rules 5 - 7
    ks, dhs = py_windows(o)
    res["n_windows"] = len(ks)
    if not ks:
        res["flags"] |= NO_WINDOW
    ground = np.ones(len(S), bool)
    for k, dh in zip(ks, dhs):
        Z = py_open(Z, k)
        ground &= h - Z.reshape(-1)[cell].astype(np.float64) <= dh
    out["is_ground"][S] = ground
    res["n_ground"] = int(ground.sum())
    # rule 8: a cell's run is its selected points in ascending input index
    T, kind = np.full(De * Dn, nan32), np.zeros(De * Dn, np.uint8)
    order = np.argsort(cell, kind="stable")
    bounds = np.nonzero(np.diff(cell[order], prepend=-1, append=De * Dn + 1))[0]
    for a, b in zip(bounds[:-1], bounds[1:]):
        run = order[a:b]
        slot, m = [0.0] * 64, 0
        for j, i in enumerate(run):
            if ground[i]:
                slot[j % 64] = slot[j % 64] + float(h[i])
                m += 1
        if not m:
            continue
        stride = 32
        while stride >= 1:
            for s in range(stride):
                slot[s] = slot[s] + slot[s + stride]
            stride //= 2
        T[cell[run[0]]], kind[cell[run[0]]] = np.float32(slot[0] / float(m)), GROUND
    T, kind = T.reshape(Dn, De), kind.reshape(Dn, De)

    def shifted(A, dx, dy, fill):
        """A[y + dy, x + dx], `fill` outside the raster."""
        P = np.full((Dn + 2, De + 2), fill, A.dtype)
        P[1:-1, 1:-1] = A
        return P[1 + dy:1 + dy + Dn, 1 + dx:1 + dx + De]

    # rule 9
    for r in range(1, o.fill_rounds + 1):
        s, m = np.zeros((Dn, De), np.float64), np.zeros((Dn, De), np.int64)
        for dx, dy in ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
            has = shifted(kind, dx, dy, EMPTY) != EMPTY
            s = np.where(has, s + shifted(T, dx, dy, nan32).astype(np.float64), s)
            m += has
        take = (kind == EMPTY) & (m > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            T = np.where(take, (s / m.astype(np.float64)).astype(np.float32), T)
        kind = np.where(take, np.uint8(FILLED), kind)
        res["fill_rounds"] = r
        if not take.any():
            break
    # rule 10
    for _ in range(o.relax_sweeps):
        own = T.astype(np.float64)
        W, E, S_, N = (np.where(shifted(kind, dx, dy, EMPTY) != EMPTY, shifted(T, dx, dy, nan32).astype(np.float64), own)
                       for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)))
        T = np.where(kind == FILLED, (((W + E) + (S_ + N)) / 4.0).astype(np.float32), T)
    res.update(n_kind1=int((kind == GROUND).sum()), n_kind2=int((kind == FILLED).sum()), n_kind0=int((kind == EMPTY).sum()))
    if res["n_kind0"]:
        res["flags"] |= UNFILLED
    if (kind != EMPTY).any():
        res.update(t_min=T[kind != EMPTY].min(), t_max=T[kind != EMPTY].max())
    # rule 11
    Tf, kf = T.reshape(-1), kind.reshape(-1)

    def stencil(v, v_min, D):
        u = (v - v_min) / c - 0.5
        i0 = np.clip(np.floor(u), 0, D - 1)
        return i0.astype(np.int64), np.minimum(i0 + 1, D - 1).astype(np.int64), np.clip(u - i0, 0.0, 1.0)

    x0, x1, fx = stencil(e, e_min, De)
    y0, y1, fy = stencil(nn, n_min, Dn)
    own = Tf[cell].astype(np.float64)
    corner = lambda y, x: np.where(kf[y * De + x] != EMPTY, Tf[y * De + x].astype(np.float64), own)
    T00, T01, T10, T11 = corner(y0, x0), corner(y0, x1), corner(y1, x0), corner(y1, x1)
    g = ((T00 * (1.0 - fx) + T01 * fx) * (1.0 - fy)) + ((T10 * (1.0 - fx) + T11 * fx) * fy)
    with np.errstate(invalid="ignore", over="ignore"):
        hag = np.where(kf[cell] != EMPTY, (h - g).astype(np.float32), nan32)
    out["hag"][S] = hag
    fin = np.isfinite(hag)
    out["norm"][S[fin]] = np.stack([fr[S[fin], 0], fr[S[fin], 1], hag[fin]], 1)
    # rule 12
    chm = np.full(De * Dn, -INF, np.float32)
    np.maximum.at(chm, cell[fin], hag[fin])
    out.update(dtm=T, kind=kind, chm=np.where(np.isneginf(chm), nan32, chm).reshape(Dn, De))
    if fin.any():
        res["hag_max"] = hag[fin].max()
    return out


def assert_transcribed(got, want):
    """The stub's run `got` against the transcription `want`."""
    for k in ARRAYS:
        assert got[k].shape == want[k].shape and got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    for f in RESULT_FIELDS:
        a, b = getattr(got["res"], f), want["res"][f]
        if f in ("e_min", "n_min", "t_min", "t_max", "hag_max"):
            assert np.float32(a).tobytes() == np.float32(b).tobytes(), (f, a, b)
        else:
            assert a == b, (f, a, b)


def small_scene(seed=3, **kw):
    return scene(seed, n_tree=1500, n_ground=6000, **kw)


def transcription_cases(tn, gn):
    """name -> (xyz, labels, label, opts): the scenes both the transcription and the device are checked on."""
    cases = {}
    xyz, member, _, _ = small_scene()
    cases["plain"] = (xyz, None, 0, stub_opts(tn))
    cases["labels"] = (xyz, (member == 2).astype(np.int32), 0, stub_opts(tn, cell=0.4, exponential=0, base=2))
    nan = xyz.copy()
    nan[::97, 0], nan[5::131, 2] = np.nan, np.inf
    cases["nan"] = (nan, None, 0, stub_opts(tn, cell=0.25))
    scale = 0.37
    rxyz, _, _, R = small_scene(rot=12, scale=scale)
    g = ground_run(gn, rxyz, opts=ground_opts(gn, inlier_tol=0.5 / scale))
    assert g.flags == 0
    o = stub_opts(tn, scale=scale)
    assert tn.ter_opts_from_ground(C.byref(g), C.byref(o)) == 0 and tuple(o.up) == tuple(g.up) and tuple(o.north) == tuple(g.north)
    cases["rot_scale"] = (rxyz, None, 0, o)
    return cases


# ---------------------------------------------------------------- the tests
def test_struct_sizes_and_defaults(tn):
    so, sr = C.c_int(0), C.c_int(0)
    tn.ter_sizes(C.byref(so), C.byref(sr))
    assert (so.value, sr.value) == (C.sizeof(TerrainOpts), C.sizeof(TerrainResult)) == (112, 72)
    o = stub_opts(tn)
    assert (o.cell, o.max_window, o.slope, o.initial_distance, o.max_distance) == (0.5, 9.0, 1.0, 0.15, 2.5)
    assert (o.base, o.exponential, o.fill_rounds, o.relax_sweeps, o.scale) == (2, 1, 64, 32, 1.0)
    assert tuple(o.up) == (0, 0, 1) and tuple(o.north) == (0, 1, 0)


@pytest.mark.parametrize("name", ["plain", "labels", "nan", "rot_scale"])
def test_transcription_gives_the_same_bytes(tn, gn, name):
    xyz, lab, label, o = transcription_cases(tn, gn)[name]
    got = stub_run(tn, xyz, lab, label, o)
    assert_transcribed(got, py_run(xyz, lab, label, o))
    r = got["res"]
    assert r.flags == 0 and r.n_windows >= 3 and r.n_kind2 > 0 and 0 < r.n_ground < r.n_selected


def random_raster(seed, Dn, De, empty):
    rng = np.random.default_rng(seed)
    Z = rng.normal(0, 1, (Dn, De)).astype(np.float32)
    if empty:
        Z[rng.uniform(size=Z.shape) < empty] = INF
    return Z


@pytest.mark.parametrize("empty", [0.0, 0.3, 0.9])
@pytest.mark.parametrize("k", [1, 2, 7, 13, 39])
def test_opening_equals_scipys_grey_filters(tn, empty, k):
    """Rule 6 against minimum_filter / maximum_filter with constant borders that never win; 13 is the raster's width, 39 three times it."""
    Z = random_raster(10 * k + int(10 * empty), 11, 13, empty)
    E = ndimage.minimum_filter(Z, size=2 * k + 1, mode="constant", cval=np.inf)
    O = ndimage.maximum_filter(np.where(np.isposinf(E), -INF, E), size=2 * k + 1, mode="constant", cval=-np.inf)
    want = np.where(np.isneginf(O), INF, O).astype(np.float32)
    assert stub_open(tn, Z, k).tobytes() == want.tobytes() == py_open(Z, k).tobytes()


def test_opening_properties(tn):
    Z = random_raster(5, 40, 37, 0.2)
    for k in (1, 3, 8):
        O = stub_open(tn, Z, k)
        full = ~np.isposinf(Z)
        assert (O[full] <= Z[full]).all() and not np.isposinf(O[full]).any()          # anti-extensive where Z has a value
        assert stub_open(tn, O, k).tobytes() == O.tobytes()                          # idempotent
    y, x = np.mgrid[0:40, 0:37]
    plane = (0.25 * x - 0.125 * y + 3.0).astype(np.float32)                           # (exact in float32)
    for k in (1, 4, 9):
        O = stub_open(tn, plane, k)
        assert np.array_equal(O[k:-k, k:-k], plane[k:-k, k:-k])                       # the plane, k cells inside
        assert (O <= plane).all() and (O[:, -1] < plane[:, -1]).all()                 # the upslope edge is flattened


def test_window_table_by_hand(tn):
    o = stub_opts(tn)                                                                 # 9 m / 0.5 m = 18 cells: 3, 5, 9, 17
    k, kd, dh = stub_windows(tn, o)
    assert k == [1, 2, 4, 8] and kd == [1.0, 2.0, 4.0, 8.0] and dh == [0.15, 1.0 * (2.0 * 0.5) + 0.15, 1.0 * (4.0 * 0.5) + 0.15, 2.5]
    assert (k, dh) == py_windows(o)
    o = stub_opts(tn, exponential=0, base=3, max_window=7.0, cell=0.25, slope=0.1)     # 28 cells: k = 3, 6, 9, 12
    k, kd, dh = stub_windows(tn, o)
    assert k == [3, 6, 9, 12] and dh == [0.15] + [0.1 * (6.0 * 0.25) + 0.15] * 3 and (k, dh) == py_windows(o)
    o = stub_opts(tn, scale=0.5, max_window=9.0, base=3)                              # lengths double: 18 cells still: 3, 7
    k, kd, dh = stub_windows(tn, o)
    assert k == [1, 3] and dh == [0.3, 1.0 * (4.0 * 1.0) + 0.3] and (k, dh) == py_windows(o)
    assert stub_windows(tn, stub_opts(tn, max_window=1.49))[0] == [] == py_windows(stub_opts(tn, max_window=1.49))[0]   # below three cells
    assert stub_windows(tn, stub_opts(tn, max_window=1.5))[0] == [1]
    k, kd, dh = stub_windows(tn, stub_opts(tn, exponential=0, max_window=1000.0))     # the cap of 32: k = 2 .. 64
    assert k == list(range(2, 66, 2)) and dh[1:] == [2.15] * 31
    k, kd, dh = stub_windows(tn, stub_opts(tn, max_window=1e300, cell=1e-3, base=1 << 20))
    assert len(k) == 32 and k[:3] == [1, 1 << 20, 1 << 24] and kd[2] == 2.0 ** 40 and kd[31] == 2.0 ** 620   # capped for the opening only
    xyz = small_scene()[0]
    r = stub_run(tn, xyz, opts=stub_opts(tn, max_window=1.0))
    assert r["res"].flags == NO_WINDOW and r["res"].n_windows == 0 and r["is_ground"].all() and r["res"].n_ground == len(xyz)


def test_one_point_three_points_and_a_one_row_raster(tn):
    r = stub_run(tn, at((1, 2, 3)))
    assert (r["res"].De, r["res"].Dn, r["res"].n_ground, r["res"].n_kind1, r["res"].flags) == (1, 1, 1, 1, 0)
    assert list(r["is_ground"]) == [1] and r["hag"][0] == 0 and r["dtm"][0, 0] == 3 and r["chm"][0, 0] == 0 and r["res"].fill_rounds == 1
    assert r["norm"].tolist() == [[1, 2, 0]]
    three = at((0, 0, 1.0), (0.1, 0.2, 1.25), (0.3, 0.1, 5.0))                        # one cell: the third is 4 above its lowest point
    r = stub_run(tn, three)
    assert list(r["is_ground"]) == [1, 0, 0] and r["dtm"][0, 0] == 1.0 and list(r["hag"]) == [0.0, 0.25, 4.0] and r["chm"][0, 0] == 4.0
    r = stub_run(tn, three, opts=stub_opts(tn, initial_distance=0.25))
    assert list(r["is_ground"]) == [1, 1, 0] and r["dtm"][0, 0] == np.float32((1.0 + 1.25) / 2.0)
    assert_transcribed(r, py_run(three, None, 0, stub_opts(tn, initial_distance=0.25)))
    row = at((0, 0, 0), (2.6, 0.1, 0.5), (5.2, 0.2, 0.25), (1.3, 0.3, 9.0))           # Dn = 1, De = 11
    r = stub_run(tn, row)
    assert (r["res"].De, r["res"].Dn) == (11, 1) and list(r["is_ground"]) == [1, 1, 1, 0] and r["res"].n_kind0 == 0
    assert_transcribed(r, py_run(row, None, 0, stub_opts(tn)))
    col = row[:, [1, 0, 2]]
    r2 = stub_run(tn, col)
    assert (r2["res"].De, r2["res"].Dn) == (1, 11) and np.array_equal(r2["dtm"].T, r["dtm"]) and np.array_equal(r2["hag"], r["hag"])


def test_the_fold_of_a_cell_of_65_ground_points(tn):
    """65 points of one cell whose sum depends on the order: slot 0 takes points 0 and 64 before the fold."""
    rng = np.random.default_rng(4)
    pts = np.zeros((65, 3), np.float32)
    pts[:, :2] = rng.uniform(0.0, 0.4, (65, 2))
    pts[:, 2] = (1e3 + rng.uniform(0, 0.1, 65)).astype(np.float32)
    pts[:2, :2] = (0, 0), (0.45, 0.45)
    r = stub_run(tn, pts)
    want = py_run(pts, None, 0, stub_opts(tn))
    assert_transcribed(r, want)
    assert r["res"].n_ground == 65 and r["res"].De == 1
    h = pts[:, 2].astype(np.float64)
    slot = [float(h[j]) for j in range(64)]
    slot[0] = slot[0] + float(h[64])
    for stride in (32, 16, 8, 4, 2, 1):
        for s in range(stride):
            slot[s] = slot[s] + slot[s + stride]
    assert r["dtm"][0, 0] == np.float32(slot[0] / 65.0)


def ring_with_a_hole(width=21, cell=0.5):
    """Ground on the border cells of a width x width raster, nothing inside, and one point high above the middle."""
    c = (np.arange(width) + 0.5) * cell
    x, y = np.meshgrid(c, c)
    edge = (x < cell) | (y < cell) | (x > (width - 1) * cell) | (y > (width - 1) * cell)
    pts = np.column_stack([x[edge], y[edge], 0.125 * x[edge]])
    pts[0, :2], pts[-1, :2] = (0.0, 0.0), (width * cell - 0.01, width * cell - 0.01)
    mid = (width // 2 + 0.25) * cell
    return np.concatenate([pts, [[mid, mid, 30.0]]]).astype(np.float32)


def test_a_hole_deeper_than_the_fill_and_the_stencil_at_its_rim(tn):
    pts = ring_with_a_hole()
    full = stub_run(tn, pts)                                                          # the default 64 rounds close it: 10 rings
    assert full["res"].flags == 0 and full["res"].n_kind0 == 0 and full["res"].fill_rounds == 11 and full["res"].n_kind2 == 19 * 19
    assert_transcribed(full, py_run(pts, None, 0, stub_opts(tn)))
    assert abs(full["hag"][-1] - (30.0 - 0.125 * 5.25)) < 0.05 and full["is_ground"][-1] == 0
    o = stub_opts(tn, fill_rounds=3)
    r = stub_run(tn, pts, opts=o)
    assert_transcribed(r, py_run(pts, None, 0, o))
    assert r["res"].flags == UNFILLED and r["res"].fill_rounds == 3 and r["res"].n_kind0 == 13 * 13 and np.isnan(r["dtm"][10, 10])
    assert np.isnan(r["hag"][-1]) and np.isnan(r["norm"][-1]).all() and np.isnan(r["chm"][10, 10])     # rule 11: its cell has kind 0
    assert np.isfinite(r["hag"][:-1]).all()
    # a point at the inner corner of the innermost filled ring, in the quarter of its cell that looks at the hole: the far corner of
    # its stencil has kind 0 and counts as the cell's own value
    probe = np.concatenate([pts[:-1], [[1.5 + 0.45, 1.5 + 0.45, 20.0]]]).astype(np.float32)
    r = stub_run(tn, probe, opts=o)
    assert r["kind"][3, 3] == FILLED and r["kind"][3, 4] == FILLED and r["kind"][4, 3] == FILLED and r["kind"][4, 4] == EMPTY
    f = np.float64(probe[-1, 0]) / 0.5 - 0.5 - 3.0
    T = r["dtm"].astype(np.float64)
    g = ((T[3, 3] * (1.0 - f) + T[3, 4] * f) * (1.0 - f)) + ((T[4, 3] * (1.0 - f) + T[3, 3] * f) * f)
    assert 0.35 < f < 0.45 and r["is_ground"][-1] == 0 and r["hag"][-1] == np.float32(20.0 - g)
    assert_transcribed(r, py_run(probe, None, 0, o))


def test_no_fill_and_no_relaxation(tn):
    pts = ring_with_a_hole(9)
    o = stub_opts(tn, fill_rounds=0)
    r = stub_run(tn, pts, opts=o)
    assert r["res"].fill_rounds == 0 and r["res"].n_kind2 == 0 and r["res"].n_kind0 == 49 and r["res"].flags == UNFILLED
    assert_transcribed(r, py_run(pts, None, 0, o))
    o = stub_opts(tn, relax_sweeps=0)
    a, b = stub_run(tn, pts, opts=o), stub_run(tn, pts)
    assert_transcribed(a, py_run(pts, None, 0, o))
    assert np.array_equal(a["kind"], b["kind"]) and not np.array_equal(a["dtm"], b["dtm"])
    assert np.array_equal(a["dtm"][a["kind"] == GROUND], b["dtm"][b["kind"] == GROUND])     # the relaxation leaves the ground cells alone


REFUSALS = [dict(cell=0.0), dict(cell=-1.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(initial_distance=0.0),
            dict(initial_distance=float("inf")), dict(max_distance=0.0), dict(max_distance=float("nan")), dict(max_window=-1.0),
            dict(max_window=float("inf")), dict(slope=-0.5), dict(slope=float("nan")), dict(base=1), dict(base=-3), dict(fill_rounds=-1),
            dict(fill_rounds=4097), dict(relax_sweeps=-1), dict(relax_sweeps=1025), dict(scale=0.0), dict(scale=float("inf")),
            dict(up=(0, 0, 2)), dict(north=(0, 0, 1)), dict(cell=1e-300, scale=1e300)]


@pytest.mark.parametrize("kw", REFUSALS)
def test_refusals(tn, kw):
    assert stub_run(tn, at((0, 0, 0), (1, 1, 1)), opts=stub_opts(tn, **kw)) is None


def test_edges_of_the_options_and_the_cap(tn):
    pts = at((0, 0, 0), (1, 1, 1))
    for kw in (dict(max_window=0.0), dict(slope=0.0), dict(base=2), dict(fill_rounds=4096), dict(relax_sweeps=1024), dict(fill_rounds=0)):
        assert stub_run(tn, pts, opts=stub_opts(tn, **kw)) is not None
    assert stub_run(tn, at((0, 0, 0), (4096, 4095, 0)), opts=stub_opts(tn, cell=1.0)) is None          # 4097 x 4096 cells
    assert py_run(at((0, 0, 0), (4096, 4095, 0)), None, 0, stub_opts(tn, cell=1.0)) is None
    r = stub_run(tn, at((0, 0, 0), (4095, 4095, 0)), opts=stub_opts(tn, cell=1.0, fill_rounds=1, relax_sweeps=0, max_window=3.0))
    assert r["res"].De * r["res"].Dn == 1 << 24 and r["res"].n_kind2 == 6
    r = stub_run(tn, pts, np.zeros(2, np.int32), 1)                                                    # nobody has label 1
    assert r["res"].flags == NONE_SELECTED and (r["res"].De, r["res"].Dn) == (0, 0) and not r["is_ground"].any() and np.isnan(r["hag"]).all()
    assert np.isnan(r["norm"]).all() and r["dtm"].size == 0
    assert_transcribed(r, py_run(pts, np.zeros(2, np.int32), 1, stub_opts(tn)))
    assert stub_run(tn, np.zeros((0, 3), np.float32))["res"].flags == NONE_SELECTED


# ---------------------------------------------------------------- the planted scenes
@pytest.fixture(scope="module")
def table_runs(tn):
    """name -> (xyz, member, above, the stub's run) on the two scenes of the table."""
    out = {}
    for name, (a, s, cell) in TABLE.items():
        xyz, member, above, _ = scene(1, a, s)
        out[name] = (xyz, member, above, stub_run(tn, xyz, opts=stub_opts(tn, cell=cell)))
    return out


def test_ground_points_on_the_planted_scenes(tn, table_runs):
    xyz, member, above, _ = scene(2, 0.0, 0.0, n_tree=4000, n_ground=20000)
    r = stub_run(tn, xyz)
    assert r["is_ground"][member < 0].all()                                           # flat: every true ground point
    assert not r["is_ground"][(member >= 0) & (above > 0.5)].any()
    for name, (xyz, member, above, r) in table_runs.items():
        assert not r["is_ground"][(member >= 0) & (above > 0.5)].any(), name
        assert r["is_ground"][member < 0].mean() > 0.9, name
    xyz, member, above, _ = scene(1, 1.0, 0.25, n_tree=4000, n_ground=20000)
    for cell in (0.5, 1.0):
        r = stub_run(tn, xyz, opts=stub_opts(tn, cell=cell))
        assert not r["is_ground"][(member >= 0) & (above > 0.5)].any(), cell


def accuracy(xyz, member, above, hag):
    """(RMS error of the heights above ground, the worst error of a tree's height)."""
    hag = hag.astype(np.float64)
    assert np.isfinite(hag).all()
    rms = math.sqrt(((hag - above) ** 2).mean())
    worst = max(abs(hag[member == k].max() - above[member == k].max()) for k in range(len(CENTRES)))
    return rms, worst


@pytest.mark.parametrize("name", list(TABLE))
def test_accuracy_against_the_analytic_terrain_and_the_plane(table_runs, name):
    xyz, member, above, r = table_runs[name]
    rms, worst = accuracy(xyz, member, above, r["hag"])
    prms, pworst = accuracy(xyz, member, above, plane_heights(xyz, member))
    print(f"{name}: terrain rms {rms:.4f} worst tree {worst:.4f}; plane rms {prms:.4f} worst tree {pworst:.4f}")
    assert rms <= 1.25 * HAG_RMS[name] and worst <= 1.25 * TREE_WORST[name]
    assert rms < prms and worst < pworst


@pytest.mark.parametrize("name", list(TABLE))
def test_chain_into_the_trees_and_the_dendrometry(tr, dn, table_runs, name):
    """The trees and dendrometry stubs on the normalised cloud, up +z and ground 0: the five planted trees at their heights."""
    xyz, member, above, r = table_runs[name]
    tree_of, stems, res = trees_run(tr, r["norm"], opts=trees_opts(tr, ground=0.0))
    assert res.n_trees == 5 and res.flags == 0
    centres = np.array(CENTRES)
    for s in range(5):
        k = int(np.argmin(np.hypot(*(centres - (stems[s]["e"], stems[s]["n"])).T)))
        assert math.hypot(stems[s]["e"] - centres[k, 0], stems[s]["n"] - centres[k, 1]) < 0.1
        assert (member[tree_of == s] == k).mean() > 0.99
        d = dendro_run(dn, r["norm"], tree_of, s, dendro_opts(dn, ground=0.0))[0]
        # (on a slope the tree's greatest height above the terrain is a crown point's downslope of the stem, not the planted top's)
        assert above[member == k].max() >= TOP and abs(d.total_height - above[member == k].max()) <= 1.25 * TREE_WORST[name], (s, d.total_height)
        assert abs(d.dbh - 0.3) < 0.02, (s, d.dbh)
