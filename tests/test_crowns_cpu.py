"""The crown delineation (csrc/crowns.h, DESIGN.md f-21: tree tops and crowns from the canopy raster) on the CPU, through a g++
build of the header the device code compiles (tests/stub/crowns_capi.cpp): a literal Python transcription of rules 3-11 against
the stub byte for byte; the smoothing and the tops against scipy.ndimage; the rule cases built by hand; on the planted crown
scenes the conditions the tops and the tree numbers must meet and the shares DESIGN.md records; and the capability itself: a
plot without stem points, where the stem route finds nothing, gives its six trees.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from sfm_danpipeline_amd.crowns import BATCH, NO_CANOPY, OVERFLOW, TILE, TOP_DTYPE, CrownsOpts, CrownsResult, set_opts
from tests.crown_scenes import APART, TOUCHING, max_raster, scene
from tests.test_ground_cpu import gn, stub_opts as ground_opts, stub_run as ground_run  # noqa: F401
from tests.test_terrain_cpu import stub_opts as terrain_opts, stub_run as terrain_run, tn  # noqa: F401
from tests.test_trees_cpu import stub_opts as trees_opts, stub_run as trees_run, tr  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "crowns_capi.cpp")
RESULT_FIELDS = [f for f, _ in CrownsResult._fields_]
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def cn(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("crowns") / "libcrownscapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.crn_default_opts.argtypes = [vp]
    lib.crn_default_opts.restype = None
    lib.crn_sizes.argtypes = [vp, vp, vp]
    lib.crn_run.argtypes = [vp, ci, ci, C.c_double, C.c_float, C.c_float, vp, vp, vp, ci, vp, vp]
    lib.crn_points.argtypes = [ci, vp, vp, vp, vp, ci, vp, vp]
    lib.crn_window.argtypes = [vp, C.c_double, C.c_float]
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_crowns.py)
def stub_opts(cn, **kw):
    o = CrownsOpts()
    cn.crn_default_opts(C.byref(o))
    return set_opts(o, **kw)


def result_bytes(r):
    return bytes(memoryview(r))


def stub_run(cn, Z, c, opts=None, e_min=0.0, n_min=0.0, cap=65536):
    """dict(labels [Dn, De], smooth [Dn, De], tops, res) of a raster; None when the call is refused."""
    Z = np.ascontiguousarray(np.asarray(Z, np.float32))
    dn, de = Z.shape
    m = max(dn * de, 1)
    labels, smooth, tops, res = np.full(m, -1, np.int32), np.full(m, np.nan, np.float32), np.zeros(max(cap, 1), TOP_DTYPE), CrownsResult()
    o = opts or stub_opts(cn)
    if cn.crn_run(Z.ctypes.data, de, dn, float(c), e_min, n_min, C.byref(o), labels.ctypes.data, smooth.ctypes.data, cap, tops.ctypes.data,
                  C.byref(res)) != 0:
        return None
    return dict(labels=labels[:dn * de].reshape(dn, de), smooth=smooth[:dn * de].reshape(dn, de),
                tops=tops[:min(cap, res.n_trees, o.max_trees)].copy(), res=res)


def stub_points(cn, enh, hag, opts, cap=65536):
    """Rule 10 after a stub_run on a terrain call's canopy raster: (tree_of, tops, res)."""
    enh, hag = np.ascontiguousarray(enh, np.float32).reshape(-1, 3), np.ascontiguousarray(hag, np.float32)
    n = len(hag)
    tree_of, tops, res = np.full(max(n, 1), -1, np.int32), np.zeros(max(cap, 1), TOP_DTYPE), CrownsResult()
    assert cn.crn_points(n, enh.ctypes.data, hag.ctypes.data, C.byref(opts), tree_of.ctypes.data, cap, tops.ctypes.data, C.byref(res)) == 0
    return tree_of[:n], tops[:min(cap, res.n_trees, opts.max_trees)].copy(), res


def stub_cloud_run(cn, t, opts, cap=65536):
    """The cloud entry by the stubs: `t` is tests/test_terrain_cpu.stub_run's dict.  dict(labels, smooth, tree_of, tops, res)."""
    r = t["res"]
    run = stub_run(cn, t["chm"], r.c, opts, r.e_min, r.n_min, cap)
    if run is None:
        return None
    run["tree_of"], run["tops"], run["res"] = stub_points(cn, t["norm"], t["hag"], opts, cap)
    return run


ARRAYS = ("labels", "smooth", "tops")


def same_run(a, b, arrays=ARRAYS):
    """Two runs hold the same bytes in every array and in the result."""
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in arrays) and result_bytes(a["res"]) == result_bytes(b["res"])


def show(run):
    return {f: getattr(run["res"], f) for f in RESULT_FIELDS}, run["tops"]


# ---------------------------------------------------------------- the transcription of rules 1-11
def py_refused(o, c, De, Dn):
    vals = [o.scale, o.min_height, o.win_a, o.win_b, o.r_min, o.r_max, o.crown_frac, o.max_crown_radius, o.ground_clear]
    if not all(math.isfinite(v) for v in vals) or not (math.isfinite(c) and c > 0):
        return True
    if not (o.scale > 0 and o.min_height > 0 and o.r_min > 0 and o.max_crown_radius > 0):
        return True
    if o.r_max < o.r_min or o.win_b < 0 or not 0 <= o.crown_frac <= 1 or o.ground_clear < 0:
        return True
    if not 0 <= o.smooth_passes <= 64 or not 1 <= o.max_trees <= 65536:
        return True
    return (o.r_max / o.scale) / c > 64 or De * Dn > 1 << 24


def py_smooth(Z, passes):
    """Rule 3 with numpy: the nine neighbours added in the rule's order, every sum an elementwise f64 operation."""
    H = np.array(Z, np.float32)
    dn, de = H.shape
    for _ in range(passes):
        P = np.full((dn + 2, de + 2), np.nan, np.float32)
        P[1:-1, 1:-1] = H
        S, W = np.zeros((dn, de)), np.zeros((dn, de))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = float((2 if dx == 0 else 1) * (2 if dy == 0 else 1))
                N = P[1 + dy:1 + dy + dn, 1 + dx:1 + dx + de]
                ok = ~np.isnan(N)
                S = np.where(ok, S + k * np.where(ok, N, 0).astype(np.float64), S)
                W = np.where(ok, W + k, W)
        with np.errstate(invalid="ignore", divide="ignore"):
            H = np.where(np.isnan(H), H, (S / W).astype(np.float32))
    return H


def py_run(Z, c, o, e_min=0.0, n_min=0.0):
    """(labels, smooth, tops, dict of the result's fields, intermediates) by rules 1-9 and 11, written from DESIGN.md f-21 with
    numpy and plain loops; None when the call is refused."""
    Z = np.asarray(Z, np.float32)
    dn, de = Z.shape
    if py_refused(o, c, de, dn):
        return None
    res = dict(c=c, e_min=np.float32(e_min), n_min=np.float32(n_min), De=de, Dn=dn, n_canopy=0, n_summits=0, n_trees=0, n_labelled_cells=0,
               n_labelled=0, max_depth=0, flags=NO_CANOPY, pad=0)
    H = py_smooth(Z, o.smooth_passes)
    labels = np.full((dn, de), -1, np.int32)
    tops = np.zeros(0, TOP_DTYPE)
    h = H.reshape(-1)
    with np.errstate(invalid="ignore"):
        canopy = np.isfinite(h) & (h.astype(np.float64) >= o.min_height / o.scale)
    res["n_canopy"] = int(canopy.sum())
    if res["n_canopy"] == 0:
        return labels, H, tops, res, {}
    res["flags"] = 0

    def key(q):                                                            # rule 5
        return (h[q], -q)

    def disc(q, R2):
        x, y, rad = q % de, q // de, math.isqrt(R2)
        return [yy * de + xx for yy in range(max(y - rad, 0), min(y + rad, dn - 1) + 1) for xx in range(max(x - rad, 0), min(x + rad, de - 1) + 1)
                if (xx - x) ** 2 + (yy - y) ** 2 <= R2 and canopy[yy * de + xx]]

    cells = [int(q) for q in np.flatnonzero(canopy)]
    up = {q: max(disc(q, 2), key=key) for q in cells}                      # rule 6: the 8 neighbours are the disc of R2 = 2
    root = {}
    for q in cells:
        path = [q]
        while up[path[-1]] != path[-1] and path[-1] not in root:
            path.append(up[path[-1]])
        r = root.get(path[-1], path[-1])
        for v in path:
            root[v] = r
    summits = [q for q in cells if up[q] == q]
    res["n_summits"] = len(summits)
    R2, parent = {}, {}
    for s in summits:                                                      # rule 7
        r = min(o.r_max, max(o.r_min, o.win_a + o.win_b * (float(h[s]) * o.scale)))
        rc = (r / o.scale) / c
        R2[s] = max(2, int(math.floor(rc * rc)))
        parent[s] = root[max(disc(s, R2[s]), key=key)]
    top, depth = {}, {}
    for s in summits:
        t, d = s, 0
        while parent[t] != t:
            t, d = parent[t], d + 1
        top[s], depth[s] = t, d
    res["max_depth"] = max(depth.values())
    all_tops = [s for s in summits if parent[s] == s]                       # rule 8 (ascending cell id: `cells` is)
    res["n_trees"] = len(all_tops)
    if len(all_tops) > o.max_trees:
        res["flags"] |= OVERFLOW
    number = {t: j for j, t in enumerate(all_tops[:o.max_trees])}
    mr = (o.max_crown_radius / o.scale) / c
    mr2 = math.floor(mr * mr)
    for q in cells:                                                        # rule 9
        t = top[root[q]]
        if t not in number:
            continue
        dx, dy = q % de - t % de, q // de - t // de
        if float(h[q]) >= o.crown_frac * float(h[t]) and float(dx * dx + dy * dy) <= mr2:
            labels[q // de, q % de] = number[t]
    res["n_labelled_cells"] = int((labels >= 0).sum())
    tops = np.zeros(len(number), TOP_DTYPE)
    for t, j in number.items():                                            # rule 11
        ix, iy, n_cells = t % de, t // de, int((labels == j).sum())
        tops[j] = (float(np.float32(e_min)) + (float(ix) + 0.5) * c, float(np.float32(n_min)) + (float(iy) + 0.5) * c, float(n_cells) * (c * c),
                   Z.reshape(-1)[t], h[t], t, ix, iy, R2[t], n_cells, 0)
    return labels, H, tops, res, dict(up=up, root=root, parent=parent, top=top, depth=depth, R2=R2, summits=summits)


def assert_transcribed(cn, Z, c, o, e_min=0.0, n_min=0.0):
    got, want = stub_run(cn, Z, c, o, e_min, n_min), py_run(Z, c, o, e_min, n_min)
    assert got is not None and want is not None
    assert got["labels"].tobytes() == want[0].tobytes() and got["smooth"].tobytes() == want[1].tobytes()
    assert {f: getattr(got["res"], f) for f in RESULT_FIELDS} == want[3], show(got)
    assert got["tops"].tobytes() == want[2].tobytes(), (got["tops"], want[2])
    return got, want[4]


def random_raster(seed, dn, de, holes=0.1, levels=None):
    """Heights 0 .. 12 (with `levels`: that many distinct values only, so that keys tie) with NaN holes."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(0, 12, (dn, de))
    if levels:
        Z = np.floor(Z / 12 * levels) * (12 / levels)
    Z = Z.astype(np.float32)
    Z[rng.uniform(size=Z.shape) < holes] = NAN
    return Z


def scene_raster(trees, seed, c):
    xyz, member = scene(seed, trees)
    Z, cell = max_raster(xyz, c)
    return xyz, member, Z, cell


def transcription_cases(cn):
    """name -> (Z, c, opts): the rasters the transcription and the device are compared on."""
    cases = {"random": (random_raster(1, 37, 41), 0.5, stub_opts(cn)),
             "ties": (random_raster(2, 40, 33, levels=6), 0.5, stub_opts(cn, smooth_passes=0)),
             "ties_smooth": (random_raster(3, 29, 52, holes=0.3, levels=4), 0.25, stub_opts(cn, smooth_passes=1, r_max=3.0)),
             "scale": (random_raster(4, 30, 30) / np.float32(0.37), 0.5 / 0.37, stub_opts(cn, scale=0.37, max_trees=7)),
             "plateau": (np.full((23, 31), 7.0, np.float32), 0.5, stub_opts(cn, smooth_passes=0)),
             "wide": (random_raster(5, 50, 50, holes=0.02), 0.5, stub_opts(cn, r_min=4.0, win_b=0.3, r_max=12.0, crown_frac=0.6, max_crown_radius=3.0))}
    for name, trees in (("apart", APART), ("touching", TOUCHING)):
        cases[name] = (scene_raster(trees, 1, 0.5)[2], 0.5, stub_opts(cn))
    cases["apart_025"] = (scene_raster(APART, 2, 0.25)[2], 0.25, stub_opts(cn, smooth_passes=1))
    return cases


@pytest.fixture(scope="module")
def cases(cn):
    return transcription_cases(cn)


def test_struct_sizes_and_defaults(cn):
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    cn.crn_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(CrownsOpts), TOP_DTYPE.itemsize, C.sizeof(CrownsResult)) == (80, 56, 56)
    o = stub_opts(cn)
    assert (o.scale, o.min_height, o.smooth_passes, o.win_a, o.win_b, o.r_min, o.r_max) == (1.0, 2.0, 2, 0.6, 0.06, 0.6, 5.0)
    assert (o.crown_frac, o.max_crown_radius, o.ground_clear, o.max_trees) == (0.3, 10.0, 0.3, 4096)
    assert cn.crn_tile() == TILE and cn.crn_batch() == BATCH


@pytest.mark.parametrize("name", ["random", "ties", "ties_smooth", "scale", "plateau", "wide", "apart", "touching", "apart_025"])
def test_transcription_gives_the_same_bytes(cn, cases, name):
    Z, c, o = cases[name]
    got, mid = assert_transcribed(cn, Z, c, o, e_min=-3.25, n_min=7.5)
    assert got["res"].n_trees >= 1 and got["res"].n_summits >= got["res"].n_trees
    if name == "scale":
        assert got["res"].flags == OVERFLOW and len(got["tops"]) == 7


# ---------------------------------------------------------------- scipy cross-checks
BINOMIAL = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float64)


def scipy_smooth(Z):
    mask = ~np.isnan(Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = ndimage.convolve(np.where(mask, Z, 0).astype(np.float64), BINOMIAL, mode="constant") / \
            ndimage.convolve(mask.astype(np.float64), BINOMIAL, mode="constant")
    return np.where(mask, out, np.nan).astype(np.float32)


@pytest.mark.parametrize("holes", [0.0, 0.25])
def test_smoothing_against_scipy_convolve(cn, holes):
    """One pass equals convolve(Z mask) / convolve(mask) under the binomial kernel within 1 float32 ulp (the two routes add the
    nine products in different orders); on small integers every f64 sum is exact in any order, and the bits are the same."""
    o = stub_opts(cn, smooth_passes=1)
    Z = random_raster(11, 45, 38, holes=holes)
    got, want = stub_run(cn, Z, 0.5, o)["smooth"], scipy_smooth(Z)
    ok = ~np.isnan(Z)
    assert (np.isnan(got) == ~ok).all() and (np.abs(got[ok] - want[ok]) <= np.spacing(np.abs(want[ok]))).all()
    Zi = np.where(ok, np.floor(Z), NAN).astype(np.float32)
    assert stub_run(cn, Zi, 0.5, o)["smooth"].tobytes() == scipy_smooth(Zi).tobytes()


@pytest.mark.parametrize("r", [0.6, 1.5, 3.2])
def test_tops_against_scipy_maximum_filter(cn, r):
    """With r_min = r_max every cell has the same window; without ties the tops are the canopy cells that equal the maximum
    filter over the window's disc."""
    rng = np.random.default_rng(12)
    Z = rng.uniform(0, 12, (60, 47)).astype(np.float32)
    assert len(np.unique(Z)) == Z.size
    c = 0.5
    run = stub_run(cn, Z, c, stub_opts(cn, smooth_passes=0, r_min=r, r_max=r))
    R2 = max(2, int(math.floor((r / c) ** 2)))
    rad = math.isqrt(R2)
    yy, xx = np.mgrid[-rad:rad + 1, -rad:rad + 1]
    want = (Z == ndimage.maximum_filter(Z, footprint=xx * xx + yy * yy <= R2, mode="constant", cval=-np.inf)) & (Z >= 2.0)
    assert sorted(run["tops"]["cell_id"]) == list(np.flatnonzero(want)) and (run["tops"]["R2"] == R2).all() and run["res"].n_trees > 3


# ---------------------------------------------------------------- rule cases built by hand
def row(*h):
    return np.array([h], np.float32)


def flat_opts(cn, r, **kw):
    """Unit cells, no smoothing, the window r cells for every summit, every canopy cell a crown cell."""
    base = dict(smooth_passes=0, r_min=float(r), r_max=float(r), win_a=0.0, win_b=0.0, crown_frac=0.0, max_crown_radius=1e4)
    base.update(kw)
    return stub_opts(cn, **base)


def test_plateau_has_its_lowest_id_for_its_one_summit(cn):
    """On an all-equal plateau rule 5 sends every cell to its neighbour of lowest id, so the walk of rule 6 ends in cell 0: one
    summit, the lowest id, and one top whatever the window; two plateaus give a top each, the lower id first."""
    got, mid = assert_transcribed(cn, np.full((9, 14), 5.0, np.float32), 1.0, flat_opts(cn, 2))
    assert (got["res"].n_summits, got["res"].n_trees) == (1, 1) and got["tops"]["cell_id"][0] == 0 and (got["labels"] == 0).all()
    Z = np.full((9, 14), 5.0, np.float32)
    Z[:, 6:8] = NAN
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 2))
    assert list(got["tops"]["cell_id"]) == [0, 8] and (got["labels"][:, :6] == 0).all() and (got["labels"][:, 8:] == 1).all()
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 8))              # the second plateau's summit sees the first: equal H, lower id
    assert list(got["tops"]["cell_id"]) == [0] and got["res"].n_summits == 2 and got["res"].max_depth == 1 and (got["labels"][~np.isnan(Z)] == 0).all()


def test_key_tie_is_broken_by_id(cn):
    got, _ = assert_transcribed(cn, row(3, 9, 3, 3, 9, 3), 1.0, flat_opts(cn, 3))
    assert got["res"].n_summits == 2 and list(got["tops"]["cell_id"]) == [1] and (got["labels"] == 0).all()
    got, _ = assert_transcribed(cn, row(3, 9, 3, 3, 9, 3), 1.0, flat_opts(cn, 2))   # out of each other's window: two tops
    assert list(got["tops"]["cell_id"]) == [1, 4] and list(got["labels"][0]) == [0, 0, 0, 1, 1, 1]


def test_window_over_the_edge_and_a_top_in_each_corner(cn):
    Z = np.full((12, 15), 3.0, np.float32)
    Z[0, 0], Z[0, -1], Z[-1, 0], Z[-1, -1] = 9, 8, 7, 6
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 5))
    corners = [0, 14, 11 * 15, 12 * 15 - 1]
    assert sorted(got["tops"]["cell_id"]) == corners and (got["tops"]["R2"] == 25).all()
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 14))             # the last corner sees the second, the second the first
    assert sorted(got["tops"]["cell_id"]) == [0] and got["res"].n_summits == 4 and got["res"].max_depth == 2
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 40, max_crown_radius=5.0))
    assert list(got["tops"]["cell_id"]) == [0] and got["res"].n_labelled_cells == int(sum(x * x + y * y <= 25 for x in range(15) for y in range(12)))


def test_minor_summit_goes_to_the_root_of_the_flank_cell_it_sees(cn):
    """The window of the minor summit (x = 10) holds x = 6, a cell of the tall tree's flank, and not the tall top (x = 2): its
    parent is that cell's root, the tall top, not the cell."""
    Z = row(12, 16, 20, 16, 12, 9, 7, 5, 3, 4, 6, 4, 3)
    got, mid = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 4))
    assert mid["summits"] == [2, 10] and mid["parent"][10] == 2 and mid["root"][6] == 2
    assert (got["res"].n_summits, got["res"].n_trees, got["res"].max_depth) == (2, 1, 1) and (got["labels"] == 0).all()
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 3))              # the window ends at x = 7, lower than the summit: a top
    assert list(got["tops"]["cell_id"]) == [2, 10] and list(got["labels"][0]) == [0] * 9 + [1] * 4


def staircase(m):
    """m summits three cells apart, each lower than the next: with windows of three cells each one's parent is the next."""
    Z = np.full((1, 3 * m), 3.0, np.float32)
    Z[0, ::3] = 5.0 + np.arange(m)
    return Z


def test_parent_chain_of_depth_three_and_more(cn):
    for m in (4, 9):
        got, mid = assert_transcribed(cn, staircase(m), 1.0, flat_opts(cn, 3))
        assert (got["res"].n_summits, got["res"].n_trees, got["res"].max_depth) == (m, 1, m - 1)
        assert got["tops"]["cell_id"][0] == 3 * (m - 1) and (got["labels"] == 0).all() and mid["depth"][0] == m - 1


def test_crown_frac_and_max_crown_radius_each_cut_a_cell(cn):
    Z = row(3, 4, 5, 10, 6, 5, 4)
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 2))
    assert list(got["labels"][0]) == [0] * 7
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 2, crown_frac=0.4))          # 4 >= 0.4 * 10 stays, 3 goes
    assert list(got["labels"][0]) == [-1, 0, 0, 0, 0, 0, 0]
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 2, max_crown_radius=2.0))    # two cells from the top
    assert list(got["labels"][0]) == [-1, 0, 0, 0, 0, 0, -1] and got["tops"]["cells"][0] == 5 and got["tops"]["area"][0] == 5.0
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 2, min_height=4.5))          # the cells below are not canopy at all
    assert list(got["labels"][0]) == [-1, -1, 0, 0, 0, 0, -1] and got["res"].n_canopy == 4


def test_max_trees_overflow(cn):
    Z = row(9, 3, 3, 8, 3, 3, 7, 3, 3, 6)
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 1, max_trees=2))
    assert got["res"].n_trees == 4 and got["res"].flags == OVERFLOW and list(got["tops"]["cell_id"]) == [0, 3]
    assert list(got["labels"][0]) == [0, 0, 1, 1, 1, -1, -1, -1, -1, -1]
    assert len(stub_run(cn, Z, 1.0, flat_opts(cn, 1), cap=3)["tops"]) == 3            # cap rows written, n_trees is all of them
    got, _ = assert_transcribed(cn, Z, 1.0, flat_opts(cn, 1, max_trees=4))
    assert got["res"].flags == 0 and len(got["tops"]) == 4


NANF = float("nan")
REFUSALS = [dict(scale=0.0), dict(scale=-1.0), dict(scale=NANF), dict(min_height=0.0), dict(min_height=float("inf")), dict(win_a=NANF),
            dict(win_b=-0.01), dict(win_b=float("inf")), dict(r_min=0.0), dict(r_min=2.0, r_max=1.0), dict(r_max=NANF), dict(crown_frac=-0.1),
            dict(crown_frac=1.1), dict(crown_frac=NANF), dict(max_crown_radius=0.0), dict(max_crown_radius=float("inf")),
            dict(ground_clear=-0.1), dict(ground_clear=NANF), dict(smooth_passes=-1), dict(smooth_passes=65), dict(max_trees=0),
            dict(max_trees=65537)]


@pytest.mark.parametrize("kw", REFUSALS)
def test_refusals_of_rule_1(cn, kw):
    Z = row(3, 9, 3)
    assert stub_run(cn, Z, 1.0, stub_opts(cn, **kw)) is None and py_run(Z, 1.0, stub_opts(cn, **kw)) is None


def test_cell_and_window_cap_and_raster_cap(cn):
    Z = row(3, 9, 3)
    for c in (0.0, -1.0, NANF, float("inf")):
        assert stub_run(cn, Z, c, stub_opts(cn)) is None
    assert stub_run(cn, Z, 0.5, stub_opts(cn, r_max=32.0)) is not None and stub_run(cn, Z, 0.5, stub_opts(cn, r_max=32.1)) is None
    assert stub_run(cn, Z, 0.5, stub_opts(cn, r_max=16.0, scale=0.5)) is not None and stub_run(cn, Z, 0.5, stub_opts(cn, r_max=16.1, scale=0.5)) is None
    got, _ = assert_transcribed(cn, np.full((70, 70), 5.0, np.float32), 0.5, stub_opts(cn, r_min=32.0, r_max=32.0, smooth_passes=0))
    assert got["tops"]["R2"][0] == 4096
    o, res = stub_opts(cn), CrownsResult()
    assert cn.crn_run(None, 4097, 4096, 1.0, 0.0, 0.0, C.byref(o), None, None, 0, None, C.byref(res)) == 1   # > 2^24 cells


def test_empty_raster_and_no_canopy(cn):
    for shape in ((0, 0), (0, 5), (4, 0)):
        run = stub_run(cn, np.zeros(shape, np.float32), 0.5)
        assert run["res"].flags == NO_CANOPY and (run["res"].Dn, run["res"].De) == shape and len(run["tops"]) == 0
    for Z in (np.full((5, 6), NAN), np.full((5, 6), 1.9, np.float32)):
        got, _ = assert_transcribed(cn, Z, 0.5, stub_opts(cn))
        assert got["res"].flags == NO_CANOPY and (got["labels"] == -1).all() and got["res"].n_canopy == 0
    got, _ = assert_transcribed(cn, np.full((1, 1), 2.0, np.float32), 0.5, stub_opts(cn))
    assert got["res"].n_trees == 1 and got["labels"][0, 0] == 0 and got["tops"]["area"][0] == 0.25


# ---------------------------------------------------------------- the planted scenes
def tree_points(cn, xyz, opts):
    """Rule 10 on a scene whose raster is tests/crown_scenes.max_raster's: the frame is the cloud's own, hag = z."""
    return stub_points(cn, xyz, xyz[:, 2], opts)


def tops_per_disc(tops, trees):
    e, n = tops["e"], tops["n"]
    return [int(((e - cx) ** 2 + (n - cy) ** 2 <= rad * rad).sum()) for cx, cy, ht, rad in trees]


def delineate_scene(cn, trees, seed, c, **kw):
    xyz, member, Z, cell = scene_raster(trees, seed, c)
    o = stub_opts(cn, **kw)
    run = stub_run(cn, Z, c, o, e_min=-14.0, n_min=-14.0)
    tree_of, tops, res = tree_points(cn, xyz, o)
    assert (tree_of == np.where(xyz[:, 2] >= 0.3, run["labels"].reshape(-1)[cell], -1)).all() and res.n_labelled == (tree_of >= 0).sum()
    assert (tops["points"] == np.bincount(tree_of[tree_of >= 0], minlength=len(tops))).all()
    return xyz, member, run, tree_of, tops, res


@pytest.mark.parametrize("c", [0.5, 0.25])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_apart_six_trees_one_top_per_disc_and_no_point_mislabelled(cn, c, seed):
    """Conditions of the scene, not measurements: the gaps between APART's crowns exceed every window, so the ascent cannot
    cross.  The unlabelled share (rule 9 prunes crown edges; DESIGN.md f-21 records it) is printed."""
    xyz, member, run, tree_of, tops, res = delineate_scene(cn, APART, seed, c)
    assert res.n_trees == 6 and res.flags == 0 and tops_per_disc(tops, APART) == [1] * 6
    order = [int(np.argmin((tops["e"] - cx) ** 2 + (tops["n"] - cy) ** 2)) for cx, cy, ht, rad in APART]
    assert sorted(order) == list(range(6))
    crown = (member >= 0) & (xyz[:, 2] >= 0.3)
    planted = np.array(order)[member[crown]]
    assert ((tree_of[crown] == planted) | (tree_of[crown] == -1)).all() and (tree_of[member < 0] == -1).all()
    for k, (cx, cy, ht, rad) in enumerate(APART):
        assert abs(tops["height"][order[k]] - ht) < 0.2
    print(f"APART seed {seed} cell {c}: unlabelled share of the crown points {(tree_of[crown] == -1).mean():.4%}")


@pytest.mark.parametrize("c", [0.5, 0.25, 0.1])
def test_touching_five_trees_one_top_per_disc(cn, c):
    """One top in every planted disc, five trees; the mislabelled share against the planted membership is measured (DESIGN.md f-21
    records it), not asserted against a number."""
    xyz, member, run, tree_of, tops, res = delineate_scene(cn, TOUCHING, 1, c, smooth_passes=0 if c == 0.1 else 2)
    assert res.n_trees == 5 and len(tops) == 5
    order = [int(np.argmin((tops["e"] - cx) ** 2 + (tops["n"] - cy) ** 2)) for cx, cy, ht, rad in TOUCHING]
    assert sorted(order) == list(range(5))
    for k, (cx, cy, ht, rad) in enumerate(TOUCHING):
        assert (tops["e"][order[k]] - cx) ** 2 + (tops["n"][order[k]] - cy) ** 2 <= rad * rad
    crown = (member >= 0) & (tree_of >= 0)
    wrong = (tree_of[crown] != np.array(order)[member[crown]]).mean()
    print(f"TOUCHING cell {c}: mislabelled share {wrong:.4%}, summits {res.n_summits}, depth {res.max_depth}")


def test_apart_at_a_tenth_of_a_metre_without_smoothing(cn):
    xyz, member, run, tree_of, tops, res = delineate_scene(cn, APART, 1, 0.1, smooth_passes=0)
    assert res.n_trees == 6 and res.n_summits > 50 and res.max_depth >= 2
    print(f"APART cell 0.1: summits {res.n_summits} of {res.n_canopy} canopy cells, depth {res.max_depth}")


def test_crowns_without_stems(cn, tn, gn, tr):
    """The capability: APART has crown and ground points only.  The chain of the stubs (ground plane, terrain, crowns) gives its
    six trees; the stem route on the same normalised cloud reports flag bit 1, no stem."""
    xyz, member = scene(1, APART)
    g = ground_run(gn, xyz, opts=ground_opts(gn, inlier_tol=0.5))
    assert g.flags == 0
    o = terrain_opts(tn)
    assert tn.ter_opts_from_ground(C.byref(g), C.byref(o)) == 0
    t = terrain_run(tn, xyz, opts=o)
    run = stub_cloud_run(cn, t, stub_opts(cn))
    assert run["res"].n_trees == 6 and len(run["tops"]) == 6 and run["res"].flags == 0
    tree_of = run["tree_of"]
    assert (tree_of[member < 0] == -1).all() and (tree_of[member >= 0] >= 0).mean() > 0.98
    for k in range(6):
        assert len(np.unique(tree_of[(member == k) & (tree_of >= 0)])) == 1
    stems = trees_run(tr, t["norm"], opts=trees_opts(tr, ground=0.0))
    assert stems[2].n_trees == 0 and stems[2].flags & 2
