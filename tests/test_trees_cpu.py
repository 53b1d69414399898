"""Individual-tree extraction (csrc/trees.h, DESIGN.md f-13: the stems of a plot and every point's tree) on the CPU, through a
g++ build of the header the device code compiles (tests/stub/trees_capi.cpp): a literal Python transcription of rules 2-9
against the stub byte for byte; the graph rules against scipy (ndimage.label for the components, csgraph.dijkstra for the
labels); the rule cases built by hand; plots whose crowns are apart, where every point must get its own tree and the
dendrometry through the new labels must equal the dendrometry through the planted membership; plots whose crowns touch,
against the share recorded in DESIGN.md; and a 20-long pole that the sweeps must climb to the top.  No GPU."""
import ctypes as C
import heapq
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage, sparse
from scipy.sparse import csgraph

from sfm_danpipeline_amd.trees import STEM_DTYPE, TreesOpts, TreesResult, set_opts
from tests.test_dendro_cpu import dn, planted, py_frame, result_bytes as dendro_bytes, rotation, stub_opts as dendro_opts, stub_run as dendro_run  # noqa: F401
from tests.test_ground_cpu import TOL, disc, gn, stub_opts as ground_opts, stub_run as ground_run  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "trees_capi.cpp")
MAX_TREES = 4096
NONE_ABOVE, NO_STEM, TOO_MANY = 1, 2, 4
RESULT_FIELDS = [f for f, _ in TreesResult._fields_]
UNREACHED = (1 << 64) - 1
# the share of the tree points above the clearance that carry their planted tree on the two touching-crown scenes at voxel
# 0.15, measured on the stub (DESIGN.md f-13 records them); the tests assert them less 0.01
TOUCHING_SHARE = {"two": 0.9570, "four": 0.9003}


@pytest.fixture(scope="module")
def tr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("trees") / "libtreescapi.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    return load_stub(so)


def load_stub(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.trs_default_opts.argtypes = [vp]
    lib.trs_default_opts.restype = None
    lib.trs_sizes.argtypes = [vp, vp, vp]
    lib.trs_run.argtypes = [ci, vp, vp, C.c_int32, vp, ci, vp, ci, vp, vp]
    lib.trs_components.argtypes = [vp, ci, ci, ci, vp]
    lib.trs_components.restype = None
    lib.trs_steps.argtypes = [vp, vp]
    lib.trs_steps.restype = None
    lib.trs_opts_from_ground.argtypes = [vp, vp]
    return lib


# ---------------------------------------------------------------- wrappers (shared with tests/test_gpu_trees.py)
def stub_opts(tr, **kw):
    o = TreesOpts()
    tr.trs_default_opts(C.byref(o))
    return set_opts(o, **kw)


def result_bytes(r):
    return bytes(memoryview(r))


def stub_run(tr, xyz, labels=None, label=0, opts=None, threads=16, cap=MAX_TREES):
    """(tree_of, stems, TreesResult); None when the call is refused."""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32))
    tree_of, stems, res = np.full(max(len(xyz), 1), -1, np.int32), np.zeros(max(cap, 1), STEM_DTYPE), TreesResult()
    rc = tr.trs_run(len(xyz), xyz.ctypes.data, None if lab is None else lab.ctypes.data, label, C.byref(opts), threads, tree_of.ctypes.data,
                    cap, stems.ctypes.data, C.byref(res))
    return None if rc != 0 else (tree_of[:len(xyz)], stems[:min(cap, res.n_trees)].copy(), res)


def same_run(a, b):
    """Two (tree_of, stems, result) triples hold the same bytes."""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and result_bytes(a[2]) == result_bytes(b[2])


def show(run):
    return {f: getattr(run[2], f) for f in RESULT_FIELDS}, run[1]


# ---------------------------------------------------------------- planted plots
SQUARE5 = [(-2.5, -2.5), (2.5, -2.5), (-2.5, 2.5), (2.5, 2.5)]      # crowns (half axes 2 x 1.5) at least 1 apart
TWO_TOUCHING = [(-1.75, 0.0), (1.75, 0.0)]                          # 3.5 apart along x: the crowns overlap by 0.5
SQUARE3 = [(-1.5, -1.5), (1.5, -1.5), (-1.5, 1.5), (1.5, 1.5)]


def plot(seed, centres, n_tree=20000, n_ground=40000, radius=9.0, rot=None, scale=1.0):
    """Planted trees (tests/test_dendro_cpu.planted) at `centres` on a noisy ground disc, rotated by `rot` and divided by `scale`:
    (xyz float32, member: -1 ground, k tree k, R)."""
    rng = np.random.default_rng(3000 + seed)
    parts, member = [disc(rng, n_ground, radius)], [np.full(n_ground, -1, np.int32)]
    for k, (cx, cy) in enumerate(centres):
        t = planted(100 * seed + k, n_tree)[0].astype(np.float64)
        parts.append(t + np.array([cx, cy, 0.0]))
        member.append(np.full(len(t), k, np.int32))
    xyz, member = np.concatenate(parts), np.concatenate(member)
    R = np.eye(3) if rot is None else rotation(rot)
    xyz = (xyz @ R.T) / scale
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(np.float32), member[perm], R


def framed_opts(tr, gn, xyz, scale, **kw):
    """The options of a rotated plot: up, north and ground from the ground stub."""
    g = ground_run(gn, xyz, opts=ground_opts(gn, inlier_tol=TOL / scale))
    assert g.flags == 0
    o = stub_opts(tr, scale=scale, **kw)
    assert tr.trs_opts_from_ground(C.byref(g), C.byref(o)) == 0
    assert tuple(o.up) == tuple(g.up) and tuple(o.north) == tuple(g.north) and o.ground == g.offset * scale
    return o, g


def pole(n=4000, height=20.0, radius=0.1, seed=7):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, n)
    p = np.stack([radius * np.cos(a), radius * np.sin(a), rng.uniform(0, height, n)], 1)
    p[0] = (radius, 0.0, height - 1e-3)
    return p.astype(np.float32)


# ---------------------------------------------------------------- the transcription of rules 2-9
def py_frame_points(xyz, labels, label, o):
    """Rule 2: (frame float32 [n, 3], selected)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    E, Nn, U = py_frame(o)
    p = xyz.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fr = np.stack([((A[0] * p[:, 0] + A[1] * p[:, 1]) + A[2] * p[:, 2]).astype(np.float32) for A in (E, Nn, U)], 1)
    sel = np.isfinite(xyz).all(1) & np.isfinite(fr).all(1)
    if labels is not None:
        sel &= np.asarray(labels) == label
    return fr, sel


def py_classes(xyz, labels, label, o):
    """Rule 3: (frame, selected, above, band)."""
    fr, sel = py_frame_points(xyz, labels, label, o)
    h0, clear, lo, hi = o.ground / o.scale, o.ground_clear / o.scale, o.band_lo / o.scale, o.band_hi / o.scale
    with np.errstate(invalid="ignore"):
        d = fr[:, 2].astype(np.float64) - h0
        above = sel & (d >= clear)
        band = above & (d >= lo) & (d < hi)
    return fr, sel, above, band


def py_steps():
    """Rule 6: the 26 steps, dz slowest and dx fastest, and their weights."""
    steps = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    return steps, [{1: 10, 2: 14, 3: 17}[(dx != 0) + (dy != 0) + (dz != 0)] for dx, dy, dz in steps]


def py_run(xyz, labels, label, o, cap=MAX_TREES):
    """(tree_of, stems, dict of the result's fields, intermediates) by rules 2-9, written from DESIGN.md f-13 with numpy and plain
    loops; None when a grid cap refuses the call."""
    n = len(xyz)
    out = dict(n_selected=0, n_above=0, n_band=0, n_trees=0, n_voxels=0, n_labelled=0, max_cost=0, flags=NONE_ABOVE)
    tree_of, stems, mid = np.full(n, -1, np.int32), np.zeros(0, STEM_DTYPE), {}
    fr, sel, above, band = py_classes(xyz, labels, label, o)
    out.update(n_selected=int(sel.sum()), n_above=int(above.sum()), n_band=int(band.sum()))
    if not above.any():
        return tree_of, stems, out, mid
    out["flags"] = 0
    h0, c, w, v = o.ground / o.scale, o.stem_cell / o.scale, o.max_stem_width / o.scale, o.voxel / o.scale
    e, nn, h = (fr[:, a].astype(np.float64) for a in range(3))
    e_min, n_min = float(fr[above, 0].min()), float(fr[above, 1].min())
    e_max, n_max, h_max = float(fr[above, 0].max()), float(fr[above, 1].max()), float(fr[above, 2].max())
    # rule 4
    De, Dn = math.floor((e_max - e_min) / c) + 1, math.floor((n_max - n_min) / c) + 1
    if float(De) * float(Dn) > 2.0 ** 24:
        return None
    Dx, Dy, Dz = math.floor((e_max - e_min) / v) + 1, math.floor((n_max - n_min) / v) + 1, math.floor((h_max - h0) / v) + 1
    if float(Dx) * float(Dy) * float(Dz) >= 2.0 ** 31:
        return None
    A = np.nonzero(above)[0]
    ix, iy = np.floor((e[A] - e_min) / c).astype(np.int64), np.floor((nn[A] - n_min) / c).astype(np.int64)
    cell = iy * De + ix
    count = np.bincount(cell[band[A]], minlength=De * Dn)
    occupied = count >= o.min_cell_pts
    # rule 5: components by flood fill in ascending cell id, so that the first cell met is the least id
    root = np.full(De * Dn, -1, np.int64)
    for c0 in np.nonzero(occupied)[0]:
        if root[c0] >= 0:
            continue
        root[c0], stack = c0, [int(c0)]
        while stack:
            q = stack.pop()
            x, y = q % De, q // De
            for yy in range(max(y - 1, 0), min(y + 2, Dn)):
                for xx in range(max(x - 1, 0), min(x + 2, De)):
                    r = yy * De + xx
                    if occupied[r] and root[r] < 0:
                        root[r] = c0
                        stack.append(r)
    comp_ids = [int(r) for r in np.unique(root[root >= 0])]
    stem_of, rows, T_all = {}, [], 0
    for r in comp_ids:                                           # ascending component id
        cells = np.nonzero(root == r)[0]
        cx, cy, k = cells % De, cells // De, count[cells]
        N = int(k.sum())
        if N < o.min_stem_pts or float(cx.max() - cx.min() + 1) * c > w or float(cy.max() - cy.min() + 1) * c > w:
            continue
        if T_all < o.max_trees:
            Se, Sn = int((k * (2 * cx + 1)).sum()), int((k * (2 * cy + 1)).sum())
            ce, cn = e_min + (c * float(Se)) / float(2 * N), n_min + (c * float(Sn)) / float(2 * N)
            E, Nn, U = py_frame(o)
            foot = [(ce * E[a] + cn * Nn[a]) + h0 * U[a] for a in range(3)]
            stem_of[r] = T_all
            rows.append((ce, cn, foot, r, N, len(cells), 0))
        T_all += 1
    T = len(rows)
    if T_all > T:
        out["flags"] |= TOO_MANY
    out["n_trees"] = T
    mid.update(count=count.reshape(Dn, De), root=root.reshape(Dn, De), stem_of=stem_of)
    if T == 0:
        out["flags"] |= NO_STEM
        return tree_of, stems, out, mid
    # rule 6
    vx, vy, vz = (np.floor((e[A] - e_min) / v).astype(np.int64), np.floor((nn[A] - n_min) / v).astype(np.int64),
                  np.floor((h[A] - h0) / v).astype(np.int64))
    vkey = (vz * Dy + vy) * Dx + vx
    keys, pvox = np.unique(vkey, return_inverse=True)
    nv = len(keys)
    out["n_voxels"] = nv
    index = {int(k): i for i, k in enumerate(keys)}
    # rule 7
    key = [UNREACHED] * nv
    for i in np.nonzero(band[A])[0]:
        r = int(root[cell[i]])
        if r >= 0 and r in stem_of:
            key[pvox[i]] = min(key[pvox[i]], stem_of[r])
    mid.update(keys=keys, dims=(Dx, Dy, Dz), seeds=list(key), pvox=pvox, A=A)
    # rule 8: the fixed point of key(v) = min(key(v), key(u) + w), reached in ascending key order
    steps, weights = py_steps()
    heap = [(k, i) for i, k in enumerate(key) if k != UNREACHED]
    heapq.heapify(heap)
    while heap:
        k, i = heapq.heappop(heap)
        if k != key[i]:
            continue
        q = int(keys[i])
        x, y, z = q % Dx, (q // Dx) % Dy, q // (Dx * Dy)
        for (dx, dy, dz), wt in zip(steps, weights):
            xx, yy, zz = x + dx, y + dy, z + dz
            if xx < 0 or yy < 0 or zz < 0 or xx >= Dx or yy >= Dy or zz >= Dz:
                continue
            u = index.get((zz * Dy + yy) * Dx + xx)
            if u is not None and k + (wt << 16) < key[u]:
                key[u] = k + (wt << 16)
                heapq.heappush(heap, (key[u], u))
    # rule 9
    capc = math.floor(10.0 * (o.max_path / o.scale) / v) if o.max_path > 0 else None
    vtree = np.array([-1 if k == UNREACHED or (capc is not None and (k >> 16) > capc) else k & 0xFFFF for k in key], np.int32)
    tree_of[A] = vtree[pvox]
    labelled = vtree >= 0
    out["n_labelled"] = int((tree_of >= 0).sum())
    out["max_cost"] = max([k >> 16 for k, ok in zip(key, labelled) if ok], default=0)
    stems = np.zeros(min(cap, T), STEM_DTYPE)
    for s in range(len(stems)):
        ce, cn, foot, r, N, ncells, _ = rows[s]
        stems[s] = (ce, cn, foot, r, N, ncells, int((tree_of == s).sum()))
    mid.update(cost=np.array([k >> 16 if k != UNREACHED else -1 for k in key], np.int64))
    return tree_of, stems, out, mid


def assert_transcribed(tr, xyz, labels, label, o, cap=MAX_TREES):
    got = stub_run(tr, xyz, labels, label, o, cap=cap)
    want = py_run(xyz, labels, label, o, cap)
    assert got is not None and want is not None
    assert {f: getattr(got[2], f) for f in RESULT_FIELDS} == want[2]
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
    return got, want[3]


def small_plot(seed, **kw):
    return plot(seed, SQUARE5, n_tree=3000, n_ground=6000, **kw)


def transcription_cases(tr, gn):
    """name -> (xyz, labels, label, opts): the scenes the transcription and the device are compared on."""
    cases = {}
    xyz, member, _ = small_plot(1)
    cases["upright"] = (xyz, None, 0, stub_opts(tr, ground=0.0))
    for name, seed, scale in (("rot_037", 2, 0.37), ("rot_25", 3, 2.5)):
        x, _, _ = small_plot(seed, rot=seed, scale=scale)
        cases[name] = (x, None, 0, framed_opts(tr, gn, x, scale)[0])
    lab = np.where(member == 3, 5, 2).astype(np.int32)           # the fourth tree carries another label
    cases["labels"] = (xyz, lab, 2, stub_opts(tr, ground=0.0))
    bad = xyz.copy()
    bad[::97, 1] = np.nan
    bad[5::211, 0] = np.inf
    cases["nan"] = (bad, None, 0, stub_opts(tr, ground=0.0))
    return cases


@pytest.fixture(scope="module")
def cases(tr, gn):
    return transcription_cases(tr, gn)


def test_struct_sizes_and_defaults(tr):
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    tr.trs_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(TreesOpts), STEM_DTYPE.itemsize, C.sizeof(TreesResult))
    o = stub_opts(tr)
    assert math.isnan(o.ground) and (o.ground_clear, o.band_lo, o.band_hi, o.stem_cell, o.max_stem_width, o.voxel, o.max_path) == \
        (0.3, 1.0, 1.6, 0.05, 1.5, 0.15, 0.0) and (o.min_cell_pts, o.min_stem_pts, o.max_trees, o.scale) == (2, 30, 4096, 1.0)
    d, wts = np.zeros((26, 3), np.int32), np.zeros(26, np.int32)
    tr.trs_steps(d.ctypes.data, wts.ctypes.data)
    steps, weights = py_steps()
    assert [tuple(r) for r in d] == steps and list(wts) == weights and sorted(set(weights)) == [10, 14, 17]


@pytest.mark.parametrize("name", ["upright", "rot_037", "rot_25", "labels", "nan"])
def test_transcription_gives_the_same_bytes(tr, cases, name):
    xyz, lab, label, o = cases[name]
    got, _ = assert_transcribed(tr, xyz, lab, label, o)
    assert got[2].flags == 0 and got[2].n_trees == (3 if name == "labels" else 4)
    if name == "upright":
        assert_transcribed(tr, xyz, lab, label, o, cap=2)        # the first two rows only


def test_components_and_labels_against_scipy(tr, cases):
    """Rule 5 against ndimage.label with a 3 x 3 structure, rule 8 against per-stem csgraph.dijkstra on the weighted voxel graph."""
    xyz, lab, label, _ = cases["upright"]
    rng = np.random.default_rng(5)                                       # clutter in the band: many small components, each a stem
    clutter = np.stack([rng.uniform(-5, 5, 60), rng.uniform(-5, 5, 60), rng.uniform(0.9, 1.7, 60)], 1).astype(np.float32)
    xyz = np.concatenate([xyz, clutter])
    o = stub_opts(tr, ground=0.0, min_cell_pts=1, min_stem_pts=1, max_stem_width=0.5)
    got, mid = assert_transcribed(tr, xyz, lab, label, o)
    count = np.ascontiguousarray(mid["count"], np.int32)
    Dn, De = count.shape
    root = np.zeros((Dn, De), np.int32)
    tr.trs_components(count.ctypes.data, De, Dn, o.min_cell_pts, root.ctypes.data)
    lbl, m = ndimage.label(count >= o.min_cell_pts, structure=np.ones((3, 3)))
    assert m > 40 and got[2].n_trees > 40
    least = ndimage.minimum(np.arange(De * Dn).reshape(Dn, De), lbl, np.arange(1, m + 1)).astype(np.int64)
    assert np.array_equal(root, np.where(lbl > 0, least[np.maximum(lbl, 1) - 1], -1))
    # the weighted graph over the occupied voxels
    keys, (Dx, Dy, Dz) = mid["keys"], mid["dims"]
    nv = len(keys)
    x, y, z = keys % Dx, (keys // Dx) % Dy, keys // (Dx * Dy)
    rows, cols, wts = [], [], []
    for (dx, dy, dz), wt in zip(*py_steps()):
        xx, yy, zz = x + dx, y + dy, z + dz
        ok = (xx >= 0) & (yy >= 0) & (zz >= 0) & (xx < Dx) & (yy < Dy) & (zz < Dz)
        nk = (zz * Dy + yy) * Dx + xx
        pos = np.searchsorted(keys, nk)
        ok &= (pos < nv) & (keys[np.minimum(pos, nv - 1)] == nk)
        rows.append(np.nonzero(ok)[0]), cols.append(pos[ok]), wts.append(np.full(int(ok.sum()), wt))
    G = sparse.csr_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(nv, nv))
    seeds = np.array(mid["seeds"], np.float64)
    T = got[2].n_trees
    dist = np.stack([csgraph.dijkstra(G, directed=False, indices=np.nonzero(seeds == s)[0], min_only=True) for s in range(T)])
    vtree = np.where(np.isfinite(dist.min(0)), np.argmin(dist, 0), -1)          # argmin: the lowest stem on a tie
    want = np.full(len(xyz), -1, np.int32)
    want[mid["A"]] = vtree[mid["pvox"]]
    assert np.array_equal(got[0], want)
    assert got[2].max_cost == int(dist.min(0)[np.isfinite(dist.min(0))].max())


# ---------------------------------------------------------------- rule cases by hand
def lattice_opts(tr, **kw):
    """Unit cells and voxels, the band 0 .. 1, no clearance, one point enough: a point at (x + 0.5, y + 0.5, z + 0.5) is voxel (x, y, z)."""
    base = dict(ground=0.0, ground_clear=0.0, band_lo=0.0, band_hi=1.0, stem_cell=1.0, voxel=1.0, max_stem_width=1.0, min_cell_pts=1,
                min_stem_pts=1)
    base.update(kw)
    return stub_opts(tr, **base)


def at(*voxels):
    return np.array(voxels, np.float32) + 0.5


TIE = at((0, 0, 0), (4, 0, 0), (0, 0, 1), (1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 0, 1))   # two stems, a bridge above the band
ISLAND = at((0, 0, 0), (0, 0, 1), (6, 0, 5))


def column(height):
    return at(*[(0, 0, z) for z in range(height)])


def test_a_voxel_equidistant_from_two_stems_goes_to_the_lower_number(tr):
    tree_of, stems, res = stub_run(tr, TIE, opts=lattice_opts(tr))
    assert res.n_trees == 2 and list(tree_of) == [0, 1, 0, 0, 0, 1, 1] and res.max_cost == 24 and list(stems["points"]) == [4, 3]
    assert list(stems["cell_id"]) == [0, 4] and list(stems["e"]) == [1.0, 5.0] and res.n_labelled == 7
    # mirrored, the middle voxel still goes to stem 0, which is now the other one
    tree_of, _, _ = stub_run(tr, TIE * np.array([-1, 1, 1], np.float32), opts=lattice_opts(tr))
    assert list(tree_of) == [1, 0, 1, 1, 0, 0, 0]


def test_an_island_no_seed_reaches_gets_none(tr):
    tree_of, stems, res = stub_run(tr, ISLAND, opts=lattice_opts(tr))
    assert list(tree_of) == [0, 0, -1] and res.n_voxels == 3 and res.n_labelled == 2 and res.n_above == 3 and res.flags == 0


def test_max_path_at_equality_and_one_over(tr):
    col = column(5)                                                              # costs 0, 10, 20, 30, 40
    assert list(stub_run(tr, col, opts=lattice_opts(tr, max_path=3.0))[0]) == [0, 0, 0, 0, -1]      # cap 30: cost 30 stays
    tree_of, _, res = stub_run(tr, col, opts=lattice_opts(tr, max_path=2.9))                        # cap 29: cost 30 is one over
    assert list(tree_of) == [0, 0, 0, -1, -1] and res.max_cost == 20 and res.n_labelled == 3
    assert stub_run(tr, col, opts=lattice_opts(tr))[2].max_cost == 40
    # the cap is in voxel steps of the scaled length: half the scale, twice the cloud units
    assert list(stub_run(tr, col, opts=lattice_opts(tr, max_path=1.5, scale=0.5, stem_cell=0.5, voxel=0.5, band_hi=0.5,
                                                    max_stem_width=0.5))[0]) == [0, 0, 0, 0, -1]


def test_cell_and_stem_thresholds_at_equality_and_one_past(tr):
    three = np.concatenate([at((0, 0, 0))] * 3 + [at((0, 0, 1))])
    assert stub_run(tr, three, opts=lattice_opts(tr, min_cell_pts=3))[2].n_trees == 1
    res = stub_run(tr, three, opts=lattice_opts(tr, min_cell_pts=4))[2]
    assert res.n_trees == 0 and res.flags == NO_STEM and res.n_band == 3 and res.n_voxels == 0
    assert stub_run(tr, three, opts=lattice_opts(tr, min_stem_pts=3))[2].n_trees == 1
    assert stub_run(tr, three, opts=lattice_opts(tr, min_stem_pts=4))[2].flags == NO_STEM
    wide = at((0, 0, 0), (1, 1, 0), (2, 0, 0))                                   # one component through a diagonal, 3 x 2 cells
    tree_of, stems, res = stub_run(tr, wide, opts=lattice_opts(tr, max_stem_width=3.0))
    assert res.n_trees == 1 and list(tree_of) == [0, 0, 0] and stems[0]["band_cells"] == 3 and stems[0]["band_points"] == 3
    assert (stems[0]["e"], stems[0]["n"]) == (0.5 + 1.5, 0.5 + 5.0 / 6.0) and tuple(stems[0]["foot"]) == (2.0, 0.5 + 5.0 / 6.0, 0.0)
    assert stub_run(tr, wide, opts=lattice_opts(tr, max_stem_width=2.9))[2].flags == NO_STEM
    assert stub_run(tr, wide[:, [1, 0, 2]], opts=lattice_opts(tr, max_stem_width=2.9))[2].flags == NO_STEM      # ... and along n


def test_flag_bits(tr):
    three = at((0, 0, 0), (3, 0, 0), (6, 0, 0), (6, 0, 1))
    tree_of, stems, res = stub_run(tr, three, opts=lattice_opts(tr, max_trees=2))
    assert res.flags == TOO_MANY and res.n_trees == 2 and len(stems) == 2 and list(tree_of) == [0, 1, -1, -1]
    assert stub_run(tr, three, opts=lattice_opts(tr, max_trees=3))[2].flags == 0
    tree_of, stems, res = stub_run(tr, three, opts=lattice_opts(tr, band_lo=2.0, band_hi=3.0))
    assert res.flags == NO_STEM and res.n_above == 4 and res.n_band == 0 and len(stems) == 0 and (tree_of == -1).all()
    tree_of, _, res = stub_run(tr, three, opts=lattice_opts(tr, ground=5.0))
    assert res.flags == NONE_ABOVE and res.n_selected == 4 and res.n_above == 0 and (tree_of == -1).all()
    assert stub_run(tr, np.zeros((0, 3), np.float32), opts=lattice_opts(tr))[2].flags == NONE_ABOVE
    assert stub_run(tr, three, np.zeros(4, np.int32), 1, lattice_opts(tr))[2].n_selected == 0


REFUSALS = [dict(ground=float("nan")), dict(ground=float("inf")), dict(ground_clear=-0.01), dict(band_lo=0.29), dict(band_hi=1.0),
            dict(stem_cell=0.0), dict(voxel=0.0), dict(voxel=float("nan")), dict(max_stem_width=0.0), dict(max_path=-1.0),
            dict(min_cell_pts=0), dict(min_stem_pts=0), dict(max_trees=0), dict(max_trees=4097), dict(up=(0, 0, 1.1)),
            dict(north=(0, 0, 1)), dict(scale=0.0)]


@pytest.mark.parametrize("kw", REFUSALS)
def test_refusals(tr, kw):
    base = dict(ground=0.0)
    base.update(kw)
    assert stub_run(tr, column(3), opts=stub_opts(tr, **base)) is None


def test_both_grid_caps(tr):
    far = at((0, 0, 0), (4096, 4095, 0))                                         # 4097 x 4096 cells: one row past 2^24
    assert stub_run(tr, far, opts=lattice_opts(tr)) is None and py_run(far, None, 0, lattice_opts(tr)) is None
    assert stub_run(tr, at((0, 0, 0), (4095, 4095, 0)), opts=lattice_opts(tr))[2].n_trees == 2       # 2^24 cells pass
    tall = at((0, 0, 0), (1023, 1023, 2047))                                     # 2^10 2^10 2^11 = 2^31 voxels
    assert stub_run(tr, tall, opts=lattice_opts(tr)) is None and py_run(tall, None, 0, lattice_opts(tr)) is None
    assert stub_run(tr, at((0, 0, 0), (1023, 1023, 2046)), opts=lattice_opts(tr))[2].n_voxels == 2


# ---------------------------------------------------------------- planted plots
def planted_share(xyz, member, centres, o, run):
    """(share of the tree points above the clearance that carry their planted tree, the run) with the stems matched to the
    planted centres by distance in the frame (upright plots)."""
    tree_of, stems, res = run
    assert res.n_trees == len(centres)
    owner = [int(np.argmin([(s["e"] - cx) ** 2 + (s["n"] - cy) ** 2 for cx, cy in centres])) for s in stems]
    assert sorted(owner) == list(range(len(centres)))
    _, _, above, _ = py_classes(xyz, None, 0, o)
    mine = above & (member >= 0)
    return float((np.array(owner)[np.maximum(tree_of[mine], 0)] == member[mine])[tree_of[mine] >= 0].sum()) / float(mine.sum())


def exact_plot(tr, gn, variant):
    """The four-trees-5-apart plot of a variant: (xyz, member, opts, ground result or None)."""
    rot, scale = {"upright": (None, 1.0), "rot": (11, 1.0), "rot_037": (12, 0.37), "rot_25": (13, 2.5)}[variant]
    xyz, member, _ = plot(20, SQUARE5, rot=rot, scale=scale)
    if rot is None:
        return xyz, member, stub_opts(tr, ground=0.0), None
    o, g = framed_opts(tr, gn, xyz, scale)
    return xyz, member, o, g


def assert_exact(xyz, member, o, run):
    """Every tree point at or above the clearance carries one number per planted tree, and no ground point any."""
    tree_of, stems, res = run
    assert res.flags == 0 and res.n_trees == 4
    _, _, above, _ = py_classes(xyz, None, 0, o)
    assert (tree_of[member < 0] == -1).all() and (tree_of[~above] == -1).all()
    stem_of_tree = []
    for k in range(4):
        got = np.unique(tree_of[above & (member == k)])
        assert len(got) == 1 and got[0] >= 0, (k, got)
        stem_of_tree.append(int(got[0]))
    assert sorted(stem_of_tree) == [0, 1, 2, 3] and res.n_labelled == int((above & (member >= 0)).sum())
    return stem_of_tree


@pytest.mark.parametrize("variant", ["upright", "rot", "rot_037", "rot_25"])
def test_separated_crowns_are_exact_and_so_is_the_dendrometry(tr, gn, dn, variant):
    xyz, member, o, g = exact_plot(tr, gn, variant)
    run = stub_run(tr, xyz, opts=o)
    stem_of_tree = assert_exact(xyz, member, o, run)
    if variant == "upright":
        for voxel in (0.2, 0.3):
            o2 = stub_opts(tr, ground=0.0, voxel=voxel)
            assert_exact(xyz, member, o2, stub_run(tr, xyz, opts=o2))
    # the dendrometry of each tree through the new labels against the planted membership masked by the clearance
    d = dendro_opts(dn, scale=o.scale, up=tuple(o.up), north=tuple(o.north), ground=o.ground)
    _, _, above, _ = py_classes(xyz, None, 0, o)
    masked = np.where(above, member, -1).astype(np.int32)
    for k in range(4):
        a, rows_a, _ = dendro_run(dn, xyz, run[0], stem_of_tree[k], d)
        b, rows_b, _ = dendro_run(dn, xyz, masked, k, d)
        assert dendro_bytes(a) == dendro_bytes(b) and rows_a.tobytes() == rows_b.tobytes() and a.flags == 0 and abs(a.dbh - 0.3) < 0.01


@pytest.mark.parametrize("name,centres", [("two", TWO_TOUCHING), ("four", SQUARE3)])
def test_touching_crowns(tr, name, centres):
    xyz, member, _ = plot(30, centres, n_tree=20000, n_ground=20000)
    o = stub_opts(tr, ground=0.0)
    share = planted_share(xyz, member, centres, o, stub_run(tr, xyz, opts=o))
    print("touching crowns, %s: share %.4f (recorded %.4f)" % (name, share, TOUCHING_SHARE[name]))
    assert share >= TOUCHING_SHARE[name] - 0.01


def test_the_sweeps_climb_a_20_long_pole(tr):
    p = pole()
    tree_of, stems, res = stub_run(tr, p, opts=stub_opts(tr, ground=0.0))
    up = p[:, 2].astype(np.float64) >= 0.3
    assert res.n_trees == 1 and (tree_of[up] == 0).all() and (tree_of[~up] == -1).all()
    assert abs(res.max_cost - 1234) <= 17 and res.n_voxels > 16 * 17             # more voxel levels than several batches of sweeps
    assert res.n_labelled == stems[0]["points"] == int(up.sum())
