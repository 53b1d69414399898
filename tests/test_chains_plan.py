"""The chains + separator plan of the reduced camera solve (csrc/ba_chains_plan.h), on the CPU: the cut it chooses, its index
maps, buffer offsets and gather job list; the maps alone drive a numpy chains + separator solve (factor the interiors, sum
their Schur complements onto the separator, solve, back-substitute) whose solution must equal a dense solve.  Replaces Eigen's
LLT behind ceres::Solve(DENSE_SCHUR), reference src/BundleAdjustment.cpp:116,123; the device kernels (nd_gather,
chol_step2_chains, nd_combine, nd_xy, nd_w in csrc/ba.hip) walk the same maps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_front_plan import band_adj, random_system, ring_adj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CP_MAX = 8
N_CU = 256          # the MI355X


@pytest.fixture(scope="module")
def cp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cplan") / "libcplan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "stub", "chains_plan_capi.cpp")])
    lib = C.CDLL(so)
    lib.cplan_build_flat.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_int]
    return lib


def dense_tiles_of(nc):
    """sfmhip_ba's ld / 32: 6 nc + 1 columns, padded to whole pairs of 32-column panels."""
    return (6 * nc + 1 + 63) // 64 * 2


def build(cp, adj, force, dense_tiles=None):
    nc = len(adj)
    wpr = (nc + 63) // 64
    bits = np.zeros((nc, wpr), np.uint64)
    for i in range(nc):
        for j in np.nonzero(adj[i])[0]:
            bits[i, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    header, cost = np.zeros(8, np.int32), np.zeros(1)
    cams, n_cams = np.zeros(nc, np.int32), np.zeros(CP_MAX + 1, np.int32)
    dims, offs, col0 = np.zeros(3 * (CP_MAX + 1), np.int32), np.zeros(3 * (CP_MAX + 1) + 1, np.int64), np.zeros(CP_MAX + 1, np.int32)
    inv, jobs = np.zeros(1 << 18, np.int32), np.zeros((1 << 18, 4), np.int32)
    rc = cp.cplan_build_flat(nc, bits.ctypes.data, wpr, dense_tiles_of(nc) if dense_tiles is None else dense_tiles, N_CU, int(force),
                             header.ctypes.data, cost.ctypes.data, cams.ctypes.data, n_cams.ctypes.data, dims.ctypes.data,
                             offs.ctypes.data, col0.ctypes.data, inv.ctypes.data, len(inv), jobs.ctypes.data, len(jobs))
    assert rc == 0
    if not header[0]:
        return None
    n = int(header[1])
    assert header[4] == n_cams[0]
    groups = np.split(cams[:n_cams[:n + 1].sum()], np.cumsum(n_cams[:n + 1])[:-1])
    dims = dims[:3 * (n + 1)].reshape(n + 1, 3)
    invs = np.split(inv[:header[7]], np.cumsum(32 * dims[:, 1])[:-1])
    return dict(n=n, NS=int(header[2]), max_ni=int(header[3]), violations=int(header[5]), cost=float(cost[0]), sep=groups[0],
                chains=groups[1:], ni=dims[:, 0], N=dims[:, 1], ld=dims[:, 2], offs=offs[:3 * (n + 1)].reshape(n + 1, 3),
                total=int(offs[3 * (n + 1)]), col0=col0[:n + 1], inv=invs, jobs=jobs[:header[6]].copy())


def check_structure(pl, adj):
    nc, n, NS = len(adj), pl["n"], pl["NS"]
    assert pl["violations"] == 0 and 2 <= n <= CP_MAX
    # separator and chains partition the cameras; no edge between two chains
    owner = np.full(nc, -2)
    owner[pl["sep"]] = -1
    for i, ch in enumerate(pl["chains"]):
        assert len(ch) and np.all(np.diff(ch) > 0) and np.all(owner[ch] == -2)
        owner[ch] = i
    assert np.all(owner > -2)
    a, c = np.nonzero(adj)
    assert not np.any((owner[a] >= 0) & (owner[c] >= 0) & (owner[a] != owner[c]))
    # the maps: every parameter once over the interiors and invS, the focal in invS, padding -1, every chain's tail is invS
    invS = pl["inv"][n]
    assert NS % 2 == 0 and pl["ni"][n] == pl["N"][n] == NS and len(invS) == 32 * NS
    assert np.array_equal(invS[:6 * len(pl["sep"])], (6 * pl["sep"][:, None] + np.arange(6)).ravel())
    assert invS[6 * len(pl["sep"])] == 6 * nc and np.all(invS[6 * len(pl["sep"]) + 1:] == -1)
    seen = np.zeros(6 * nc + 1, int)
    np.add.at(seen, invS[invS >= 0], 1)
    for i in range(n):
        ni, N, inv = int(pl["ni"][i]), int(pl["N"][i]), pl["inv"][i]
        assert ni % 2 == 0 and ni == (6 * len(pl["chains"][i]) + 63) // 64 * 2 and N == ni + NS and len(inv) == 32 * N
        own = inv[:32 * ni]
        assert np.array_equal(own[:6 * len(pl["chains"][i])], (6 * pl["chains"][i][:, None] + np.arange(6)).ravel())
        assert np.all(own[6 * len(pl["chains"][i]):] == -1)
        assert np.array_equal(inv[32 * ni:], invS)
        np.add.at(seen, own[own >= 0], 1)
    assert np.all(seen == 1)
    assert np.all(pl["ld"] == 32 * pl["N"]) and pl["max_ni"] == pl["ni"][:n].max()
    assert np.array_equal(pl["col0"], np.concatenate([[0], np.cumsum(32 * pl["ni"][:n])]))
    # M | X | y of every chain in turn: disjoint, and together the whole buffer
    at = 0
    for i in range(n + 1):
        ld = int(pl["ld"][i])
        assert tuple(pl["offs"][i]) == (at, at + ld * ld, at + 2 * ld * ld)
        at += 2 * ld * ld + ld
    assert at == pl["total"]
    # the gather's jobs, in the order the device takes them.  Per tile row tr of chain i: role 0 the tiles of M that come from S
    # (lower triangle, interior columns); role 1 the row of y and of X's diagonal; role 2 the lower right block of M (zero: the
    # factorisation reads it before it writes); role 3 the interior rows of X (the identity; a chain's X ends at its interior
    # columns); one role-4 job at the end (ba_finalize's part)
    want = []
    for i in range(n + 1):
        ni, N = int(pl["ni"][i]), int(pl["N"][i])
        for tr in range(N):
            want += [(i, tr, tc, 0) for tc in range(min(tr, ni - 1) + 1)]
            want.append((i, tr, 0, 1))
            want += [(i, tr, tc, 2) for tc in range(ni, tr + 1)]
            if tr < ni:
                want += [(i, tr, tc, 3) for tc in range(ni)]
    want.append((0, 0, 0, 4))
    assert [tuple(j) for j in pl["jobs"]] == want


def chains_solve(pl, S, g):
    """The solve the kernels do, from the maps alone: M_i = [D_i, . ; C_i, 0] gathered from S (padding: the identity),
    L_ii = chol(D_i), L_Si = C_i L_ii^-T, D_S' = D_S - sum_i L_Si L_Si^T, z_S = D_S'^-1 (g_S - sum_i L_Si y_i),
    z_i = L_ii^-T (y_i - L_Si^T z_S)."""
    def gather(inv):
        ok = inv >= 0
        M = np.eye(len(inv))
        M[np.ix_(ok, ok)] = S[np.ix_(inv[ok], inv[ok])]
        y = np.zeros(len(inv))
        y[ok] = g[inv[ok]]
        return M, y
    n = pl["n"]
    DS, yS = gather(pl["inv"][n])
    L, LS, Y = [], [], []
    for i in range(n):
        o = 32 * int(pl["ni"][i])
        M, y = gather(pl["inv"][i])
        Lii = np.linalg.cholesky(M[:o, :o])
        LSi = np.linalg.solve(Lii, M[o:, :o].T).T
        yi = np.linalg.solve(Lii, y[:o])
        DS -= LSi @ LSi.T
        yS -= LSi @ yi
        L.append(Lii), LS.append(LSi), Y.append(yi)
    zS = np.linalg.solve(DS, yS)
    z = np.full(len(g), np.nan)
    ok = pl["inv"][n] >= 0
    z[pl["inv"][n][ok]] = zS[ok]
    for i in range(n):
        zi = np.linalg.solve(L[i].T, Y[i] - LS[i].T @ zS)
        own = pl["inv"][i][:len(zi)]
        z[own[own >= 0]] = zi[own >= 0]
    return z


def two_rings(nc, k):
    adj = np.zeros((2 * nc, 2 * nc), bool)
    adj[:nc, :nc] = adj[nc:, nc:] = ring_adj(nc, k)
    return adj


GRAPHS = {"ring96": (lambda: ring_adj(96, 6), True), "ring200": (lambda: ring_adj(200, 10), False),
          "ring560": (lambda: ring_adj(560, 8), True), "band24": (lambda: band_adj(24, 3), True),
          "two_rings": (lambda: two_rings(40, 4), True), "two_small_rings": (lambda: two_rings(10, 4), True),
          "ring1100": (lambda: ring_adj(1100, 4), True)}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_plans_are_sound_and_solve_the_system(cp, name):
    make, force = GRAPHS[name]
    adj = make()
    pl = build(cp, adj, force)
    assert pl is not None
    check_structure(pl, adj)
    S, g = random_system(adj, len(adj))
    z = chains_solve(pl, S, g)
    zr = np.linalg.solve(S, g)
    assert np.abs(z - zr).max() <= 1e-10 * np.abs(zr).max()
    if name == "band24":            # chains shorter than one tile pair
        assert np.all(pl["ni"][:pl["n"]] == 2) and all(6 * len(c) < 64 for c in pl["chains"])
    if name == "two_rings":         # components without a cut (8 tiles each, the focal alone in a separator of 2) are a plan:
        assert pl["cost"] <= 0.5 * 8 + 0.5 * 2 + 2.5    # the one chosen (it cuts the rings further) costs no more
    if name == "two_small_rings":   # one tile pair each: no cut can win, the separator holds the focal alone
        assert len(pl["sep"]) == 0 and pl["NS"] == 2 and pl["n"] == 2 and [len(c) for c in pl["chains"]] == [10, 10]
        assert np.array_equal(pl["inv"][2], [6 * 20] + [-1] * 63)
    if name == "ring1100":          # the coarse grid, two cuts at the most: they cut a ring (ordered from one camera in both
        assert pl["n"] <= 4         # directions) into four arcs; a third cut would leave six


def test_a_complete_graph_has_no_cut(cp):
    adj = np.ones((40, 40), bool) & ~np.eye(40, dtype=bool)
    assert build(cp, adj, True) is None and build(cp, adj, False) is None


def test_the_layouts_the_gpu_tests_see(cp):
    """What tests/test_gpu_geometry.py asserts of sfmhip_ba_reduced_layout under SFMHIP_BA_ND=1, here without a GPU."""
    pl = build(cp, ring_adj(200, 10), True)             # test_reduced_layout_follows_the_camera_graph
    assert pl["n"] == 4 and pl["max_ni"] + pl["NS"] <= 16
    pl96 = build(cp, ring_adj(96, 6), True)             # test_dissected_reduced_system_walks_the_dense_iterates
    assert pl96["n"] >= 2 and pl96["max_ni"] + pl96["NS"] < dense_tiles_of(96) == 20
    # the layouts themselves: (chains, chain_tiles, separator_tiles) as the planner gave them while it was inline in ba.hip
    assert (pl["n"], pl["max_ni"], pl["NS"]) == (4, 8, 8) and (pl96["n"], pl96["max_ni"], pl96["NS"]) == (4, 4, 4)
    # unforced, cfg4's 38 dense tiles: the same plan, accepted (its cost 0.5 (max_ni + NS) + 2.5 against 0.8 * 19 launches)
    un = build(cp, ring_adj(200, 10), False, dense_tiles=38)
    assert un is not None and un["cost"] == 0.5 * (pl["max_ni"] + pl["NS"]) + 2.5 <= 0.8 * 19
    assert all(np.array_equal(a, b) for a, b in zip(un["inv"], pl["inv"])) and np.array_equal(un["jobs"], pl["jobs"])
    # and refused where it does not win by 20 %: only a forced plan is left
    assert build(cp, ring_adj(200, 10), False, dense_tiles=int(2 * un["cost"] / 0.8) - 1) is None
