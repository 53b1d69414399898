"""The launch plan of the blocked Cholesky of the reduced camera system (csrc/ba_chol_plan.h), on the CPU: the shape of a
launch, the decode of its trailing tiles, the dense route's schedule (X in diagonal blocks, deferred trailing updates, the
catch-up launch, tiles per workgroup), the separator's grid and the packing of a set of chains.  The plan alone drives a numpy
factorisation -- the panel step of every launch, then exactly the tiles and pending pairs `decode` names, in a shuffled order --
whose L, y = L^-1 g and X = L^-T must equal numpy's.  Replaces Eigen's LLT behind ceres::Solve(DENSE_SCHUR), reference
src/BundleAdjustment.cpp:116,123; chol_step2 / chol_step2_chains in csrc/ba.hip take the same counts from the same header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256          # the MI355X
BS = 2              # the numpy tile: the plan is in tile units, the kernel's 32 means nothing to it
TILE_S, TILE_RHS, TILE_X = 0, 1, 2
# numpy against itself at condition 1e3 in f64 agrees to ~1e-13; 1e-10 leaves room for the different summation order only
RTOL = 1e-10


def build_stub(dirname):
    """The stub over the header, built with g++ (no HIP); the GPU tests take the dense schedule's length from it too."""
    so = os.path.join(str(dirname), "libc2plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "stub", "chol_plan_capi.cpp")])
    lib = C.CDLL(so)
    lib.c2plan_constants.argtypes = [C.c_void_p]
    lib.c2plan_shape.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.c2plan_decode.argtypes = [C.c_int] * 8 + [C.c_void_p]
    lib.c2plan_dense_schedule.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.c2plan_dense_xb.argtypes = [C.c_int]
    lib.c2plan_launch_grid.argtypes = [C.c_int] * 4 + [C.c_void_p]
    lib.c2plan_pack_chains.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    return lib


@pytest.fixture(scope="module")
def c2(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("c2plan"))


def constants(c2):
    v = np.zeros(8, np.int32)
    c2.c2plan_constants(v.ctypes.data)
    return dict(zip(("CB", "C2_WAVES", "MAX_CHAINS", "DENSE_XB", "DENSE_XB_MIN_NT", "DENSE_DEFER4_MIN_NT", "DENSE_SWITCH_M2",
                     "DENSE_TPW8_ROUNDS"), (int(x) for x in v)))


def shape(c2, nt, nxc, k2, xb, dfr):
    v = np.zeros(7, np.int32)
    c2.c2plan_shape(nt, nxc, k2, xb, dfr, v.ctypes.data)
    return dict(zip(("m2", "npanel", "xlo", "nx", "ntile", "mx", "total"), (int(x) for x in v)))


def decode(c2, nt, nxc, k2, xb, dfr, catchup, total):
    """(kind, rb, cb, pair0, npend) of every trailing tile of the launch."""
    v = np.zeros((max(total, 1), 5), np.int32)
    c2.c2plan_decode(nt, nxc, k2, xb, dfr, catchup, 0, total, v.ctypes.data)
    return v[:total]


def dense_schedule(c2, nt, n_cu=N_CU):
    v = np.zeros((nt // 2 + 1, 6), np.int32)
    n = c2.c2plan_dense_schedule(nt, n_cu, v.ctypes.data, len(v))
    assert n <= len(v)
    return [dict(zip(("k2", "xb", "dfr", "catchup", "tpw", "grid"), (int(x) for x in row))) for row in v[:n]]


def launch_grid(c2, nt, nxc, k2, n_cu=N_CU):
    v = np.zeros(2, np.int32)
    c2.c2plan_launch_grid(nt, nxc, k2, n_cu, v.ctypes.data)
    return int(v[0]), int(v[1])


def pack_chains(c2, nts, nxcs, k2, n_cu, max_chains):
    a, b = np.asarray(nts, np.int32), np.asarray(nxcs, np.int32)
    h, ch = np.zeros(3, np.int32), np.zeros(max_chains, np.int32)
    pan0, trl0 = np.zeros(max_chains + 1, np.int32), np.zeros(max_chains + 1, np.int32)
    c2.c2plan_pack_chains(len(a), a.ctypes.data, b.ctypes.data, k2, n_cu, h.ctypes.data, ch.ctypes.data, pan0.ctypes.data,
                          trl0.ctypes.data)
    n = int(h[0])
    return dict(n=n, tpw=int(h[1]), total=int(h[2]), chain=ch[:n].tolist(), pan0=pan0[:n + 1].tolist(), trl0=trl0[:n + 1].tolist())


# ---------------------------------------------------------------------------------------------- the numpy factorisation
def spd(n, seed):
    """Random SPD matrix of condition ~1e3, a right-hand side."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    S = (q * np.logspace(0, 3, n)) @ q.T
    return 0.5 * (S + S.T), rng.standard_normal(n)


def factor_by_plan(c2, S, g, nt, nxc, launches, consts, seed=0):
    """Runs the launches on the lower triangle of S, g and the identity; returns (M, y, X) -- M's lower triangle holds L in
    the columns the launches factored and what is left of S right of them.  Asserts the structure of every launch on the way."""
    rng = np.random.default_rng(seed)
    n = nt * BS
    M, y, X = np.tril(S), g.copy(), np.eye(n)
    # folds[rb, cb, p]: how often pair p was subtracted from tile (rb, cb) of S (row nt: the rhs row)
    folds = np.zeros((nt + 1, nt, max(nt // 2, 1)), np.int8)
    sl = lambda b0, b1: slice(b0 * BS, b1 * BS)
    for L in launches:
        k2, xb, dfr, catchup = L["k2"], L["xb"], L["dfr"], L["catchup"]
        sh = shape(c2, nt, nxc, k2, xb, dfr)
        a = 2 * k2
        assert sh["m2"] == nt - a - 2 and sh["npanel"] == sh["m2"] + 2 and sh["xlo"] == (a // xb * xb if xb else 0)
        assert sh["nx"] == a + 2 - sh["xlo"]
        assert 4 <= L["tpw"] <= consts["C2_WAVES"]
        assert L["grid"] == sh["npanel"] + sh["nx"] + -(-sh["total"] // L["tpw"])
        P, xr = sl(a, a + 2), sl(sh["xlo"], a + 2)
        # ---- the panel step: the pending pair into the two panel columns, then factor and solve
        if k2 > 0:
            Q = sl(a - 2, a)
            M[a * BS:, P] -= M[a * BS:, Q] @ M[P, Q].T
            y[P] -= y[Q] @ M[P, Q].T
            X[xr, P] -= X[xr, Q] @ M[P, Q].T
            folds[a:, a:a + 2, k2 - 1] += 1
        # (every pair before the panels' own, once, in every tile of the two columns at and below the diagonal, and the rhs)
        for cb in (a, a + 1):
            assert np.all(folds[cb:, cb, :k2] == 1) and not folds[cb:, cb, k2:].any(), (nt, k2, cb)
        D = np.tril(M[P, P])        # (the folds of a diagonal tile leave something above the diagonal: never read)
        Lpp = np.linalg.cholesky(D + np.tril(D, -1).T)
        inv_t = np.linalg.inv(Lpp).T
        M[P, P] = Lpp
        M[(a + 2) * BS:, P] = M[(a + 2) * BS:, P] @ inv_t
        y[P] = y[P] @ inv_t
        X[xr, P] = X[xr, P] @ inv_t
        # ---- the trailing tiles: what decode names, no more; in any order
        tiles = decode(c2, nt, nxc, k2, xb, dfr, catchup, sh["total"])
        assert len({(int(t[0]), int(t[1]), int(t[2])) for t in tiles}) == sh["total"]
        n_kind = np.bincount(tiles[:, 0], minlength=3) if len(tiles) else np.zeros(3, int)
        assert (n_kind[TILE_S], n_kind[TILE_RHS], n_kind[TILE_X]) == (
            (sh["ntile"], sh["m2"], (a - sh["xlo"]) * sh["mx"]) if k2 else (0, 0, 0))
        for kind, rb, cb, pair0, npend in tiles[rng.permutation(len(tiles))]:
            # only pairs that earlier launches finished, up to the last of them; only columns right of the panels
            assert npend >= 1 and pair0 >= 0 and pair0 + npend == k2 and a + 2 <= cb < nt
            Q, c = sl(2 * pair0, 2 * (pair0 + npend)), sl(cb, cb + 1)
            if kind == TILE_S:
                assert cb <= rb < nt
                M[sl(rb, rb + 1), c] -= M[sl(rb, rb + 1), Q] @ M[c, Q].T
                folds[rb, cb, pair0:pair0 + npend] += 1
            elif kind == TILE_RHS:
                assert rb == nt
                y[c] -= y[Q] @ M[c, Q].T
                folds[nt, cb, pair0:pair0 + npend] += 1
            else:
                assert kind == TILE_X and sh["xlo"] <= rb < a and cb < min(nxc, sh["xlo"] + xb if xb else nxc)
                X[sl(rb, rb + 1), c] -= X[sl(rb, rb + 1), Q] @ M[c, Q].T
    return np.tril(M), y, X


def close(a, b):
    return np.abs(a - b).max() <= RTOL * np.abs(b).max()


# every even size to 60; the thresholds (X in blocks from 48, visits of four pairs from 100) from both sides; the GPU tests' two
# large shapes.  From 100 on the switch at DENSE_SWITCH_M2 = 40 tile rows falls inside every run.
DENSE_NT = sorted(set(range(2, 61, 2)) | {46, 48, 50, 98, 100, 102, 106, 264})


@pytest.mark.parametrize("nt", DENSE_NT)
def test_dense_schedule_drives_a_numpy_factorisation(c2, nt):
    consts = constants(c2)
    sched = dense_schedule(c2, nt)
    assert [L["k2"] for L in sched] == list(range(nt // 2))
    xb = c2.c2plan_dense_xb(nt)
    assert all(L["xb"] == xb for L in sched)
    S, g = spd(nt * BS, seed=nt)
    M, y, X = factor_by_plan(c2, S, g, nt, nt, sched, consts, seed=nt)
    Lr = np.linalg.cholesky(S)
    assert close(M, Lr)
    assert close(y, np.linalg.solve(Lr, g))
    Xr = np.linalg.inv(Lr).T
    if xb == 0:
        assert close(X, Xr)
    else:
        for b0 in range(0, nt, xb):
            blk = slice(b0 * BS, min(nt, b0 + xb) * BS)
            assert close(X[blk, blk], Xr[blk, blk]), (nt, b0)


def test_dense_schedule_at_its_thresholds(c2):
    """What the schedule's constants say, from both sides of each."""
    k = constants(c2)
    assert (k["DENSE_XB"], k["DENSE_XB_MIN_NT"], k["DENSE_DEFER4_MIN_NT"], k["DENSE_SWITCH_M2"], k["DENSE_TPW8_ROUNDS"]) == (8, 48, 100, 40, 4)
    assert (k["CB"], k["C2_WAVES"], k["MAX_CHAINS"]) == (32, 11, 8)
    # below 48 tile columns: all of X, nothing deferred
    for nt in (2, 46):
        assert all((L["xb"], L["dfr"], L["catchup"]) == (0, 1, 0) for L in dense_schedule(c2, nt))
    # 48 .. 98: X in blocks of 8, visits of two pairs as long as there is a column to visit, no launch that catches any up
    for nt in (48, 50, 98):
        sched = dense_schedule(c2, nt)
        assert all((L["xb"], L["dfr"], L["catchup"]) == (8, 2, 0) for L in sched[:-1])
        assert (sched[-1]["xb"], sched[-1]["dfr"]) == (8, 1) and shape(c2, nt, nt, nt // 2 - 1, 8, 1)["ntile"] == 0
    # from 100: visits of four pairs (four tiles a workgroup, eight where that makes more than four rounds) while more than 40 tile
    # rows are left, ONE catch-up launch, the rest undeferred
    for nt in (100, 102, 106, 264):
        sched = dense_schedule(c2, nt)
        for L in sched:
            m2 = nt - 2 * L["k2"] - 2
            assert L["dfr"] == (4 if m2 > 40 else 1)
            if L["dfr"] == 4:
                total = shape(c2, nt, nt, L["k2"], 8, 4)["total"]
                assert L["tpw"] == (8 if -(-total // 4) > 4 * N_CU else 4)
        first = next(i for i, L in enumerate(sched) if L["dfr"] == 1)
        assert [L["catchup"] for L in sched] == [4 if i == first else 0 for i in range(len(sched))]
        assert sched[first]["tpw"] == 4 and nt - 2 * sched[first]["k2"] - 2 == 40
    assert any(L["tpw"] == 8 for L in dense_schedule(c2, 264)) and not any(L["tpw"] == 8 for L in dense_schedule(c2, 106))
    # a small device: more tiles per workgroup, never more than a workgroup has waves
    assert max(L["tpw"] for L in dense_schedule(c2, 46, n_cu=64)) == k["C2_WAVES"]


@pytest.mark.parametrize("nt,nxc", [(2, 2), (12, 12), (38, 38), (14, 6), (30, 8), (44, 36)])
def test_one_matrix_and_a_chain_by_launch_grid(c2, nt, nxc):
    """The separator (nxc = nt) and one chain on its own (interior nxc < nt: nxc / 2 launches, X only over the interior): what is
    left right of the interior is the Schur complement that nd_combine sums onto the separator."""
    consts = constants(c2)
    launches = []
    for k2 in range(nxc // 2):
        tpw, grid = launch_grid(c2, nt, nxc, k2)
        launches.append(dict(k2=k2, xb=0, dfr=1, catchup=0, tpw=tpw, grid=grid))
    S, g = spd(nt * BS, seed=100 + nt)
    M, y, X = factor_by_plan(c2, S, g, nt, nxc, launches, consts, seed=nt)
    o = nxc * BS
    L11 = np.linalg.cholesky(S[:o, :o])
    assert close(M[:o, :o], L11)
    assert close(y[:o], np.linalg.solve(L11, g[:o]))
    assert close(X[:o, :o], np.linalg.inv(L11).T)
    if nxc < nt:
        W = np.linalg.solve(L11, S[:o, o:]).T
        assert close(M[o:, :o], W)
        # (the last launch's panels are still pending right of the interior: nd_combine folds them as it sums)
        Q = slice(o - 2 * BS, o)
        assert close(np.tril(M[o:, o:] - M[o:, Q] @ M[o:, Q].T), np.tril(S[o:, o:] - W @ W.T))
        assert close(y[o:] - M[o:, Q] @ y[Q], g[o:] - W @ y[:o])


def locate(blk, n, pan0, trl0):
    """The head of chol_step2_chains: the chain of a workgroup and its index within the chain's launch."""
    c = 0
    if blk < pan0[n]:
        while c + 1 < n and blk >= pan0[c + 1]:
            c += 1
        return c, blk - pan0[c]
    t = blk - pan0[n]
    while c + 1 < n and t >= trl0[c + 1]:
        c += 1
    return c, pan0[c + 1] - pan0[c] + (t - trl0[c])


@pytest.mark.parametrize("nis,NS,n_cu", [((4, 10, 6), 6, 256), ((12, 2, 8, 20), 4, 256), ((30, 26, 34, 28, 32, 30), 10, 256),
                                         ((16, 18, 12, 14, 20), 8, 64), ((40, 44, 42), 12, 256), ((6, 8, 4), 2, 8)])
def test_pack_chains_covers_every_workgroup_once(c2, nis, NS, n_cu):
    consts = constants(c2)
    nts = [ni + NS for ni in nis]
    dead_seen = False
    for k2 in range(max(nis) // 2):
        pk = pack_chains(c2, nts, nis, k2, n_cu, consts["MAX_CHAINS"])
        live = [i for i, ni in enumerate(nis) if 2 * k2 < ni]      # (a chain that has run out of panels is not in the launch)
        dead_seen |= len(live) < len(nis)
        assert pk["chain"] == live and pk["n"] == len(live)
        assert 4 <= pk["tpw"] <= consts["C2_WAVES"] and pk["pan0"][0] == 0 and pk["trl0"][0] == 0
        assert pk["total"] == pk["pan0"][-1] + pk["trl0"][-1]

        def wgs(tpw):
            out = []
            for i in live:
                sh = shape(c2, nts[i], nis[i], k2, 0, 1)
                out.append((sh["npanel"] + sh["nx"], -(-sh["total"] // tpw)))
            return out
        want = wgs(pk["tpw"])
        # the fewest tiles per workgroup, from four, that fit one round of workgroups
        assert pk["total"] <= n_cu or pk["tpw"] == consts["C2_WAVES"]
        if pk["tpw"] > 4:
            assert sum(p + t for p, t in wgs(pk["tpw"] - 1)) > n_cu
        hit = [locate(blk, pk["n"], pk["pan0"], pk["trl0"]) for blk in range(pk["total"])]
        assert len(set(hit)) == len(hit)
        assert set(hit) == {(j, bid) for j, (p, t) in enumerate(want) for bid in range(p + t)}
        # (panel workgroups first: a chain's panel workgroups are bid < npanel + nx, and lie in the first pan0[n] of the grid)
        assert all((bid < want[j][0]) == (blk < pk["pan0"][-1]) for blk, (j, bid) in enumerate(hit))
    assert dead_seen
