"""The set-up of a bundle-adjustment problem (csrc/ba_setup.h), on the CPU: the observations grouped by point, the points
grouped by camera list into runs (run ids in order of first appearance, ascending points inside a run) -- checked against a
numpy restatement, on one thread and on several --, the runs cut into the elimination's pieces or sent to the pair path, and
the camera co-visibility graph.  One shape runs again under AddressSanitizer / UBSan, with the host pool's nested and
throwing passes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sfm_danpipeline_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stub", "ba_setup_capi.cpp")
N_CU = 256
SHORT_RUN = 12
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -3, -5


@pytest.fixture(scope="module")
def bs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bsetup") / "libbsetup.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-o", so, STUB])
    lib = C.CDLL(so)
    lib.bsetup_run.restype = C.c_void_p
    lib.bsetup_run.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.POINTER(C.c_int)]
    lib.bsetup_free.argtypes = [C.c_void_p]
    lib.bsetup_scalar.argtypes = [C.c_void_p, C.c_char_p]
    lib.bsetup_array.restype = C.c_void_p
    lib.bsetup_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.bsetup_pool_nested.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.bsetup_pool_throw.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


def ld_of(n_cam):
    return (6 * n_cam + 1 + 63) // 64 * 64


ARRAYS = {"order": np.int32, "optr": np.int32, "ocam": np.int32, "obs_src": np.int32, "cam_used": np.uint8,
          "chunks": (np.int32, 4), "sig_cams": np.int32, "bs_desc": np.int32, "adj": np.uint64, "fb": np.int32,
          "pp_obase": np.int32, "cptr": np.int32, "cpt": np.int32, "cxy_src": np.int32, "pair_cams": (np.int32, 2),
          **{f"ids{k}": np.int32 for k in range(8)}}


def run(bs, n_cam, n_pt, oc, op, xy, threads=0, short_pieces=512):
    oc, op = np.ascontiguousarray(oc, np.int32), np.ascontiguousarray(op, np.int32)
    xy = np.ascontiguousarray(xy, np.float64)
    st = C.c_int(0)
    h = bs.bsetup_run(n_cam, n_pt, len(oc), oc.ctypes.data, op.ctypes.data, xy.ctypes.data, ld_of(n_cam), N_CU, 1,
                      short_pieces, threads, C.byref(st))
    try:
        out = {"status": st.value}
        for k in ("np", "no", "cam_split", "grow_waves", "grow_accw", "elim_deterministic"):
            out[k] = bs.bsetup_scalar(h, k.encode())
        for k, t in ARRAYS.items():
            dt, w = t if isinstance(t, tuple) else (t, 1)
            n, eb = C.c_longlong(0), C.c_int(0)
            p = bs.bsetup_array(h, k.encode(), C.byref(n), C.byref(eb))
            assert eb.value == np.dtype(dt).itemsize * w, k     # (an empty array may have no data pointer)
            a = np.ctypeslib.as_array((C.c_ubyte * (n.value * eb.value)).from_address(p)) if n.value else np.zeros(0, np.uint8)
            out[k] = a.view(dt).reshape(-1, w).copy() if w > 1 else a.view(dt).copy()
        return out
    finally:
        bs.bsetup_free(h)


def restate(n_cam, n_pt, oc, op):
    """The grouping as the reference's containers define it: a point's observations by ascending camera (std::map, ties in
    input order), runs of equal camera lists numbered in order of their first point, ascending points inside a run."""
    src = np.lexsort((oc, op))                       # (stable: ties keep the input order)
    cnt = np.bincount(op, minlength=n_pt)
    start = np.concatenate([[0], np.cumsum(cnt)])
    sig = {}
    run_of = np.full(n_pt, -1)
    for p in np.flatnonzero(cnt):
        run_of[p] = sig.setdefault(tuple(oc[src[start[p]:start[p + 1]]]), len(sig))
    pts = np.flatnonzero(run_of >= 0)
    order = pts[np.lexsort((pts, run_of[pts]))]
    obs_src = np.concatenate([src[start[p]:start[p + 1]] for p in order]) if len(order) else np.zeros(0, int)
    optr = np.concatenate([[0], np.cumsum(cnt[order])])
    runs = list(sig)                                 # camera list of every run, by run id
    run_start = np.concatenate([[0], np.cumsum(np.bincount(run_of[pts], minlength=len(runs)))])
    return dict(order=order, optr=optr, obs_src=obs_src, ocam=oc[obs_src], runs=runs, run_start=run_start,
                cam_used=np.bincount(oc, minlength=n_cam) > 0)


def check_grouping(got, ref):
    assert got["status"] == OK
    assert got["np"] == len(ref["order"]) and got["no"] == len(ref["obs_src"])
    for k in ("order", "optr", "obs_src", "ocam"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(got["cam_used"].astype(bool), ref["cam_used"])


def check_pieces(got, ref, short_pieces=512):
    runs, rs = ref["runs"], ref["run_start"]
    np_ = got["np"]
    chunks = got["chunks"]                           # (sig_off, n, p0, cnt)
    # every grouped point is in exactly one chunk or on the pair path
    cover = np.zeros(np_ + 1, np.int64)
    for _, _, p0, c in chunks:
        cover[p0] += 1
        cover[p0 + c] -= 1
    cover = np.cumsum(cover)[:np_]
    cover[got["fb"]] += 1
    assert (cover == 1).all()
    assert (np.diff(got["fb"]) > 0).all()            # the pair path's points ascend
    # which runs are pieces: a strictly ascending list of <= 10 cameras, unless the run is short and short runs stay on the
    # pair path (they become pieces while nothing else needs that path and there are at most `short_pieces` of them)
    mfma = [len(s) <= 10 and all(a < b for a, b in zip(s, s[1:])) for s in runs]
    size = np.diff(rs)
    n_short = int(sum(1 for r in range(len(runs)) if mfma[r] and size[r] <= SHORT_RUN))
    short_as_pieces = all(mfma) and 0 < n_short <= short_pieces
    run_at = np.searchsorted(rs, chunks[:, 2], side="right") - 1
    for r in range(len(runs)):
        mine = chunks[run_at == r]
        if not mfma[r] or (size[r] <= SHORT_RUN and not short_as_pieces):
            assert len(mine) == 0
            continue
        # the pieces of a run tile it with no gap, and carry its camera list
        mine = mine[np.argsort(mine[:, 2])]
        assert mine[0, 2] == rs[r] and (mine[:-1, 2] + mine[:-1, 3] == mine[1:, 2]).all() and mine[-1, 2] + mine[-1, 3] == rs[r + 1]
        assert (mine[:, 3] > 0).all() and (mine[:, 1] == len(runs[r])).all()
        for so in mine[:, 0]:
            assert tuple(got["sig_cams"][so:so + len(runs[r])]) == runs[r]
    # every chunk in the list of its width, once; each list largest piece first
    listed = np.concatenate([got[f"ids{k}"] for k in range(8)])
    assert sorted(listed) == list(range(len(chunks)))
    for k in range(8):
        ids = got[f"ids{k}"]
        assert ((6 * chunks[ids, 1] + 2 + 15) // 16 == k + 1).all()
        assert (np.diff(chunks[ids, 3]) <= 0).all()
    # ba_backsub_runs' descriptors: every chunk, largest first
    desc = got["bs_desc"].reshape(-1, 16)
    assert len(desc) == len(chunks) and (np.diff(desc[:, 2]) <= 0).all()


def check_graph(got, ref, n_cam):
    """h_adj: the union of the runs' camera cliques, a symmetric bit matrix."""
    wpr = (n_cam + 63) // 64
    bits = got["adj"].reshape(n_cam, wpr)
    adj = ((bits[:, np.arange(n_cam) >> 6] >> (np.arange(n_cam) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    ref_adj = np.zeros((n_cam, n_cam), bool)
    for s in ref["runs"]:
        ref_adj[np.ix_(s, s)] = True
    assert (adj == adj.T).all()
    np.testing.assert_array_equal(adj, ref_adj)


def shapes():
    """The three shapes of a problem the set-up sees: one camera list per start camera (cfg3 / cfg4's), ragged lists of 2-10
    cameras in thousands of combinations (most of them short runs), the same observations in random order with every third
    point left without any."""
    rng = np.random.default_rng(12)
    pb = synth.ba_problem(60, 30000, 10, seed=19)
    oc, op, xy = pb["obs_cam"], pb["obs_pt"], pb["obs_xy"]
    keep = rng.random(len(oc)) < 0.6
    keep[0::10] = True
    keep[1::10] = True
    sel = np.flatnonzero(keep & (op % 3 != 0))
    rng.shuffle(sel)
    return {"ring": (oc, op, xy), "ragged": (oc[keep], op[keep], xy[keep]), "shuffled": (oc[sel], op[sel], xy[sel])}


SHAPES = shapes()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_setup_groups_and_cuts_as_the_restatement(bs, shape):
    oc, op, xy = SHAPES[shape]
    ref = restate(60, 30000, oc, op)
    one = run(bs, 60, 30000, oc, op, xy, threads=1)
    check_grouping(one, ref)
    check_pieces(one, ref)
    check_graph(one, ref, 60)
    # several threads (odd blocks, whatever the machine has): the same set-up, array for array
    many = run(bs, 60, 30000, oc, op, xy, threads=5)
    for k in one:
        np.testing.assert_array_equal(many[k], one[k], err_msg=k)


def test_short_runs_stay_on_the_pair_path_past_the_limit(bs):
    oc, op, xy = SHAPES["ring"]
    keep = np.ones(len(oc), bool)
    keep[[10 * 17 + 2, 10 * 900 + 0, 10 * 2499 + 5]] = False         # three points of one view less: three short runs
    oc, op, xy = oc[keep], op[keep], xy[keep]
    ref = restate(60, 30000, oc, op)
    for limit in (512, 0):
        got = run(bs, 60, 30000, oc, op, xy, short_pieces=limit)
        check_grouping(got, ref)
        check_pieces(got, ref, short_pieces=limit)
        assert (len(got["fb"]) == 0) == (limit > 0)


def test_setup_refuses_bad_observations(bs):
    oc = np.zeros(4097, np.int32)
    op = np.zeros(4097, np.int32)
    xy = np.zeros((4097, 2))
    assert run(bs, 1, 1, oc, op, xy)["status"] == ERR_UNSUPPORTED    # more than FB_MAXN observations of one point
    assert run(bs, 1, 1, oc[:4096], op[:4096], xy[:4096])["status"] == OK
    assert run(bs, 2, 1, np.array([0, 2]), np.array([0, 0]), xy[:2])["status"] == ERR_ARG
    assert run(bs, 2, 1, np.array([0, 1]), np.array([0, 1]), xy[:2])["status"] == ERR_ARG


def test_host_pool_nested_pass(bs):
    """A pass inside a pass of the pool (sfmhip_host_parallel_for's callback re-entering the library): the inner pass runs
    on threads of its own and every item is visited once."""
    hits = np.zeros(64 * 50, np.int32)
    bs.bsetup_pool_nested(64, 50, 4, hits.ctypes.data)
    assert (hits == 1).all()


def test_host_pool_exception_on_the_calling_thread(bs):
    """Thread 0 throws while the workers still run the job: the exception reaches the caller only once they are done, and
    the pool takes the next job."""
    done = np.zeros(40000, np.int32)
    assert bs.bsetup_pool_throw(40000, 4, done.ctypes.data) == 1
    assert (done[10000:] == 1).all() and (done[:10000] == 0).all()
    hits = np.zeros(64 * 50, np.int32)
    bs.bsetup_pool_nested(64, 50, 4, hits.ctypes.data)
    assert (hits == 1).all()


def test_setup_under_asan_ubsan(bs, tmp_path):
    exe = str(tmp_path / "bsetup_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DBSETUP_MAIN", "-o", exe, STUB])
    oc, op, xy = SHAPES["shuffled"]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([60, 30000, len(oc), ld_of(60), N_CU, 4], np.int32).tobytes())
        f.write(np.asarray(oc, np.int32).tobytes() + np.asarray(op, np.int32).tobytes() + np.asarray(xy, np.float64).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=600, env=env)
    bad = [m for m in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:") if m in r.stderr]
    assert r.returncode == 0 and not bad, r.stderr[-3000:]
    got = run(bs, 60, 30000, oc, op, xy, threads=4)
    assert r.stdout.splitlines()[0].split()[:6] == ["status", "0", "np", str(got["np"]), "no", str(got["no"])]
    assert r.stdout.splitlines()[1] == "pool nested+throw ok"
