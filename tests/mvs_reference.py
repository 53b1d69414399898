"""Shared by tests/test_mvs_reference_cpu.py and tests/test_gpu_mvs.py: an independent reference of the dense stereo
 and the scenes the kernel and the header's host build are compared on.  A plain module: numpy only, no
device code, nothing of csrc/mvs.h.

The reference is written from f-10's rule list.  Every window sum is the direct sum of (2w+1)^2 shifted slices in int64: no
separable sums, no tiles, no row bands.  Every f64 expression is a chain of numpy's elementwise ufuncs in the rule list's
order (numpy never contracts a multiply and an add), so the result is expected to equal the header's bit for bit.  The
winner is found plane by plane over a stored score volume, and its neighbours are looked up there afterwards.

The scenes: general poses ([R | t], x_cam = R X + t) through `rodrigues`, a renderer for them (`render_posed`), smooth
random textures, and one constructor per case of the table in tests/test_mvs_reference_cpu.py.  Everything random comes
from np.random.RandomState."""
import functools

import numpy as np

from tests.test_mvs_cpu import texture

OPTS = dict(n_planes=128, window=3, n_src=4, n_best=2, min_views=3, ncc_min=0.7, eps=0.01, var_min=614656.0)
ALL_PIXELS = dict(ncc_min=-1.0, var_min=0.0)   # every pixel with a full window that some source sees gets a winner
K_AWK = np.array([[100.0, 0, 23.3], [0, 96.0, 16.8], [0, 0, 1]])   # fx != fy, cx and cy no half-integers: H has no zero entry


def ref_opts(**kw):
    o = dict(OPTS)
    assert set(kw) <= set(o)
    o.update(kw)
    return o


def new_stats():
    """what ref_sample counts: positions sampled, samples that exist, of those the ones with a vertical weight, c <= 0"""
    return dict(positions=0, valid=0, wy=0, behind=0)


# ---------------------------------------------------------------- the reference
def ref_pyramid(img, level):
    """rule 1: [rows, cols] or [rows, cols, 3] uint8 halved `level` times, an odd last row / column dropped"""
    a = np.asarray(img).astype(np.int64)
    for _ in range(level):
        r, c = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
        a = (a[0:r:2, 0:c:2] + a[0:r:2, 1:c:2] + a[1:r:2, 0:c:2] + a[1:r:2, 1:c:2] + 2) >> 2
    return a.astype(np.uint8)


def ref_level_K(K, level):
    K = np.array(K, np.float64)
    for _ in range(level):
        K[0, 0], K[1, 1] = K[0, 0] * 0.5, K[1, 1] * 0.5
        K[0, 2], K[1, 2] = (K[0, 2] + 0.5) * 0.5 - 0.5, (K[1, 2] + 0.5) * 0.5 - 0.5
    return K


def ref_sample(img, H, x, y, view=None, stats=None):
    """rule 3 over arrays: the 12-bit sample of img [rows, cols] (or of img[view] for a stack) at H (x, y, 1), -1 where
    there is none.  H [..., 3, 3], x, y and view broadcast against each other."""
    img = np.asarray(img)
    rows, cols = img.shape[-2:]
    H = np.asarray(H, np.float64)
    h = [H[..., i // 3, i % 3] for i in range(9)]
    xd, yd = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        a = (h[0] * xd + h[1] * yd) + h[2]
        b = (h[3] * xd + h[4] * yd) + h[5]
        c = (h[6] * xd + h[7] * yd) + h[8]
        front = c > 0.0
        u, v = a / c, b / c
        ok = front & (u >= 0.0) & (v >= 0.0) & (u < float(cols)) & (v < float(rows))
        u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        fu, fv = np.floor(u), np.floor(v)
        wx, wy = np.floor((u - fu) * 32.0 + 0.5).astype(np.int64), np.floor((v - fv) * 32.0 + 0.5).astype(np.int64)
    ix, iy = fu.astype(np.int64) + (wx == 32), fv.astype(np.int64) + (wy == 32)
    wx, wy = np.where(wx == 32, 0, wx), np.where(wy == 32, 0, wy)
    ok &= (ix + 1 < cols) & (iy + 1 < rows)          # all four taps inside, also a tap of weight 0
    ix, iy = np.where(ok, ix, 0), np.where(ok, iy, 0)
    if rows < 2 or cols < 2:
        out = np.full(ok.shape, -1, np.int64)
    else:
        tap = (lambda dy, dx: img[iy + dy, ix + dx]) if view is None else (lambda dy, dx: img[view, iy + dy, ix + dx])
        i00, i01, i10, i11 = (tap(dy, dx).astype(np.int64) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
        s = ((i00 * (32 - wx) + i01 * wx) * (32 - wy) + (i10 * (32 - wx) + i11 * wx) * wy + 32) >> 6
        out = np.where(ok, s, -1)
    if stats is not None:
        stats["positions"] += int(ok.size)
        stats["valid"] += int(ok.sum())
        stats["wy"] += int((ok & (wy != 0)).sum())
        stats["behind"] += int((~np.broadcast_to(front, ok.shape)).sum())
    return out


def plane_range(dmin, dmax, D):
    inv_far = 1.0 / float(dmax)
    return inv_far, (1.0 / float(dmin) - inv_far) / float(D - 1)


def ref_homographies(K, poses, ref, src, D, dmin, dmax):
    """rule 2: H [D, len(src), 3, 3] = K (R_rel + t_rel e3^T inv_k) K^-1, the operations in csrc/mvs.h's order (asserted bit
    for bit against the stub's mvs_homographies)"""
    K, P = np.asarray(K, np.float64), np.asarray(poses, np.float64).reshape(-1, 3, 4)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    inv_far, step = plane_range(dmin, dmax, D)
    inv = inv_far + np.arange(D, dtype=np.float64) * step
    Pr = P[ref]
    out = np.zeros((D, len(src), 3, 3))
    for s, sv in enumerate(src):
        Ps = P[sv]
        R = [[(Ps[i, 0] * Pr[j, 0] + Ps[i, 1] * Pr[j, 1]) + Ps[i, 2] * Pr[j, 2] for j in range(3)] for i in range(3)]
        t = [Ps[i, 3] - ((R[i][0] * Pr[0, 3] + R[i][1] * Pr[1, 3]) + R[i][2] * Pr[2, 3]) for i in range(3)]
        M = [[np.full(D, R[i][0]), np.full(D, R[i][1]), R[i][2] + t[i] * inv] for i in range(3)]
        A = [[fx * M[0][j] + cx * M[2][j] for j in range(3)], [fy * M[1][j] + cy * M[2][j] for j in range(3)], M[2]]
        for i in range(3):
            h0, h1 = A[i][0] / fx, A[i][1] / fy
            out[:, s, i, 0], out[:, s, i, 1], out[:, s, i, 2] = h0, h1, (A[i][2] - h0 * cx) - h1 * cy
    return out


def ref_centres(poses):
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    return np.array([[-((p[0, a] * p[0, 3] + p[1, a] * p[1, 3]) + p[2, a] * p[2, 3]) for a in range(3)] for p in P])


def ref_sources(poses, ref, n_src):
    """rule 6: the n_src other views with the nearest camera centres, ties by lower index"""
    c = ref_centres(poses)
    d = [(float((dx * dx + dy * dy) + dz * dz), v) for v, (dx, dy, dz) in enumerate(c - c[ref]) if v != ref]
    return [v for _, v in sorted(d)[:n_src]]


def ref_depthmap(gray, H, ref, src, opts, dmin, dmax, stats=None, chunk=32):
    """rules 3-5 for one reference view: gray [n, rows, cols] uint8 at the working level, H [D, len(src), 3, 3];
    returns idx int32, depth f32, score f32, each [rows, cols]"""
    gray = np.asarray(gray)
    n, rows, cols = gray.shape
    D, w, nb = opts["n_planes"], opts["window"], opts["n_best"]
    W2, N, S = 2 * w + 1, (2 * w + 1) ** 2, len(src)
    idx, depth, score = np.full((rows, cols), -1, np.int32), np.zeros((rows, cols), np.float32), np.zeros((rows, cols), np.float32)
    hh, ww = rows - 2 * w, cols - 2 * w
    if hh <= 0 or ww <= 0:                            # no window fits the image
        return idx, depth, score

    def wsum(a):
        out = np.zeros(a.shape[:-2] + (hh, ww), np.int64)
        for dy in range(W2):
            for dx in range(W2):
                out += a[..., dy:dy + hh, dx:dx + ww]
        return out

    r = 16 * gray[ref].astype(np.int64)
    sr, srr = wsum(r), wsum(r * r)
    vr = N * srr - sr * sr
    rok = (vr > 0) & (vr.astype(np.float64) >= opts["var_min"])
    y, x = np.mgrid[0:rows, 0:cols]
    view = np.asarray(src, np.int64)[None, :, None, None]
    scores, oks = np.zeros((D, hh, ww)), np.zeros((D, hh, ww), bool)
    for k0 in range(0, D, chunk):
        q = ref_sample(gray, np.asarray(H)[k0:k0 + chunk, :, None, None], x, y, view=view, stats=stats)   # [c, S, rows, cols]
        bad = q < 0
        q = np.where(bad, 0, q)
        sq, sqq, srq, nbad = wsum(np.stack([q, q * q, r * q, bad.astype(np.int64)]))
        vq = N * sqq - sq * sq
        counts = rok & (nbad == 0) & (vq > 0)
        num = N * srq - sr * sq
        with np.errstate(all="ignore"):
            ncc = num.astype(np.float64) / np.sqrt(vr.astype(np.float64) * vq.astype(np.float64))
        best = -np.sort(-np.where(counts, ncc, -np.inf), axis=1)          # descending over the sources
        ok = rok & (counts.sum(1) >= nb)
        if nb <= S:
            a = best[:, 0]
            for i in range(1, nb):
                a = a + best[:, i]
            scores[k0:k0 + chunk] = np.where(ok, a, 0.0) / float(nb)
        oks[k0:k0 + chunk] = ok
    top, bk = np.zeros((hh, ww)), np.full((hh, ww), -1, np.int64)
    for k in range(D):                                # largest score, lowest index on ties
        better = oks[k] & ((bk < 0) | (scores[k] > top))
        top, bk = np.where(better, scores[k], top), np.where(better, k, bk)
    at = lambda vol, k: np.take_along_axis(vol, np.clip(k, 0, D - 1)[None], 0)[0]
    sm, sp = at(scores, bk - 1), at(scores, bk + 1)
    interior = (bk > 0) & (bk < D - 1) & at(oks, bk - 1) & at(oks, bk + 1)
    den = (sm - 2.0 * top) + sp
    with np.errstate(all="ignore"):
        off = np.where(interior & (den < 0.0), 0.5 * (sm - sp) / den, 0.0)
    off = np.clip(off, -0.5, 0.5)
    inv_far, step = plane_range(dmin, dmax, D)
    acc = (bk >= 0) & (top >= opts["ncc_min"])
    with np.errstate(all="ignore"):
        z = (1.0 / (inv_far + (bk.astype(np.float64) + off) * step)).astype(np.float32)
    idx[w:rows - w, w:cols - w] = np.where(acc, bk, -1)
    depth[w:rows - w, w:cols - w] = np.where(acc, z, np.float32(0))
    score[w:rows - w, w:cols - w] = np.where(acc, top.astype(np.float32), np.float32(0))
    return idx, depth, score


def ref_fuse(K, poses, depth, gray, bgr, eps, min_views):
    """rule 7: depth [n, rows, cols] f32 (anything not > 0: no depth), K of the working level; returns xyz f32 [m, 3],
    normals f32 [m, 3], rgb u32 [m] in view, row, column order"""
    depth = np.asarray(depth, np.float32)
    n, rows, cols = depth.shape
    K, P = np.asarray(K, np.float64), np.asarray(poses, np.float64).reshape(n, 3, 4)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    y, x = (a.astype(np.float64) for a in np.mgrid[0:rows, 0:cols])
    xyz, nrm, rgb = [], [], []
    with np.errstate(all="ignore"):
        for r in range(n):
            z = depth[r].astype(np.float64)
            R, t = P[r, :, :3], P[r, :, 3]
            a, b, c = (x - cx) / fx * z - t[0], (y - cy) / fy * z - t[1], z - t[2]
            X = [(R[0, j] * a + R[1, j] * b) + R[2, j] * c for j in range(3)]       # R^T (z K^-1 p - t)
            count, owner = np.ones((rows, cols), np.int64), np.ones((rows, cols), bool)
            for v in range(n):
                if v == r:
                    continue
                Q = P[v]
                xi, yi, zi = (((Q[i, 0] * X[0] + Q[i, 1] * X[1]) + Q[i, 2] * X[2]) + Q[i, 3] for i in range(3))
                pu, pv = np.floor((fx * (xi / zi) + cx) + 0.5), np.floor((fy * (yi / zi) + cy) + 0.5)
                ins = (zi > 0.0) & (pu >= 0.0) & (pv >= 0.0) & (pu < float(cols)) & (pv < float(rows))
                zv = depth[v][np.where(ins, pv, 0.0).astype(np.int64), np.where(ins, pu, 0.0).astype(np.int64)].astype(np.float64)
                cons = ins & (zv > 0.0) & (np.abs(zv - zi) <= eps * zi)
                count += cons
                if v < r:
                    owner &= ~cons
            keep = (z > 0.0) & (count >= min_views) & owner
            d = [-((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2]) - X[j] for j in range(3)]   # C_r - X
            ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            xyz.append(np.stack([X[j][keep] for j in range(3)], 1).astype(np.float32))
            nrm.append(np.stack([np.where(ln > 0.0, d[j] / ln, 0.0)[keep] for j in range(3)], 1).astype(np.float32))
            if bgr is not None:
                q = np.asarray(bgr)[r][keep].astype(np.uint32)
                rgb.append((q[:, 2] << 16) | (q[:, 1] << 8) | q[:, 0])
            else:
                rgb.append(np.asarray(gray)[r][keep].astype(np.uint32) * np.uint32(0x010101))
    return np.concatenate(xyz), np.concatenate(nrm), np.concatenate(rgb).astype(np.uint32)


def ref_run(gray, K, poses, dmin, dmax, opts, bgr=None, level=0, stats=None):
    """rule 1, rule 6, every depth map, rule 7: ((xyz, normals, rgb), [(idx, depth, score) per view])"""
    g = np.stack([ref_pyramid(im, level) for im in gray])
    b = np.stack([ref_pyramid(im, level) for im in bgr]) if bgr is not None else None
    KL, n = ref_level_K(K, level), len(g)
    lo, hi = np.broadcast_to(np.asarray(dmin, np.float64), (n,)), np.broadcast_to(np.asarray(dmax, np.float64), (n,))
    maps = []
    for v in range(n):
        src = ref_sources(poses, v, opts["n_src"])
        H = ref_homographies(KL, poses, v, src, opts["n_planes"], lo[v], hi[v])
        maps.append(ref_depthmap(g, H, v, src, opts, lo[v], hi[v], stats=stats))
    return ref_fuse(KL, poses, np.stack([m[1] for m in maps]), g, b, opts["eps"], opts["min_views"]), maps


# ---------------------------------------------------------------- scenes
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def make_poses(R, C):
    """[n, 3, 4] = [R | -R C] of rotations R [n, 3, 3] and centres C [n, 3]"""
    return np.concatenate([R, -np.einsum("nij,nj->ni", R, C)[:, :, None]], 2)


def posed_cameras(n, rng, rot, jitter, baseline):
    """n cameras on the x axis around 0, `baseline` apart, each centre moved by N(0, jitter) per axis and each camera turned
    by the Rodrigues vector N(0, rot) per axis"""
    C = np.zeros((n, 3))
    C[:, 0] = (np.arange(n) - (n - 1) / 2) * baseline
    C += rng.normal(0, jitter, (n, 3)) if jitter else 0.0
    R = np.stack([rodrigues(rng.normal(0, rot, 3)) if rot else np.eye(3) for _ in range(n)])
    return make_poses(R, C)


def render_posed(K, rows, cols, poses, surfaces, lam, seed=1):
    """tests/test_mvs_cpu.py's render() for any [R | t]: rays R^T K^-1 p from C = -R^T t, the depth in the camera frame (the
    ray parameter, the camera-frame ray being (dx, dy, 1)), the texture in the world's X, Y.  surfaces: ("plane", n, d) for
    n . X = d, ("sphere", centre, radius).  Returns (gray [n, rows, cols] uint8, depth [n, rows, cols], inf where nothing is hit)."""
    x, y = np.meshgrid(np.arange(cols, dtype=float), np.arange(rows, dtype=float))
    ray = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones_like(x)], -1)
    gray, depth = [], []
    for P in np.asarray(poses, float).reshape(-1, 3, 4):
        R, C = P[:, :3], -P[:, :3].T @ P[:, 3]
        d = ray @ R                                    # R^T ray per pixel
        z = np.full(x.shape, np.inf)
        for s in surfaces:
            with np.errstate(all="ignore"):
                if s[0] == "plane":
                    t = (s[2] - np.asarray(s[1], float) @ C) / (d @ np.asarray(s[1], float))
                else:
                    oc = C - np.asarray(s[1], float)
                    a, b = (d * d).sum(-1), 2 * (d @ oc)
                    disc = b * b - 4 * a * (oc @ oc - s[2] ** 2)
                    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
            z = np.where((t > 0) & (t < z), t, z)
        hit = np.isfinite(z)
        X = C + np.where(hit, z, 0.0)[..., None] * d
        g = np.clip(np.rint(127.5 + 110 * texture(X[..., 0], X[..., 1], lam, seed)), 0, 255)
        gray.append(np.where(hit, g, 0).astype(np.uint8))
        depth.append(z)
    return np.stack(gray), np.stack(depth)


def smooth_views(rng, n, rows, cols, shifts, passes=2):
    """a smooth random texture (uniform noise under `passes` 3 x 3 box means, stretched to 0 ... 255, periodic), seen
    shifted by shifts[v] = (rows, columns) in view v"""
    a = rng.rand(rows + 16, cols + 16)
    for _ in range(passes):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0)) / 3
        a = (a + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 3
    a = np.rint(255 * (a - a.min()) / (a.max() - a.min())).astype(np.uint8)
    return np.stack([np.roll(a, s, (0, 1))[:rows, :cols] for s in shifts[:n]])


# ---------------------------------------------------------------- the cases (the table is in tests/test_mvs_reference_cpu.py)
class Case:
    """one depth map (view `ref` against `src` between dmin and dmax under the options kw) and, where `run` is set, the whole
    call on the same views.  The images are those given to create(); the sweep sees them at `level`."""

    def __init__(self, gray, poses, kw, K=K_AWK, ref=None, src=None, dmin=1.0, dmax=8.0, bgr=None, level=0, run=True):
        self.gray, self.bgr, self.K, self.poses, self.level, self.run = gray, bgr, np.array(K), poses, level, run
        self.kw, self.opts, self.dmin, self.dmax = kw, ref_opts(**kw), dmin, dmax
        self.ref = len(gray) // 2 if ref is None else ref
        self.src = list(ref_sources(poses, self.ref, self.opts["n_src"]) if src is None else src)
        for a in (self.gray, self.bgr, self.K, self.poses):
            if a is not None:
                a.setflags(write=False)


SHIFTS = [(0, 0), (1, -2), (-1, 2), (2, 1), (-2, -1), (1, 1), (-1, -1), (0, 2), (2, -1)]


def s1_poses():
    return posed_cameras(5, np.random.RandomState(11), 0.05, 0.02, 0.04)


def case_s1():
    gray = smooth_views(np.random.RandomState(12), 5, 33, 47, SHIFTS)
    return Case(gray, s1_poses(), dict(n_planes=17, window=3, n_src=4, n_best=2, **ALL_PIXELS), ref=2, src=[1, 3, 0, 4])


def case_s2():
    P = s1_poses()
    gray, _ = render_posed(K_AWK, 33, 47, P, [("plane", (0, 0, 1), 3.0)], 8 * 3.0 / 100)
    return Case(gray, P, dict(n_planes=17, window=7, n_src=4, n_best=4), ref=2, src=[1, 3, 0, 4])


S3_PLANE, S3_LAM, S3_D = 1 / (1 / 8.0 + 16 * (1 - 1 / 8.0) / 32), 8 * 1.78 / 100, 33


def case_s3():
    P = posed_cameras(5, np.random.RandomState(31), 0.04, 0.02, 0.16)
    gray, _ = render_posed(K_AWK, 40, 56, P, [("plane", (0, 0, 1), S3_PLANE)], S3_LAM)
    return Case(gray, P, dict(n_planes=S3_D), bgr=np.ascontiguousarray(np.stack([gray, 255 - gray, gray // 3], -1)))


def s3_truth():
    c = case("S3")
    return render_posed(K_AWK, 40, 56, c.poses, [("plane", (0, 0, 1), S3_PLANE)], S3_LAM)[1]


def case_s4():
    """view 1 rolled 90 degrees about the optical axis, view 2 yawed 80 degrees: c <= 0 on part of the image, u and v
    leaving on all four sides"""
    R = np.stack([np.eye(3), rodrigues([0, 0, np.pi / 2]), rodrigues([0, np.radians(80), 0])])
    C = np.array([[0, 0, 0], [0.05, 0.02, 0.0], [-0.04, 0.03, 0.01]])
    gray = smooth_views(np.random.RandomState(41), 3, 33, 47, SHIFTS)
    return Case(gray, make_poses(R, C), dict(n_planes=9, window=2, n_src=2, n_best=1, **ALL_PIXELS), ref=0, src=[1, 2])


def case_s4_back():
    """view 2 yawed 180 degrees: every sample of it has c < 0 and, were that not asked, would land inside the image"""
    R = np.stack([np.eye(3), rodrigues([0.01, -0.02, 0.015]), rodrigues([0, np.pi, 0])])
    C = np.array([[0, 0, 0], [0.03, 0.01, 0.0], [0.0, 0.0, 0.0]])
    gray = smooth_views(np.random.RandomState(43), 3, 33, 47, SHIFTS)
    return Case(gray, make_poses(R, C), dict(n_planes=9, window=2, n_src=2, n_best=1, **ALL_PIXELS), ref=0, src=[1, 2])


def case_s5():
    """dmax = dmin + 1e-7: every plane warps to the same 1/32-pixel samples, every score ties"""
    P = posed_cameras(3, np.random.RandomState(51), 0.005, 0.0, 0.1)
    gray = smooth_views(np.random.RandomState(52), 3, 33, 47, SHIFTS)
    return Case(gray, P, dict(n_planes=9, n_src=2, n_best=1, **ALL_PIXELS), ref=1, src=[0, 2], dmin=4.0, dmax=4.0 + 1e-7)


def case_s7():
    """white images with about one black pixel in 30, window 7: a window's sum of q^2 passes 2^31"""
    rng = np.random.RandomState(71)
    base = np.where(rng.rand(40, 60 + 18) < 1 / 30, 0, 255).astype(np.uint8)
    gray = np.stack([base[:, 9 * (2 - v):9 * (2 - v) + 60] for v in range(3)])   # 9 pixels of disparity on plane 4 of 9
    K = np.array([[100.0, 0, 29.5], [0, 100.0, 19.5], [0, 0, 1]])
    P = posed_cameras(3, None, 0.0, 0.0, 0.16)
    return Case(gray, P, dict(n_planes=9, window=7, n_src=2, n_best=1, **ALL_PIXELS), K=K, ref=1, src=[0, 2])


def s8_views(flat_ref):
    P = posed_cameras(3, np.random.RandomState(81), 0.01, 0.005, 0.05)
    gray, _ = render_posed(K_AWK, 40, 60, P, [("plane", (0, 0, 1), 3.0)], 8 * 3.0 / 100)
    gray[:, :, :27] = 128                              # the seam at column 27: inside the tile of columns 16 ... 31
    if flat_ref:
        gray[1] = 128
    return gray, P


def case_s8_seam():
    gray, P = s8_views(False)
    return Case(gray, P, dict(n_planes=9, n_src=2, n_best=1, ncc_min=-1.0), ref=1, src=[0, 2])


def case_s8_flat():
    gray, P = s8_views(True)
    return Case(gray, P, dict(n_planes=9, n_src=2, n_best=1, ncc_min=-1.0), ref=1, src=[0, 2])


S9_SIZES = [(1, 1, 1), (1, 40, 1), (40, 1, 1), (2, 2, 1), (3, 3, 1), (15, 15, 7), (15, 17, 7), (16, 16, 3), (17, 17, 3), (31, 33, 7)]
S9_EMPTY = [(15, 15, 7), (15, 17, 7)]                  # no pixel with depth
S9_SOME = [(16, 16, 3), (17, 17, 3), (31, 33, 7)]      # at least one


def case_s9(rows, cols, w):
    P = posed_cameras(3, np.random.RandomState(91), 0.01, 0.005, 0.03)
    gray = smooth_views(np.random.RandomState(92), 3, 40, 40, SHIFTS)[:, :rows, :cols].copy()
    return Case(gray, P, dict(n_planes=5, window=w, n_src=2, n_best=1, **ALL_PIXELS), ref=1, src=[0, 2])


def case_s10():
    """the ceilings together: 256 planes, 8 sources, best 4 (the whole call is compared between device and stub only)"""
    rng = np.random.RandomState(101)
    R = np.stack([rodrigues(rng.normal(0, 0.02, 3)) for _ in range(9)])
    P = make_poses(R, rng.normal(0, 0.015, (9, 3)))
    gray = smooth_views(rng, 9, 24, 37, SHIFTS)
    return Case(gray, P, dict(n_planes=256, n_src=8, n_best=4, **ALL_PIXELS), ref=4, src=[0, 1, 2, 3, 5, 6, 7, 8], run=False)


def case_s11(rows, cols, level):
    """a 1 x 1 or 1 x 2 working image: created, swept and fused"""
    rng = np.random.RandomState(111)
    gray = rng.randint(0, 256, (3, rows, cols)).astype(np.uint8)
    bgr = rng.randint(0, 256, (3, rows, cols, 3)).astype(np.uint8)
    P = posed_cameras(3, rng, 0.01, 0.005, 0.03)
    return Case(gray, P, dict(n_planes=5, window=1, n_src=2, n_best=1, min_views=1, **ALL_PIXELS), ref=1, src=[0, 2], bgr=bgr, level=level)


def s12_views(n):
    P = posed_cameras(n, np.random.RandomState(121), 0.02, 0.01, 0.04)
    return smooth_views(np.random.RandomState(122), n, 33, 47, SHIFTS), P


def case_s12_two_views():
    gray, P = s12_views(2)
    return Case(gray, P, dict(n_planes=9, n_src=4, n_best=1, min_views=2, eps=0.05, **ALL_PIXELS), ref=0, src=[1])


def case_s12_five_views():
    gray, P = s12_views(5)
    return Case(gray, P, dict(n_planes=9, n_src=8, n_best=4, min_views=2, eps=0.05, **ALL_PIXELS), ref=2, src=[1, 3, 0, 4])


S12_DMIN, S12_DMAX = np.array([1.0, 1.5, 0.8, 2.0, 1.2]), np.array([8.0, 6.0, 9.5, 7.0, 12.0])


def case_s12_ranges():
    gray, P = s12_views(5)
    return Case(gray, P, dict(n_planes=9, min_views=2, eps=0.05, **ALL_PIXELS), ref=2, dmin=S12_DMIN, dmax=S12_DMAX)


CASES = {"S1": case_s1, "S2": case_s2, "S3": case_s3, "S4": case_s4, "S4-back": case_s4_back, "S5": case_s5, "S7": case_s7, "S8-seam": case_s8_seam,
         "S8-flat": case_s8_flat, "S10": case_s10, "S11-3x3": lambda: case_s11(3, 3, 1), "S11-7x9": lambda: case_s11(7, 9, 2),
         "S12-two": case_s12_two_views, "S12-five": case_s12_five_views, "S12-ranges": case_s12_ranges}
CASES.update({f"S9-{r}x{c}": functools.partial(case_s9, r, c, w) for r, c, w in S9_SIZES})


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


class Reference:
    pass


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per process, shared, never written to: .idx .depth .score of the case's depth map, .stats of its
    samples, and where the case runs the whole call .points = (xyz, normals, rgb) and .maps (every view's triple)"""
    c, out = case(name), Reference()
    g = np.stack([ref_pyramid(im, c.level) for im in c.gray])
    lo, hi = (float(np.broadcast_to(a, (len(g),))[c.ref]) for a in (c.dmin, c.dmax))
    out.stats = new_stats()
    H = ref_homographies(ref_level_K(c.K, c.level), c.poses, c.ref, c.src, c.opts["n_planes"], lo, hi)
    out.idx, out.depth, out.score = ref_depthmap(g, H, c.ref, c.src, c.opts, lo, hi, stats=out.stats)
    out.points = out.maps = None
    if c.run:
        out.points, out.maps = ref_run(c.gray, c.K, c.poses, c.dmin, c.dmax, c.opts, bgr=c.bgr, level=c.level)
    for a in (out.idx, out.depth, out.score) + tuple(out.points or ()) + tuple(a for m in out.maps or () for a in m):
        a.setflags(write=False)
    return out


def s12_reuse(D):
    """the whole call at D planes on three views (one handle runs it at 9, 256 and 9 planes again)"""
    gray, P = s12_views(3)
    return Case(gray, P, dict(n_planes=D, n_src=2, n_best=1, min_views=2, eps=0.05, **ALL_PIXELS), ref=1, src=[0, 2])


CASES.update({"S12-reuse-9": functools.partial(s12_reuse, 9), "S12-reuse-256": functools.partial(s12_reuse, 256)})


def same_bits(a, b):
    """bit for bit, except that a NaN must meet a NaN in the same entry: the host's and the device's NaNs differ in sign
    (as same_bits of tests/test_gpu_tracks.py)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na = np.isnan(a)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, np.isnan(b)) and np.array_equal(a.view(u)[~na], b.view(u)[~na]))


def s3_step_errors(maps):
    """|refined inverse depth - render_posed's| in hypothesis steps over every pixel with depth of the five views:
    (pixels, median, 95th percentile)"""
    truth = s3_truth()
    has = np.stack([m[0] for m in maps]) >= 0
    d = np.stack([m[1] for m in maps]).astype(np.float64)
    e = np.abs(1 / d[has] - 1 / truth[has]) / ((1 - 1 / 8.0) / (S3_D - 1))
    return int(has.sum()), float(np.median(e)), float(np.percentile(e, 95))


# fusion: tests/test_mvs_cpu.py's dyadic 8 x 8 views (fx = fy = 8, cx = cy = 3.5, a plane at depth 2), everything exact
FK = np.array([[8.0, 0, 3.5], [0, 8.0, 3.5], [0, 0, 1]])


def fusion_line(n, baseline, seed=3):
    P = np.zeros((n, 3, 4))
    P[:, :, :3] = np.eye(3)
    P[:, 0, 3] = -baseline * np.arange(n)
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, 8, 8)).astype(np.uint8), rng.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8), P


def half_pixel_has(n, seed=5):
    """which pixels have depth: about three in four, so that the column a projection is rounded to matters"""
    return np.random.RandomState(seed).rand(n, 8, 8) < 0.75


def half_pixel_expected(n, min_views, has):
    """centres 0.125 apart: pixel x of view r projects to u = x + (r - v) / 2 in view v, so floor(u + 1/2) decides, also at
    u = -0.5 (pixel 0: inside) and u = 7.5 (pixel 8: outside).  (view, row, column) of the kept points, in integers."""
    out = []
    for r in range(n):
        for y in range(8):
            for x in range(8):
                col = {v: (2 * x + (r - v) + 1) // 2 for v in range(n) if v != r}
                cons = [v for v, u in col.items() if 0 <= u < 8 and has[v, y, u]]
                if has[r, y, x] and 1 + len(cons) >= min_views and all(v > r for v in cons):
                    out.append((r, y, x))
    return out


ODD_DEPTHS = (np.nan, np.inf, -1.0, 0.0, 1e-45, 1e30)   # (1e-45 rounds to the smallest float32 denormal)


def odd_depth_maps(n):
    """depth 2 everywhere but for the odd values, each in one pixel of every view (another pixel in each)"""
    d = np.full((n, 8, 8), 2.0, np.float32)
    for v in range(n):
        for i, z in enumerate(ODD_DEPTHS):
            d[v, (1 + i + v) % 8, (2 + 2 * i + 3 * v) % 8] = z
    return d
