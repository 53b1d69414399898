"""Shared by tests/test_oracle_sift.py and tests/test_gpu_sift.py: seeded test images for the SIFT front end, the table of
cases (image, parameters) both files run, the numpy restatement's answer per case (computed once per process) and what
that answer shows about a case: sites with several orientations, octaves, descriptor windows that leave the image."""
import functools

import numpy as np

from oracle import sfm_oracle_sift as S

DEFAULTS = dict(n_layers=3, contrast_thr=0.04, edge_thr=10.0, sigma=1.6)


# ---------------------------------------------------------------- generators
def texture(h, w, seed):
    """band-limited 1/f noise (amplitude 1/f from 0.03 to 0.12 cycles per pixel, nothing outside: the contrast sits at the
    scales the first octaves detect), mean 128, standard deviation 50 before the clip to 0..255: keypoints all over
    the image, many with several orientations, most with windows that pass a border"""
    rng = np.random.default_rng(seed)
    f = np.hypot(np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :])
    amp = np.where((f >= 0.03) & (f <= 0.12), 1.0 / np.maximum(f, 1e-9), 0.0)
    img = np.fft.ifft2(np.fft.fft2(rng.normal(size=(h, w))) * amp).real
    return np.clip(np.rint(128.0 + 50.0 * img / img.std()), 0, 255).astype(np.uint8)


def checker(h, w, cell=(7, 9)):
    """a 0 / 255 checkerboard with cells of cell[0] rows x cell[1] columns: saturated edges (the edge test rejects) and
    corners (several orientation peaks)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // cell[0] + xx // cell[1]) & 1) * 255).astype(np.uint8)


def blocks(h, w, seed, side=4):
    """random 0 / 255 blocks of side x side pixels"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, ((h + side - 1) // side, (w + side - 1) // side))
    return (np.kron(b, np.ones((side, side), np.int64))[:h, :w] * 255).astype(np.uint8)


def corner_blob(h=64, w=64, seed=0, s=9.0, at=(13.0, 12.0)):
    """one Gaussian blob of sigma s centred at (x, y) = at, near the top-left corner, over noise of sigma 1.5: a keypoint
    in a coarse octave whose orientation and descriptor windows spill over two borders"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 30.0 + 190.0 * np.exp(-((xx - at[0]) ** 2 + (yy - at[1]) ** 2) / (2 * s * s)) + rng.normal(0, 1.5, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def sliver(h, w, seed):
    """the degenerate sizes: a blob of sigma 1.4 at the centre over noise of sigma 6 (where an octave is higher and wider
    than twice the border there is something to find; elsewhere the answer is no keypoint)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 40.0 + 180.0 * np.exp(-((xx - (w - 1) / 2) ** 2 + (yy - (h - 1) / 2) ** 2) / (2 * 1.4 * 1.4)) + rng.normal(0, 6.0, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- the cases: name -> (image factory, parameters)
def _tex129():
    return texture(36, 129, 1)


CASES = {
    # width past one block of 256 threads in x: base widths 258 (the second block holds 2 threads), 360, 264, 300; the
    # 280-wide strip (base 560) is the one whose octave after the base is wider than a block too, so that the halving
    # runs a second x block (24 threads) -- in the others only the up-sampling and the blurs of the base octave do
    "texture_129": (_tex129, {}),
    "texture_180": (lambda: texture(36, 180, 2), {}),
    "checker_132": (lambda: checker(40, 132), {}),
    "blocks_150": (lambda: blocks(40, 150, 3), {}),
    "texture_280": (lambda: texture(16, 280, 5), {}),
    # layers (texture_129 is the 3-layer case)
    "layers_1": (_tex129, dict(n_layers=1)),
    "layers_2": (_tex129, dict(n_layers=2)),
    "layers_5": (_tex129, dict(n_layers=5)),
    "layers_8": (_tex129, dict(n_layers=8)),
    # sigma
    "sigma_1.0": (_tex129, dict(sigma=1.0)),
    "sigma_2.4": (_tex129, dict(sigma=2.4)),
    # thresholds
    "thr_0.09_3": (_tex129, dict(contrast_thr=0.09, edge_thr=3.0)),
    "thr_0_1000": (_tex129, dict(contrast_thr=0.0, edge_thr=1000.0)),
    "thr_0.2_10": (_tex129, dict(contrast_thr=0.2, edge_thr=10.0)),
    # windows off the image
    "corner_blob": (corner_blob, {}),
}
WIDTH_CASES = ("texture_129", "texture_180", "checker_132", "blocks_150", "texture_280")
DENSE_CASES = tuple(n for n in CASES if n not in ("thr_0.2_10", "corner_blob"))     # >= 20 keypoints each
DEGENERATE_SHAPES = ((2, 2), (5, 5), (2, 300), (200, 6), (6, 200), (11, 40))


def image(name):
    return CASES[name][0]()


def params(name):
    return dict(DEFAULTS, **CASES[name][1])


def degenerate_image(shape):
    return sliver(shape[0], shape[1], 7)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's (keypoints, descriptors) of a case: computed once per process, shared, never modified"""
    K, D = S.detect_and_compute(image(name), **params(name))
    K.setflags(write=False)
    D.setflags(write=False)
    return K, D


@functools.lru_cache(maxsize=None)
def degenerate_reference(shape, n_layers=3, sigma=1.6):
    K, D = S.detect_and_compute(degenerate_image(shape), n_layers=n_layers, sigma=sigma)
    K.setflags(write=False)
    D.setflags(write=False)
    return K, D


# ---------------------------------------------------------------- what a keypoint list shows
def multi_sites(K):
    """sites (x, y, size) that carry more than one angle"""
    _, cnt = np.unique(np.ascontiguousarray(K[:, :3]).view(np.int32), axis=0, return_counts=True)
    return int((cnt > 1).sum())


def octaves(K):
    """the stored octave index of every keypoint (-1 = the doubled base)"""
    o = np.ascontiguousarray(K[:, 5]).view(np.int32) & 255
    return np.where(o < 128, o, o - 256)


def borders_crossed(K, shape):
    """per keypoint: (the descriptor window 3 sqrt(2) 2.5 size / 2 passes the left or right border, ... the top or bottom)"""
    h, w = shape
    rad = 3.0 * np.sqrt(2.0) * 2.5 * K[:, 2].astype(np.float64) / 2
    x, y = K[:, 0].astype(np.float64), K[:, 1].astype(np.float64)
    return np.minimum(x, w - 1 - x) < rad, np.minimum(y, h - 1 - y) < rad


def windows_off(K, shape):
    """keypoints whose descriptor window radius exceeds their distance to the nearest border"""
    bx, by = borders_crossed(K, shape)
    return int((bx | by).sum())


# ---------------------------------------------------------------- non-vacuity: what the restatement alone must show
def check_case(name):
    """a case on its own: the dense ones have keypoints to compare, corner_blob has its coarse keypoint over two borders"""
    K, _ = reference(name)
    if name in DENSE_CASES:
        assert len(K) >= 20, (name, len(K))
    if name == "texture_280":                      # something found in the halved octaves right of column 256
        assert ((octaves(K) >= 0) & (K[:, 0] >= 256)).any()
    if name == "corner_blob":
        bx, by = borders_crossed(K, image(name).shape)
        assert ((octaves(K) >= 1) & bx & by).any(), (octaves(K), bx, by)


def check_groups():
    """what the groups of cases have to exercise between them (the keypoint counts are the restatement's)"""
    refs = {n: reference(n)[0] for n in CASES}
    for n in CASES:
        check_case(n)
    # the default-parameter width cases: several orientations per site, three octaves, windows beyond the border
    assert sum(multi_sites(refs[n]) for n in WIDTH_CASES) >= 5 and multi_sites(refs["checker_132"]) >= 20
    assert len(set(np.concatenate([octaves(refs[n]) for n in WIDTH_CASES]).tolist())) >= 3
    assert sum(windows_off(refs[n], image(n).shape) for n in WIDTH_CASES) >= 20
    # the thresholds cut, the layer count changes the answer
    assert len(refs["thr_0.2_10"]) < len(refs["thr_0.09_3"]) < len(refs["texture_129"])
    # (layers_1, layers_8 and texture_129 are the same image)
    assert CASES["layers_1"][0] is CASES["layers_8"][0] is CASES["texture_129"][0]
    for n in ("layers_1", "layers_8"):
        assert len(refs[n]) != len(refs["texture_129"])
        assert not set(map(bytes, refs[n][:, :3])) >= set(map(bytes, refs["texture_129"][:, :3]))     # other sites, not only more
    # a tiny image that has something to compare
    assert len(degenerate_reference((11, 40))[0]) >= 1
