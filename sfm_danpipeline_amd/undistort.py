"""Lens distortion in front of the dense stereo (include/sfmhip.h, sfmhip_image_undistort; csrc/undistort.hip; DESIGN.md
f-14): pictures of a camera with the five coefficients k1 k2 p1 p2 k3 of the calibration file, resampled on the GPU into the
pinhole camera of the same K.  One map per call (it depends on K, the coefficients and the size only), one gather over all
pictures and channels; fractions of 1/32 pixel and an integer blend, so the result equals the header's host build byte for
byte.

`undistort(images, K, dist)` returns (images [n, rows, cols(, 3)] uint8, valid [rows, cols] uint8: 0 where a tap fell off the
source, and the picture is 0 there); `last_timing()` the kernel times of the last call under Context.set_timing.
K is kept: pincushion coefficients leave a black margin, barrel coefficients crop (mvs.Mvs(dist=...) keeps its windows off
the margin)."""
import ctypes as C

import numpy as np

from . import _lib
from .mvs import image_pointers


def undistort(images, K, dist, ctx=None):
    """images: n arrays [rows, cols] (gray) or [rows, cols, 3] (BGR) of one shape."""
    ctx = ctx or _lib.default_context()
    first = np.asarray(images[0]) if len(images) else np.zeros((0, 0), np.uint8)
    ch = 3 if first.ndim == 3 else 1
    src, sp = image_pointers(images, ch)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    dist = np.ascontiguousarray(dist, np.float64).reshape(-1)
    if len(dist) != 5:
        raise ValueError("dist must be the five coefficients k1 k2 p1 p2 k3")
    rows, cols = first.shape[:2]
    out = np.zeros((len(src),) + first.shape, np.uint8)
    dp = (C.c_void_p * len(src))(*[out[i].ctypes.data for i in range(len(src))])
    valid = np.zeros((rows, cols), np.uint8)
    _lib.check(_lib.lib().sfmhip_image_undistort(ctx.h, len(src), rows, cols, ch, sp, K.ctypes.data, dist.ctypes.data, dp,
                                                 valid.ctypes.data), "sfmhip_image_undistort")
    return out, valid


def last_timing(ctx=None):
    """ms of the last undistort call on the context, by device events (zeros unless Context.set_timing is on): map, gather."""
    ctx = ctx or _lib.default_context()
    ms = np.zeros(2, np.float64)
    _lib.check(_lib.lib().sfmhip_image_undistort_last_timing(ctx.h, ms.ctypes.data), "sfmhip_image_undistort_last_timing")
    return dict(zip(("map", "gather"), map(float, ms)))
