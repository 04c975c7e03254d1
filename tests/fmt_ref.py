"""A plain numpy restatement of the display formats (include/rt_api.h: RT_FORMAT_RGBA8,
RT_FORMAT_SRGBA8, RT_FORMAT_RGBA16F), float32 throughout.

Per channel c of the float32 RGBA frame:
  rgba8   q = rint(min(max(c, 0), 1) * 255) in float32, nearest even; NaN gives 0; alpha 255.
  srgba8  R, G, B: q = the number of k in 1..255 with clamp(c) >= T[k], T the 255 thresholds
          given as an argument (rtamd.srgb_thresholds()); NaN gives 0; alpha 255.
  rgba16f IEEE float32 -> float16, nearest even, no clamp; alpha 1.0 (0x3C00).
The frame's own alpha is exactly 1, so the fixed alphas are also its conversions.
"""
import numpy as np

RGBA8, SRGBA8, RGBA16F = 3, 4, 5  # rt_format
DTYPE = {RGBA8: np.uint8, SRGBA8: np.uint8, RGBA16F: np.float16}
BYTES = {RGBA8: 4, SRGBA8: 4, RGBA16F: 8}


def clamp01(c):
    """fminf(fmaxf(c, 0), 1) with C's NaN rule: fmaxf(NaN, 0) is 0."""
    c = np.asarray(c, np.float32)
    c = np.where(np.isnan(c), np.float32(0), c)
    return np.minimum(np.maximum(c, np.float32(0)), np.float32(1)).astype(np.float32)


def unorm8(c):
    p = clamp01(c) * np.float32(255.0)
    assert p.dtype == np.float32
    return np.rint(p).astype(np.uint8)


def srgb8(c, T):
    T = np.asarray(T, np.float32)
    assert T.shape == (255,)
    return np.searchsorted(T, clamp01(c), side="right").astype(np.uint8)


def half(c):
    with np.errstate(over="ignore"):
        return np.asarray(c, np.float32).astype(np.float16)


def convert(img, fmt, T=None):
    """img: (..., 4) float32 RGBA -> (..., 4) uint8 or float16 in format `fmt`."""
    a = np.asarray(img, np.float32)
    if a.shape[-1] != 4:
        raise ValueError("convert expects RGBA in the last axis")
    if fmt == RGBA16F:
        out = half(a)
        out[..., 3] = np.float16(1.0)
        return out
    if fmt == RGBA8:
        out = unorm8(a)
    elif fmt == SRGBA8:
        out = srgb8(a, T)
    else:
        raise ValueError("not a display format")
    out[..., 3] = 255
    return out
