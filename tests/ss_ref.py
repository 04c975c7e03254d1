"""A plain restatement of the supersampling filter (rt_set_samples, include/rt_api.h).

A frame with n x n samples per pixel is the box filter, in a fixed float32 order, of
the one-sample frame of n*W x n*H pixels rendered with resX*n, resY*n. Per channel
(alpha included): log2 n rounds along x, each a[..., i] = a[..., 2i] + a[..., 2i+1];
then log2 n such rounds along y; then one multiply by 1/n^2 (a power of two: exact).
"""
import numpy as np

SAMPLES = (1, 2, 4, 8)


def box(img, n):
    """img: (n*H, n*W, C) float32 -> (H, W, C) float32, in the normative order."""
    a = np.ascontiguousarray(img, np.float32)
    if n not in SAMPLES:
        raise ValueError("n must be 1, 2, 4 or 8")
    if a.ndim != 3 or a.shape[0] % n or a.shape[1] % n:
        raise ValueError("the sample frame's extents must be multiples of n")
    k = n
    while k > 1:  # rounds along x
        a = a[:, 0::2] + a[:, 1::2]
        k //= 2
    k = n
    while k > 1:  # rounds along y
        a = a[0::2] + a[1::2]
        k //= 2
    assert a.dtype == np.float32
    return a * np.float32(1.0 / (n * n))
