"""Frame comparisons that see non-finite values, shared by the GPU frame tests.

A plain `|a - b| > tol` is false wherever either side is NaN, so a frame with a NaN where the
oracle has a colour passes it. Both helpers here compare the NaN masks and the infinities
element for element first.
"""
import numpy as np


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def same_frame(a, b, what=""):
    """a and b are equal element for element: NaN equal to NaN in the same position (whatever
    the payload), infinities equal with their sign. For "kernel A == kernel B" and "refit ==
    fresh upload"."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    if np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
        return
    bad = a != b
    if a.dtype.kind == "f":
        bad &= ~(np.isnan(a) & np.isnan(b))
    at = _first(bad)
    raise AssertionError(f"{what}: {int(bad.sum())} values differ, first at {at}: {a[at]!r} vs {b[at]!r}")


def close_to_oracle(img, ref, tol, what=""):
    """img is the oracle's frame ref: NaN exactly where ref has NaN, the same infinity where ref
    has one, and within tol of ref everywhere else."""
    img, ref = np.asarray(img), np.asarray(ref)
    assert img.shape == ref.shape, f"{what}: shape {img.shape} vs the oracle's {ref.shape}"
    bad = np.isnan(img) != np.isnan(ref)
    if bad.any():
        at = _first(bad)
        raise AssertionError(f"{what}: NaN in {int(np.isnan(img).sum())} values, in {int(np.isnan(ref).sum())} of the "
                             f"oracle's; {int(bad.sum())} positions differ, first at {at}: {img[at]!r} vs the oracle's "
                             f"{ref[at]!r}")
    inf = np.isinf(img) | np.isinf(ref)
    bad = inf & (img != ref)
    if bad.any():
        at = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} infinities differ, first at {at}: {img[at]!r} vs the oracle's "
                             f"{ref[at]!r}")
    rest = ~(inf | np.isnan(ref))
    diff = np.zeros(img.shape, np.float64)
    diff[rest] = np.abs(img[rest].astype(np.float64) - ref[rest].astype(np.float64))
    bad = diff > tol
    if bad.any():
        at = _first(bad)
        px = int(bad.any(axis=-1).sum()) if bad.ndim > 1 else int(bad.sum())
        raise AssertionError(f"{what}: {px} pixels over {tol}, max diff {diff.max():.3g}, first at {at}: {img[at]!r} vs "
                             f"the oracle's {ref[at]!r}")
