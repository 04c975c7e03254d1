"""Adaptive supersampling's definition (tests/adaptive_ref.py), the oracle facts the GPU tests
lean on, and the interface that carries it (no GPU)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import adaptive_ref as ar
import oracle
import rtamd

F = np.float32
FULL3 = np.arange(3)
FULL4 = np.arange(4)


def flat(h, w, v=0.25):
    img = np.full((h, w, 4), v, np.float32)
    img[..., 3] = 1.0
    return img


def test_a_bright_pixel_refines_itself_and_its_four_neighbours():
    B = flat(3, 3)
    B[1, 1, 1] = 0.75  # one channel is enough
    want = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    assert np.array_equal(ar.mask(B, FULL3, 1 / 16), want)
    B = flat(4, 4)
    B[0, 3, 2] = 1.0  # a corner: two neighbours inside the frame
    want = np.zeros((4, 4), bool)
    want[0, 3] = want[0, 2] = want[1, 3] = True
    assert np.array_equal(ar.mask(B, FULL4, 1 / 16), want)


def test_the_comparison_is_not_above_the_threshold():
    """!(d <= t): a contrast equal to the threshold does not refine, the next float does."""
    B = flat(3, 3, 0.0)
    B[1, 1, 0] = F(1 / 16)
    assert not ar.mask(B, FULL3, 1 / 16).any()
    B[1, 1, 0] = np.nextafter(F(1 / 16), F(1))
    assert ar.mask(B, FULL3, 1 / 16).sum() == 5
    assert ar.mask(B, FULL3, 0.0).sum() == 5 and not ar.mask(flat(3, 3), FULL3, 0.0).any()


def test_alpha_does_not_enter():
    B = flat(3, 3)
    B[1, 1, 3] = 0.0
    assert not ar.mask(B, FULL3, 1 / 16).any()


def test_nan_refines_and_inf_refines_nothing():
    B = flat(4, 4)
    B[2, 1, 0] = np.nan
    want = np.zeros((4, 4), bool)
    want[2, 1] = want[1, 1] = want[3, 1] = want[2, 0] = want[2, 2] = True
    assert np.array_equal(ar.mask(B, FULL4, 1 / 16), want)
    assert np.array_equal(ar.mask(B, FULL4, np.inf), want)  # !(NaN <= inf)
    B = flat(4, 4)
    B[1, 2, :3] = 1e30
    assert not ar.mask(B, FULL4, np.inf).any()
    with pytest.raises(ValueError):
        ar.mask(B, FULL4, np.nan)


def test_no_vertical_neighbour_across_a_stripe_gap():
    """stripe = 2, period = 6: compact rows 0..3 are image rows 0, 1, 6, 7. A bright pixel in
    compact row 1 reaches row 0, not row 2; one in row 2 reaches row 3, not row 1."""
    y = ar.rows_of(8, 0, 2, 6, 4)
    assert list(y) == [0, 1, 6, 7]
    B = flat(4, 4)
    B[1, 1, 0] = 1.0
    want = np.zeros((4, 4), bool)
    want[1, 0:3] = True
    want[0, 1] = True
    assert np.array_equal(ar.mask(B, y, 1 / 16), want)
    B = flat(4, 4)
    B[2, 2, 0] = 1.0
    want = np.zeros((4, 4), bool)
    want[2, 1:4] = True
    want[3, 2] = True
    assert np.array_equal(ar.mask(B, y, 1 / 16), want)
    # the same frame as whole rows: the gap closes
    assert ar.mask(B, FULL4, 1 / 16)[1, 2]


def test_compose_takes_s_where_refined():
    B, S = flat(3, 3, 0.25), flat(3, 3, 0.5)
    m = np.zeros((3, 3), bool)
    m[0, 2] = True
    out = ar.compose(B, S, m)
    assert out.dtype == np.float32 and out[0, 2, 0] == 0.5 and (out[..., 0] == 0.5).sum() == 1
    assert (out[..., 3] == 1.0).all()
    with pytest.raises(ValueError):
        ar.compose(B, S[:2], m)


@functools.lru_cache(maxsize=None)
def oracle_one(cfg, W, H, n, s):
    """The oracle's one-sample W x H frame of the scene generated for the n*W x n*H sample frame."""
    fs = rtamd.generate(cfg, 0, n * W, n * H)
    img, _ = oracle.render(fs, W, H, oracle.params(W, H, *s))
    return img


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("cfg", [1, 2, 3])
def test_the_corner_sample_is_the_one_sample_pixel(cfg, n):
    """B(p) is sample (0, 0) of p's block, bit for bit: 2 (n x) / (n resX) and (n y) / (n resY)
    are the float32 values 2 x / resX and y / resY for n a power of two."""
    W, H, s = 20, 15, (2, True, False, False)
    fs = rtamd.generate(cfg, 0, n * W, n * H)
    one, _ = oracle.render(fs, W, H, oracle.params(W, H, *s))
    big, _ = oracle.render(fs, n * W, n * H, oracle.params(n * W, n * H, *s))
    assert np.array_equal(big[::n, ::n], one)


@pytest.mark.parametrize("case", ar.ORACLE_CASES, ids=lambda c: "c%d_%dx%d_n%d_b%d_f%d" % (
    c[0], c[1], c[2], c[3], c[4][0], c[4][2]))
def test_few_oracle_pixels_lie_near_the_threshold(case):
    """The GPU comparison against the oracle leaves out pixels whose oracle contrast lies within
    2e-4 of the threshold; that must stay a small share, and the mask must use both branches."""
    cfg, W, H, n, s = case
    B = oracle_one(cfg, W, H, n, s)
    y = np.arange(H)
    out = ar.near(B, y, ar.THRESHOLD)
    m = ar.mask(B, y, ar.THRESHOLD)
    print(f"cfg{cfg} {W}x{H}: refined {m.mean():.3f}, near the threshold {int(out.sum())} pixels")
    assert out.mean() <= ar.NEAR_CAP
    assert 0 < m.mean() < 1


def test_entry_points_are_exported_and_bound():
    assert rtamd.RT_SYMBOLS["rt_set_adaptive"] == (C.c_int, [C.c_void_p, C.c_float])
    assert rtamd.RT_SYMBOLS["rt_adaptive_stats"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    so = C.CDLL(os.path.join(rtamd.LIBDIR, "librtamd.so"))
    assert hasattr(so, "rt_set_adaptive") and hasattr(so, "rt_adaptive_stats")
    assert callable(rtamd.ComputeShader.set_adaptive) and callable(rtamd.ComputeShader.adaptive_stats)


def test_null_context_is_refused():
    lib = rtamd.rt_lib()
    assert lib.rt_set_adaptive(None, 0.5) == -1  # RT_ERR_INVALID
    assert lib.rt_adaptive_stats(None, None, None) == -1
