"""The supersampling filter's definition (tests/ss_ref.py) and the interface that
carries it (no GPU): the numpy helper the GPU tests compare against is itself checked
against a naive mean and against hand-computed values that pin the summation order."""
import ctypes as C
import os

import numpy as np
import pytest

import rtamd
import ss_ref

F = np.float32


@pytest.mark.parametrize("n", [2, 4, 8])
def test_box_is_the_mean(n):
    """Against the float64 mean of each n x n block, within 1e-6 (values in [0, 1):
    a sum of 64 float32 terms carries at most 6 roundings of 2^-24 relative each)."""
    rng = np.random.default_rng(n)
    H, W = 5, 7
    img = rng.random((n * H, n * W, 4), dtype=np.float32)
    want = img.astype(np.float64).reshape(H, n, W, n, 4).mean(axis=(1, 3))
    got = ss_ref.box(img, n)
    assert got.shape == (H, W, 4) and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1e-6


def test_box_of_one_sample_is_the_frame():
    img = np.random.default_rng(0).random((3, 4, 4), dtype=np.float32)
    assert np.array_equal(ss_ref.box(img, 1), img)


def test_box_order_pairs_before_rows():
    """2 x 2 block [[a, b], [c, d]]: the filter is (a + b) + (c + d), x first.
    a = 2^24, b = 1, c = -2^24, d = 1: a + b rounds to 2^24 and c + d = -(2^24 - 1) is
    exact, so x first gives 1, while y first, (a + c) + (b + d), gives 2.
    a = 2^24, b = 0, c = 1, d = 1: (a + b) + (c + d) = 2^24 + 2, while the running sum
    ((a + b) + c) + d stays 2^24 (each + 1 is a tie that rounds to even)."""
    big = F(2.0 ** 24)
    blk = np.array([[big, 1.0], [-big, 1.0]], np.float32)[:, :, None]
    assert ss_ref.box(blk, 2)[0, 0, 0] == F(0.25)
    assert (blk[0, 0, 0] + blk[1, 0, 0]) + (blk[0, 1, 0] + blk[1, 1, 0]) == F(2.0)  # the other order differs
    blk = np.array([[big, 0.0], [1.0, 1.0]], np.float32)[:, :, None]
    assert ss_ref.box(blk, 2)[0, 0, 0] == F((2.0 ** 24 + 2.0) / 4.0)
    assert ((blk[0, 0, 0] + blk[0, 1, 0]) + blk[1, 0, 0]) + blk[1, 1, 0] == big  # the running sum differs


def test_box_order_is_a_balanced_tree():
    """4 x 4 with one non-zero row [2^24, 1, 1, 1]: rounds of adjacent pairs give
    (2^24 + 1 -> 2^24) + (1 + 1) = 2^24 + 2; left to right the sum stays 2^24. The same
    column-wise: the y rounds pair adjacent rows."""
    big = F(2.0 ** 24)
    blk = np.zeros((4, 4, 1), np.float32)
    blk[0, :, 0] = [big, 1, 1, 1]
    assert ss_ref.box(blk, 4)[0, 0, 0] == F((2.0 ** 24 + 2.0) / 16.0)
    assert ss_ref.box(blk.transpose(1, 0, 2), 4)[0, 0, 0] == F((2.0 ** 24 + 2.0) / 16.0)
    # 8 x 8: three rounds; [2^24, 1, 1, 1, 1, 1, 1, 1] -> (2^24 + 2) + 4 = 2^24 + 6
    blk = np.zeros((8, 8, 1), np.float32)
    blk[0, :, 0] = [big, 1, 1, 1, 1, 1, 1, 1]
    assert ss_ref.box(blk, 8)[0, 0, 0] == F((2.0 ** 24 + 6.0) / 64.0)


def test_box_keeps_alpha_one_and_blocks_apart():
    img = np.zeros((8, 16, 4), np.float32)
    img[..., 3] = 1.0
    img[0:4, 4:8, 0] = 3.0  # one whole 4 x 4 block
    out = ss_ref.box(img, 4)
    assert (out[..., 3] == 1.0).all()
    assert out[0, 1, 0] == 3.0 and np.count_nonzero(out[..., 0]) == 1


def test_box_refuses_ragged_frames():
    with pytest.raises(ValueError):
        ss_ref.box(np.zeros((5, 4, 4), np.float32), 2)
    with pytest.raises(ValueError):
        ss_ref.box(np.zeros((4, 4, 4), np.float32), 3)


def test_entry_points_are_exported_and_bound():
    """rt_set_samples is in the header's table with its signature; the forced general
    path is a debug export, not part of rt_api.h."""
    assert rtamd.RT_SYMBOLS["rt_set_samples"] == (C.c_int, [C.c_void_p, C.c_int])
    so = C.CDLL(os.path.join(rtamd.LIBDIR, "librtamd.so"))
    assert hasattr(so, "rt_set_samples") and hasattr(so, "rt_debug_ss_general")
    assert "rt_debug_ss_general" not in rtamd.RT_SYMBOLS
    assert callable(rtamd.ComputeShader.set_samples) and callable(rtamd.ComputeShader.debug_ss_general)


def test_null_context_is_refused():
    lib = rtamd.rt_lib()
    assert lib.rt_set_samples(None, 2) == -1  # RT_ERR_INVALID
