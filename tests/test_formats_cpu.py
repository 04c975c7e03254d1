"""The display formats' definitions without a GPU: the exported sRGB threshold table
(rt_srgb_thresholds) against the float64 formula, and tests/fmt_ref.py, the numpy
restatement the GPU tests compare frames with, on hand-made values."""
import os
import sys

import numpy as np
import pytest

import fmt_ref
import rtamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    t = rtamd.srgb_thresholds()
    t.setflags(write=False)
    return t


def eotf64(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def test_thresholds_are_255_increasing_values_inside_0_1(T):
    assert T.dtype == np.float32 and T.shape == (255,)
    assert (np.diff(T) > 0).all()
    assert T[0] > 0 and T[-1] < 1


def test_thresholds_match_the_float64_formula_within_one_ulp(T):
    """One float32 ulp allows for pow differing between math libraries."""
    k = np.arange(1, 256, dtype=np.float64)
    want = eotf64((k - 0.5) / 255.0)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(T.astype(np.float64) - want)
    print(f"max |T - formula| = {(err / ulp).max():.3f} ulp")
    assert (err <= ulp).all()


def test_each_threshold_starts_its_code(T):
    k = np.arange(1, 256)
    assert np.array_equal(fmt_ref.srgb8(T, T), k)
    assert np.array_equal(fmt_ref.srgb8(np.nextafter(T, np.float32(0)), T), k - 1)


def test_the_generator_reproduces_the_committed_header(T):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_srgb_table as gen
    finally:
        sys.path.pop(0)
    # within one ulp, not bit for bit: this machine's pow need not be the one the header was made with
    g = gen.thresholds()
    assert (np.abs(g.astype(np.float64) - T.astype(np.float64)) <= np.spacing(T)).all()
    # the committed header in the generator's layout holds exactly the library's table
    with open(gen.HEADER) as f:
        text = f.read()
    assert text == gen.render(T), "csrc/srgb_table.h is not the generator's rendering of the exported table"


def test_null_destination_is_refused():
    assert rtamd.rt_lib().rt_srgb_thresholds(None) == -1


# 0.5/255 times 255 is exactly 0.5 in float32, the tie that rounds to the even 0; 1.5/255 lands
# on or beside the tie 1.5 (even: 2), so its code is rint of the float32 product, stated below.
VEC = np.float32([0.0, 1.0, -1.0, 2.0, np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 65504.0, 65520.0, 1e-8])


def test_rgba8_on_the_hand_made_vector():
    got = fmt_ref.unorm8(VEC)
    tie0 = int(np.rint(np.float32(0.5 / 255) * np.float32(255)))
    tie1 = int(np.rint(np.float32(1.5 / 255) * np.float32(255)))
    assert np.float32(0.5 / 255) * np.float32(255) == np.float32(0.5), "the tie is exact in float32"
    assert tie0 == 0, "0.5 rounds to the even 0"
    assert tie1 in (1, 2)
    assert got.tolist() == [0, 255, 0, 255, 0, 255, 0, tie0, tie1, 255, 255, 0]
    assert got.dtype == np.uint8


def test_srgba8_on_the_hand_made_vector(T):
    got = fmt_ref.srgb8(VEC, T)
    # 0.5/255 and 1.5/255 are linear-light values here: their codes come from the table
    c0 = int((T <= np.float32(0.5 / 255)).sum())
    c1 = int((T <= np.float32(1.5 / 255)).sum())
    assert got.tolist() == [0, 255, 0, 255, 0, 255, 0, c0, c1, 255, 255, 0]
    # 0.5/255 is on the linear segment: 12.92 * 0.5 = 6.46 -> 6; 1.5/255 on the power segment:
    # 255 * (1.055 * (1.5/255)^(1/2.4) - 0.055) = 17.63 -> 18
    assert (c0, c1) == (6, 18)
    # the middle of the range: linear 0.5 has the sRGB code 188
    assert int(fmt_ref.srgb8(np.float32(0.5), T)) == 188


def test_rgba16f_on_the_hand_made_vector():
    got = fmt_ref.half(VEC)
    bits = got.view(np.uint16)
    assert bits[0] == 0x0000 and bits[1] == 0x3C00 and bits[2] == 0xBC00 and bits[3] == 0x4000
    assert np.isnan(got[4]) and bits[5] == 0x7C00 and bits[6] == 0xFC00
    assert bits[9] == 0x7BFF, "65504 is the largest half"
    assert bits[10] == 0x7C00, "65520 is the tie between 65504 and 2^16: to even, which overflows to inf"
    assert bits[11] == 0x0000, "1e-8 lies below half the smallest subnormal half (2^-25)"
    sub = fmt_ref.half(np.float32([2.0 ** -24, 1e-7, 6.1e-5]))
    assert sub.view(np.uint16).tolist() == [0x0001, 0x0002, 0x03FF], "subnormal halves are kept"


def test_convert_packs_alpha_and_order(T):
    px = np.float32([[0.25, 2.0, np.nan, 1.0]])
    assert fmt_ref.convert(px, fmt_ref.RGBA8).tolist() == [[64, 255, 0, 255]]
    assert fmt_ref.convert(px, fmt_ref.SRGBA8, T).tolist() == [[137, 255, 0, 255]]
    h = fmt_ref.convert(px, fmt_ref.RGBA16F)
    assert h.view(np.uint16)[0, [0, 1, 3]].tolist() == [0x3400, 0x4000, 0x3C00] and np.isnan(h[0, 2])
    # little-endian dword R | G<<8 | B<<16 | A<<24
    assert fmt_ref.convert(px, fmt_ref.RGBA8).view("<u4")[0, 0] == 64 | 255 << 8 | 0 << 16 | 255 << 24
