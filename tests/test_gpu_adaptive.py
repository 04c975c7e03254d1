"""Adaptive supersampling (rt_set_adaptive; -m gpu, needs an MI355X).

The definition under test (include/rt_api.h, restated in tests/adaptive_ref.py): with B the
frame a dispatch writes with rt_set_samples(1) and S the one it writes with rt_set_samples(n),
the adaptive frame is S at the pixels whose B contrasts with a 4-neighbour's by more than the
threshold and B elsewhere -- bit for bit against the renderer's own B and S, and within the
parity tolerance against the oracle's, with the same mask wherever the oracle's contrast is
not within 2e-4 of the threshold.

Scenes come from rtamd.generate(cfg, 0, n*W, n*H). Every float destination starts
NaN-poisoned, so a pixel left unwritten fails the comparison. B and S are rendered once per
(scene, size, settings, kernel) and shared read-only.
"""
import functools

import numpy as np
import pytest
import torch

import adaptive_ref as ar
import fmt_ref
import oracle
import rtamd
import ss_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the parity tests' own
KERNELS = [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET, rtamd.KERNEL_LANE]
KNAME = {rtamd.KERNEL_ACCEL: "accel", rtamd.KERNEL_PACKET: "packet", rtamd.KERNEL_LANE: "lane"}
RT_ERR_INVALID = -1
T16, T64, INF = 1.0 / 16.0, 1.0 / 64.0, float("inf")
PLAIN3 = (3, True, False, False)  # (maxBounces, useBVH, useFresnel, useMollerTrumbore)


def case_id(c):
    return "c%d_%dx%d_n%d_b%d_bvh%d_f%d_mt%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1], c[4][2], c[4][3])


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def defaults(ctx):
    """Every test starts from, and leaves, the context's default switches."""
    yield
    ctx.set_samples(1)
    ctx.set_adaptive(-1.0)
    ctx.debug_ss_general(0)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_latency_mode(0)
    ctx.set_tail(-1)
    ctx.set_schedule(rtamd.SCHED_COST)
    ctx.set_walk(-1)
    ctx.set_surface_format(rtamd.FORMAT_RGBA32F)


@functools.lru_cache(maxsize=None)
def scene(cfg, sw, sh):
    return rtamd.generate(cfg, 0, sw, sh)


def frozen(a):
    a.setflags(write=False)
    return a


def surface(rows, width, channels=4, fill=float("nan"), dtype=torch.float32):
    out = torch.full((rows, width, channels), fill, dtype=dtype, device="cuda")
    torch.cuda.synchronize()  # the renderer's stream does not wait on torch's
    return out


def load(ctx, cfg, W, H, n, s, kernel):
    ctx.upload(scene(cfg, n * W, n * H))
    ctx.set_params(W, H, *s)
    ctx.set_kernel(kernel)


def full_frame(ctx, W, H, n, thr=-1.0):
    """The whole W x H frame through rt_dispatch_rows with n x n samples and this threshold."""
    ctx.set_samples(n)
    ctx.set_adaptive(thr)
    out = surface(H, W)
    ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
    ctx.sync()
    return out.cpu().numpy()


_frames = {}


def frames(ctx, cfg, W, H, n, s, kernel):
    """(B, S): the renderer's own one-sample frame and its n x n frame with adaptive off, with
    the context's default switches. Leaves the scene loaded."""
    key = (cfg, W, H, n, s, kernel)
    load(ctx, cfg, W, H, n, s, kernel)
    if key not in _frames:
        B = full_frame(ctx, W, H, 1)
        S = full_frame(ctx, W, H, n)
        assert np.isfinite(B).all() and np.isfinite(S).all()
        _frames[key] = (frozen(B), frozen(S))
    return _frames[key]


def same(img, ref, what):
    assert img.shape == ref.shape, what
    assert np.array_equal(img, ref), f"{what}: {int((img != ref).any(axis=-1).sum())} pixels differ"


def composed(B, S, thr, y=None):
    m = ar.mask(B, np.arange(B.shape[0]) if y is None else y, thr)
    return ar.compose(B, S, m), m


# --------------------------------------------------------------------------
# 1. exact against the renderer's own frames
EXACT_CASES = [
    (1, 80, 60, 2, PLAIN3),
    (1, 40, 30, 4, PLAIN3),
    (1, 20, 15, 8, PLAIN3),                    # one pixel is a wave
    (2, 100, 75, 2, (1, True, False, False)),
    (2, 100, 75, 2, (4, True, True, False)),
    (3, 96, 54, 2, PLAIN3),
    (3, 64, 40, 4, PLAIN3),
    (2, 60, 45, 2, (2, True, False, True)),    # Moller-Trumbore
    (1, 80, 60, 2, (3, False, False, False)),  # the brute-force branch
    (1, 83, 61, 2, PLAIN3),                    # width no multiple of 8, the last chunk partial
]


@pytest.mark.parametrize("kernel", KERNELS, ids=KNAME.get)
@pytest.mark.parametrize("case", EXACT_CASES, ids=case_id)
def test_equals_the_composed_frames(ctx, case, kernel):
    cfg, W, H, n, s = case
    B, S = frames(ctx, cfg, W, H, n, s, kernel)
    ref, m = composed(B, S, T16)
    print(f"{case_id(case)} {KNAME[kernel]}: refined share {m.mean():.3f}")
    assert 0 < m.mean() < 1, "both branches must run"
    img = full_frame(ctx, W, H, n, T16)
    same(img, ref, "adaptive")
    assert (img[..., 3] == 1.0).all()
    assert ctx.adaptive_stats() == (int(m.sum()), W * H)
    last = ctx.accel_info()["last_kernel"]
    ctx.debug_ss_general(1)
    gen = full_frame(ctx, W, H, n, T16)
    same(gen, img, "forced general path against the dispatch's own path")
    assert ctx.adaptive_stats() == (int(m.sum()), W * H)
    assert ctx.accel_info()["last_kernel"] == last


# --------------------------------------------------------------------------
# 2. extremes
@pytest.mark.parametrize("general", [0, 1], ids=["own_path", "general"])
def test_infinite_threshold_is_the_one_sample_frame(ctx, general):
    B, S = frames(ctx, 3, 96, 54, 2, PLAIN3, rtamd.KERNEL_ACCEL)
    ctx.debug_ss_general(general)
    same(full_frame(ctx, 96, 54, 2, INF), B, "threshold inf")
    assert ctx.adaptive_stats() == (0, 96 * 54)


@pytest.mark.parametrize("general", [0, 1], ids=["own_path", "general"])
def test_threshold_below_every_contrast_is_the_full_frame(ctx, general):
    """cfg 1 at 20 x 15: the sky gradient alone moves a channel by 0.9 / 15 per row, so at
    1/64 every pixel refines."""
    B, S = frames(ctx, 1, 20, 15, 8, PLAIN3, rtamd.KERNEL_ACCEL)
    assert ar.mask(B, np.arange(15), T64).all()
    ctx.debug_ss_general(general)
    same(full_frame(ctx, 20, 15, 8, T64), S, "threshold 1/64")
    assert ctx.adaptive_stats() == (300, 300)


def test_one_sample_ignores_the_threshold(ctx):
    B, _ = frames(ctx, 3, 96, 54, 2, PLAIN3, rtamd.KERNEL_ACCEL)
    same(full_frame(ctx, 96, 54, 1, T16), B, "adaptive on with n = 1")


# --------------------------------------------------------------------------
# 3. dispatch forms and formats, cfg 3 at 96 x 54, n = 2
FW, FH, FN = 96, 54, 2


@pytest.fixture
def form(ctx, request):
    kernel = getattr(request, "param", rtamd.KERNEL_ACCEL)
    B, S = frames(ctx, 3, FW, FH, FN, PLAIN3, kernel)
    ctx.set_samples(FN)
    ctx.set_adaptive(T16)
    return B, S


BOTH = pytest.mark.parametrize("form", [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET], ids=KNAME.get, indirect=True)


@BOTH
def test_own_surface(ctx, form):
    B, S = form
    ref, m = composed(B, S, T16)
    same(ctx.render(FW, FH), ref, "rt_dispatch + rt_read_image")
    assert ctx.adaptive_stats() == (int(m.sum()), FW * FH)


def striped(B, S, y0, stripe, period, out_rows):
    """The rows a striped dispatch writes: (compact rows inside the frame, their image rows, the
    composed values); neighbours are those of the dispatch, not of the whole frame."""
    ys = ar.rows_of(FH, y0, stripe, period, out_rows)
    own = np.flatnonzero(ys < FH)
    y = ys[own]
    ref, m = composed(B[y], S[y], T16, y)
    return own, y, ref, m


@BOTH
def test_striped_rows_running_past_the_frame(ctx, form):
    """rt_dispatch_rows with y0 = stripe = 4, step = 3: image rows 4..7, 16..19, 28..31, 40..43,
    52..53; of 24 compact rows the last six lie below the frame and stay NaN. A stripe's first
    and last rows have no neighbour across the gap."""
    B, S = form
    own, y, ref, m = striped(B, S, 4, 4, 12, 24)
    assert len(own) == 18 and 0 < m.mean() < 1
    whole = ar.mask(B, np.arange(FH), T16)[y]
    assert (whole != m).any(), "the case must tell the stripe rule from the whole frame's"
    out = surface(24, FW)
    ctx.dispatch_rows(FW, FH, 4, 4, 3, 24, out.data_ptr(), FW * 16)
    ctx.sync()
    got = out.cpu().numpy()
    same(got[own], ref, "striped")
    assert np.isnan(got[len(own):]).all()
    assert ctx.adaptive_stats() == (int(m.sum()), 18 * FW)


@BOTH
def test_rows_ex_rgb32f_and_image_rows(ctx, form):
    """rt_dispatch_rows_ex with period > stripe (y0 = 3, stripe = 5, period = 7), as RGBA32F,
    RGB32F and at the image rows of a whole surface."""
    B, S = form
    own, y, ref, m = striped(B, S, 3, 5, 7, 30)
    assert 0 < m.mean() < 1
    for fmt, ch in [(rtamd.FORMAT_RGBA32F, 4), (rtamd.FORMAT_RGB32F, 3)]:
        out = surface(30, FW, ch)
        ctx.dispatch_rows_ex(FW, FH, 3, 5, 7, 30, out.data_ptr(), FW * 4 * ch, fmt=fmt)
        ctx.sync()
        got = out.cpu().numpy()
        same(got[own], ref[..., :ch], f"format {fmt}")
        assert np.isnan(got[np.setdiff1d(np.arange(30), own)]).all()
    out = surface(FH, FW)
    ctx.dispatch_rows_ex(FW, FH, 3, 5, 7, 30, out.data_ptr(), FW * 16, fmt=rtamd.FORMAT_RGBA32F_IMAGE)
    ctx.sync()
    got = out.cpu().numpy()
    same(got[y], ref, "image rows")
    assert np.isnan(got[np.setdiff1d(np.arange(FH), y)]).all()


@BOTH
@pytest.mark.parametrize("fmt", [rtamd.FORMAT_RGBA8, rtamd.FORMAT_SRGBA8, rtamd.FORMAT_RGBA16F])
def test_display_formats(ctx, form, fmt):
    B, S = form
    ref, _ = composed(B, S, T16)
    want = fmt_ref.convert(ref, fmt, rtamd.srgb_thresholds())
    dt = {np.uint8: torch.uint8, np.float16: torch.float16}[fmt_ref.DTYPE[fmt]]
    out = surface(FH, FW, 4, 7, dt)
    ctx.dispatch_rows_ex(FW, FH, 0, FH, FH, FH, out.data_ptr(), FW * fmt_ref.BYTES[fmt], fmt=fmt)
    ctx.sync()
    got = out.cpu().numpy()
    assert got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # the context surface in the same format
    got = ctx.render(FW, FH, fmt=fmt)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), want.view(np.uint8))


# --------------------------------------------------------------------------
# 4. against the oracle
@functools.lru_cache(maxsize=None)
def oracle_frames(cfg, W, H, n, s):
    fs = scene(cfg, n * W, n * H)
    one, _ = oracle.render(fs, W, H, oracle.params(W, H, *s))
    big, _ = oracle.render(fs, n * W, n * H, oracle.params(n * W, n * H, *s))
    return frozen(one), frozen(ss_ref.box(big, n))


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_ACCEL, rtamd.KERNEL_LANE], ids=KNAME.get)
@pytest.mark.parametrize("case", ar.ORACLE_CASES, ids=case_id)
def test_against_the_oracle(ctx, case, kernel):
    cfg, W, H, n, s = case
    Bo, So = oracle_frames(cfg, W, H, n, s)
    y = np.arange(H)
    mo = ar.mask(Bo, y, ar.THRESHOLD)
    ref = ar.compose(Bo, So, mo)
    out = ar.near(Bo, y, ar.THRESHOLD)
    B, _ = frames(ctx, cfg, W, H, n, s, kernel)
    img = full_frame(ctx, W, H, n, float(ar.THRESHOLD))
    mg = ar.mask(B, y, ar.THRESHOLD)  # the renderer's mask (test_equals_the_composed_frames)
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64))[~out]
    print(f"{case_id(case)} {KNAME[kernel]}: left out {int(out.sum())} pixels, "
          f"max |gpu - oracle| = {diff.max():.3g}, masks differ at {int((mg != mo)[~out].sum())}")
    assert out.mean() <= ar.NEAR_CAP
    assert np.array_equal(mg[~out], mo[~out])
    assert ctx.adaptive_stats()[0] == int(mg.sum())
    assert diff.max() <= TOL


# --------------------------------------------------------------------------
# 5. settings that must not change the image
def _latency(ctx):
    ctx.set_latency_mode(1)
    return 3  # the cost order exists from the second frame on


def _rows(ctx):
    ctx.set_schedule(rtamd.SCHED_ROWS)
    return 2


def _walk(depth):
    def run(ctx):
        ctx.set_walk(depth)
        return 1
    return run


def _tail(ctx):
    ctx.set_tail(1)
    return 2


SWITCHES = {"latency": _latency, "sched_rows": _rows, "walk0": _walk(0), "walk9": _walk(9), "tail1": _tail}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_switches_do_not_change_the_frame(ctx, switch):
    B, S = frames(ctx, 3, FW, FH, FN, PLAIN3, rtamd.KERNEL_ACCEL)
    ref, m = composed(B, S, T16)
    for k in range(SWITCHES[switch](ctx)):
        same(full_frame(ctx, FW, FH, FN, T16), ref, f"{switch} frame {k}")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
        assert ctx.adaptive_stats() == (int(m.sum()), FW * FH)


# --------------------------------------------------------------------------
# 6. stream order
@pytest.mark.parametrize("general", [0, 1], ids=["own_path", "general"])
def test_dispatches_in_flight_and_a_new_size(ctx, general):
    """Three adaptive dispatches without a sync in between, three thresholds, three surfaces:
    a refined-pixel counter that was not reset in stream order shows in the second or third.
    Then a frame of another size, which reallocates the context's buffers."""
    B, S = frames(ctx, 1, 20, 15, 8, PLAIN3, rtamd.KERNEL_ACCEL)
    ctx.set_samples(8)
    ctx.debug_ss_general(general)
    outs = [surface(15, 20) for _ in range(3)]
    for thr, out in zip((T16, INF, T64), outs):
        ctx.set_adaptive(thr)
        ctx.dispatch_rows(20, 15, 0, 1, 1, 15, out.data_ptr(), 20 * 16)
    ctx.sync()
    for thr, out in zip((T16, INF, T64), outs):
        same(out.cpu().numpy(), composed(B, S, thr)[0], f"threshold {thr} in flight")
    assert ctx.adaptive_stats() == (300, 300)
    B, S = frames(ctx, 1, 40, 30, 4, PLAIN3, rtamd.KERNEL_ACCEL)
    ref, m = composed(B, S, T16)
    same(full_frame(ctx, 40, 30, 4, T16), ref, "after a change of size")
    assert ctx.adaptive_stats() == (int(m.sum()), 1200)


# --------------------------------------------------------------------------
# 7. errors
def test_nan_threshold_is_refused_and_the_setting_stays(ctx):
    B, S = frames(ctx, 3, FW, FH, FN, PLAIN3, rtamd.KERNEL_ACCEL)
    ctx.set_adaptive(T16)
    with pytest.raises(rtamd.RTError) as e:
        ctx.set_adaptive(float("nan"))
    assert e.value.code == RT_ERR_INVALID
    ctx.set_samples(FN)
    out = surface(FH, FW)
    ctx.dispatch_rows(FW, FH, 0, 1, 1, FH, out.data_ptr(), FW * 16)
    ctx.sync()
    same(out.cpu().numpy(), composed(B, S, T16)[0], "the threshold set before the refusal")


def test_stats_without_an_adaptive_dispatch_are_refused():
    fresh = rtamd.ComputeShader(0)
    try:
        with pytest.raises(rtamd.RTError) as e:
            fresh.adaptive_stats()
        assert e.value.code == RT_ERR_INVALID
        fresh.upload(scene(1, 40, 30))
        fresh.set_params(20, 15, *PLAIN3)
        fresh.set_samples(2)
        fresh.render(20, 15)  # supersampled, adaptive off
        with pytest.raises(rtamd.RTError) as e:
            fresh.adaptive_stats()
        assert e.value.code == RT_ERR_INVALID
    finally:
        fresh.close()
