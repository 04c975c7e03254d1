"""Display formats (RT_FORMAT_RGBA8 / SRGBA8 / RGBA16F; -m gpu, needs an MI355X).

The definition under test (include/rt_api.h): a frame in a display format is the
per-channel conversion, restated in tests/fmt_ref.py, of the float32 RGBA frame of the
same dispatch. So the reference of every comparison is fmt_ref.convert applied to the
renderer's own RGBA32F frame: same context, kernel and settings, rendered first (frames
are deterministic; the float frame's parity with the oracle is the other suites' subject).
8-bit frames are compared exactly, half frames bit for bit (NaN against NaN).

Every destination starts as 0xA5 bytes and is a few bytes wider than its rows, so a pixel
left unwritten, written twice as wide, or written past its row shows.
"""
import functools

import numpy as np
import pytest
import torch

import fmt_ref
import rtamd

pytestmark = pytest.mark.gpu
RT_ERR_INVALID = -1
POISON = 0xA5
PAD = 8  # poisoned bytes after each row (keeps every format's pitch alignment)
FORMATS = [rtamd.FORMAT_RGBA8, rtamd.FORMAT_SRGBA8, rtamd.FORMAT_RGBA16F]
FNAME = {rtamd.FORMAT_RGBA8: "rgba8", rtamd.FORMAT_SRGBA8: "srgba8", rtamd.FORMAT_RGBA16F: "rgba16f"}
KERNELS = [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET, rtamd.KERNEL_LANE]
KNAME = {rtamd.KERNEL_ACCEL: "accel", rtamd.KERNEL_PACKET: "packet", rtamd.KERNEL_LANE: "lane"}
# (maxBounces, useBVH, useFresnel, useMollerTrumbore)
SET = {2: (1, True, False, False), 3: (3, True, False, False)}
# config 2 (monkey, 1 bounce) at 70 x 37: neither a multiple of 8 nor of 4, so partial tiles in
# both directions and row pitches that are no multiple of 16; config 3 (car, 3 bounces) at
# 96 x 56: large enough for the tail and heavy-tile paths. The third number scales the light.
MONKEY, MONKEY_X4, CAR = (2, 70, 37, 1), (2, 70, 37, 4), (3, 96, 56, 1)
CNAME = {MONKEY: "monkey", MONKEY_X4: "monkey_light_x4", CAR: "car"}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T():
    t = rtamd.srgb_thresholds()
    t.setflags(write=False)
    return t


@pytest.fixture(autouse=True)
def defaults(ctx):
    """Every test starts from, and leaves, the context's default switches."""
    yield
    ctx.set_samples(1)
    ctx.debug_ss_general(0)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_latency_mode(0)
    ctx.debug_heavy(-1, 4)
    ctx.set_tail(-1)
    ctx.debug_tail_lanes(64)
    ctx.set_surface_format(rtamd.FORMAT_RGBA32F)


@functools.lru_cache(maxsize=None)
def scene(case):
    cfg, W, H, light = case
    fs = rtamd.generate(cfg, 0, W, H)
    if light != 1:
        fs.light["color"] = fs.light["color"] * np.float32(light)
    return fs


def load(ctx, case, s=None, kernel=rtamd.KERNEL_ACCEL):
    cfg, W, H, _ = case
    ctx.upload(scene(case))
    ctx.set_params(W, H, *(s or SET[cfg]))
    ctx.set_kernel(kernel)
    return W, H


def poisoned(rows, row_bytes):
    out = torch.full((rows, row_bytes + PAD), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the renderer's stream does not wait on torch's
    return out


def decode(buf, W, fmt):
    """(rows, pitch) uint8 -> (rows, W, 4) in the format's type; the bytes after each row
    must still be poison."""
    raw = buf.cpu().numpy()
    used = W * fmt_ref.BYTES[fmt]
    assert (raw[:, used:] == POISON).all(), "bytes past a row's end were written"
    return np.ascontiguousarray(raw[:, :used]).view(fmt_ref.DTYPE[fmt]).reshape(raw.shape[0], W, 4)


def rows_frame(ctx, W, H, fmt, y0=0, stripe=1, period=1, out_rows=None):
    """One dispatch through rt_dispatch_rows_ex into a poisoned surface of format fmt."""
    rows = H if out_rows is None else out_rows
    if fmt == rtamd.FORMAT_RGBA32F:
        out = torch.full((rows, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.dispatch_rows_ex(W, H, y0, stripe, period, rows, out.data_ptr(), W * 16, fmt=fmt)
        ctx.sync()
        return out.cpu().numpy()
    out = poisoned(rows, W * fmt_ref.BYTES[fmt])
    ctx.dispatch_rows_ex(W, H, y0, stripe, period, rows, out.data_ptr(), out.shape[1], fmt=fmt)
    ctx.sync()
    return decode(out, W, fmt)


def float_frame(ctx, W, H):
    img = rows_frame(ctx, W, H, rtamd.FORMAT_RGBA32F)
    assert np.isfinite(img).all(), "the float frame has an unwritten pixel"
    assert (img[..., 3] == 1.0).all()
    return img


def same(got, ref, fmt, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if fmt == rtamd.FORMAT_RGBA16F:
        g, r = got.view(np.uint16), ref.view(np.uint16)
        nan = np.isnan(ref)
        ok = np.where(nan, np.isnan(got), g == r)
    else:
        ok = got == ref
    bad = int((~ok).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} of {ok.shape[0] * ok.shape[1]} pixels differ from fmt_ref of the float frame"


def check_formats(ctx, T, W, H, ref32, what, formats=FORMATS):
    for fmt in formats:
        same(rows_frame(ctx, W, H, fmt), fmt_ref.convert(ref32, fmt, T), fmt, f"{what} {FNAME[fmt]}")


# --------------------------------------------------------------------------
# 1. full frames, every kernel
@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
@pytest.mark.parametrize("kernel", KERNELS, ids=KNAME.get)
@pytest.mark.parametrize("case", [MONKEY, MONKEY_X4, CAR], ids=CNAME.get)
def test_full_frame(ctx, T, case, kernel, fmt):
    W, H = load(ctx, case, kernel=kernel)
    ref32 = float_frame(ctx, W, H)
    if case == MONKEY_X4:
        rgb = ref32[..., :3]
        print(f"light x4: {int((rgb > 1).sum())} channels above 1, {int(((rgb > 0) & (rgb < 1)).sum())} inside (0, 1)")
        assert (rgb > 1).any(), "no channel above 1: the clamp is not exercised"
        assert ((rgb > 0) & (rgb < 1)).any(), "no channel strictly inside (0, 1)"
    got = rows_frame(ctx, W, H, fmt)
    same(got, fmt_ref.convert(ref32, fmt, T), fmt, f"{CNAME[case]} {KNAME[kernel]} {FNAME[fmt]}")
    want_kernel = kernel
    assert ctx.accel_info()["last_kernel"] == want_kernel


# --------------------------------------------------------------------------
# 2. a striped mapping whose last rows lie below the frame
@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
@pytest.mark.parametrize("kernel", [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET], ids=KNAME.get)
def test_stripes(ctx, T, kernel, fmt):
    """y0 = 3, stripe = 5, period = 13: compact row r is image row 3 + (r / 5) * 13 + r % 5,
    i.e. rows 3..7, 16..20, 29..33 and 42..46; the last five of 20 lie below the 37-row frame."""
    W, H = load(ctx, MONKEY_X4, kernel=kernel)
    ref = fmt_ref.convert(float_frame(ctx, W, H), fmt, T)
    out_rows = 20
    ys = [3 + (r // 5) * 13 + r % 5 for r in range(out_rows)]
    assert sum(y >= H for y in ys) == 5
    out = poisoned(out_rows, W * fmt_ref.BYTES[fmt])
    ctx.dispatch_rows_ex(W, H, 3, 5, 13, out_rows, out.data_ptr(), out.shape[1], fmt=fmt)
    ctx.sync()
    got = decode(out, W, fmt)
    raw = out.cpu().numpy()
    for r, y in enumerate(ys):
        if y < H:
            same(got[r:r + 1], ref[y:y + 1], fmt, f"{FNAME[fmt]} row {r} (image row {y})")
        else:
            assert (raw[r] == POISON).all(), f"{FNAME[fmt]} row {r} lies below the frame"
    # rt_dispatch_rows_fmt (period = stripe * step) takes the formats too
    out = poisoned(10, W * fmt_ref.BYTES[fmt])
    rc = ctx._lib.rt_dispatch_rows_fmt(ctx._h, W, H, 5, 5, 3, 10, out.data_ptr(), out.shape[1], fmt)
    assert rc == 0
    ctx.sync()
    got = decode(out, W, fmt)
    for r, y in enumerate([5, 6, 7, 8, 9, 20, 21, 22, 23, 24]):
        same(got[r:r + 1], ref[y:y + 1], fmt, f"{FNAME[fmt]} rows_fmt row {r}")


# --------------------------------------------------------------------------
# 3. rt_set_samples: the in-kernel store and the render-then-filter path
@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
@pytest.mark.parametrize("general", [0, 1], ids=["fused", "filter_kernel"])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("case", [MONKEY_X4, CAR], ids=CNAME.get)
def test_supersampled(ctx, T, case, n, general, fmt):
    W, H = load(ctx, case)
    ctx.set_samples(n)
    ctx.debug_ss_general(general)
    ref32 = float_frame(ctx, W, H)
    same(rows_frame(ctx, W, H, fmt), fmt_ref.convert(ref32, fmt, T), fmt,
         f"{CNAME[case]} n={n} general={general} {FNAME[fmt]}")
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL


@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
def test_supersampled_packet_kernel_with_stripes(ctx, T, fmt):
    """The filter kernel's own row mapping and bounds: packet kernel, stripes, rows below the frame."""
    W, H = load(ctx, MONKEY_X4, kernel=rtamd.KERNEL_PACKET)
    ctx.set_samples(2)
    ref = fmt_ref.convert(float_frame(ctx, W, H), fmt, T)
    out = poisoned(20, W * fmt_ref.BYTES[fmt])
    ctx.dispatch_rows_ex(W, H, 3, 5, 13, 20, out.data_ptr(), out.shape[1], fmt=fmt)
    ctx.sync()
    got, raw = decode(out, W, fmt), out.cpu().numpy()
    for r in range(20):
        y = 3 + (r // 5) * 13 + r % 5
        if y < H:
            same(got[r:r + 1], ref[y:y + 1], fmt, f"{FNAME[fmt]} row {r} (image row {y})")
        else:
            assert (raw[r] == POISON).all(), f"{FNAME[fmt]} row {r} lies below the frame"


# --------------------------------------------------------------------------
# 4. the accelerated kernel's other instances: latency mode, heavy tiles, the tail kernel
def _latency(ctx, render):
    ctx.set_latency_mode(1)
    return [render() for _ in range(3)]


def _heavy(ctx, render):
    # as tests/test_gpu_supersample.py: the cost order exists from the second frame on; latency
    # mode splits on the frames that record no cost, the default mode on those that do
    ctx.set_latency_mode(1)
    ctx.debug_heavy(10 ** 6, 4)
    frames = [render() for _ in range(3)]
    ctx.set_latency_mode(0)
    ctx.debug_heavy(7, 4)
    return frames + [render() for _ in range(2)]


def _tail(ctx, render):
    ctx.set_tail(2)
    ctx.debug_tail_lanes(24)  # some waves queue their rays for k_accel_tail, others keep them
    frames = [render(), render()]
    ctx.debug_tail_lanes(64)  # every wave queues
    return frames + [render(), render()]


SWITCHES = {"latency": _latency, "heavy": _heavy, "tail": _tail}


@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_accel_instances(ctx, T, switch, fmt):
    W, H = load(ctx, CAR)
    ref32 = float_frame(ctx, W, H)
    # the float frame under the same switches is the same frame
    for k, img in enumerate(SWITCHES[switch](ctx, lambda: rows_frame(ctx, W, H, rtamd.FORMAT_RGBA32F))):
        assert np.array_equal(img, ref32), f"{switch}: float frame {k} moved"
    ref = fmt_ref.convert(ref32, fmt, T)
    ctx.set_latency_mode(0)
    ctx.debug_heavy(-1, 4)
    for k, img in enumerate(SWITCHES[switch](ctx, lambda: rows_frame(ctx, W, H, fmt))):
        same(img, ref, fmt, f"{switch} {FNAME[fmt]} frame {k}")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL


# --------------------------------------------------------------------------
# 5. the sub-contexts inherit the format
@pytest.mark.parametrize("s,fmt", [((3, False, False, False), rtamd.FORMAT_RGBA8),
                                   ((3, True, True, False), rtamd.FORMAT_SRGBA8),
                                   ((3, True, False, True), rtamd.FORMAT_SRGBA8),
                                   ((3, False, False, True), rtamd.FORMAT_RGBA8)],
                         ids=["brute_rgba8", "fresnel_srgba8", "moller_trumbore_srgba8", "brute_mt_rgba8"])
def test_uniforms(ctx, T, s, fmt):
    W, H = load(ctx, CAR, s=s)
    ref32 = float_frame(ctx, W, H)
    for k in range(2):
        same(rows_frame(ctx, W, H, fmt), fmt_ref.convert(ref32, fmt, T), fmt, f"settings {s} frame {k}")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL


# --------------------------------------------------------------------------
# 6. the context's own surface
def test_own_surface(ctx, T):
    W, H = load(ctx, MONKEY_X4)
    assert ctx.surface_format() == rtamd.FORMAT_RGBA32F
    ref32 = ctx.render(W, H)
    for fmt in FORMATS:
        ctx.set_surface_format(fmt)
        assert ctx.surface_format() == fmt
        ctx.dispatch(W, H)
        ctx.sync()
        got = ctx.read_surface(W, H)
        assert got.dtype == fmt_ref.DTYPE[fmt] and got.shape == (H, W, 4)
        same(got, fmt_ref.convert(ref32, fmt, T), fmt, f"own surface {FNAME[fmt]}")
        ptr, pitch = ctx.device_image()
        bpp = fmt_ref.BYTES[fmt]
        assert ptr and pitch >= W * bpp and pitch % bpp == 0
        # rt_read_image is the float surface's
        with pytest.raises(rtamd.RTError) as e:
            ctx.read_image(W, H)
        assert e.value.code == RT_ERR_INVALID
        # a short pitch, or another size, is refused and writes nothing
        host = np.full((H, W * bpp), POISON, np.uint8)
        lib, h = ctx._lib, ctx._h
        assert lib.rt_read_surface(h, host.ctypes.data, W * bpp - bpp, W, H) == RT_ERR_INVALID
        assert lib.rt_read_surface(h, host.ctypes.data, W * bpp, W, H - 1) == RT_ERR_INVALID
        assert lib.rt_read_surface(h, host.ctypes.data, W * bpp, W + 1, H) == RT_ERR_INVALID
        assert lib.rt_read_surface(h, None, W * bpp, W, H) == RT_ERR_INVALID
        assert (host == POISON).all()
        # render(fmt=) is the same frame
        same(ctx.render(W, H, fmt=fmt), got, fmt, f"render(fmt={FNAME[fmt]})")
    # a band of the surface: the rows outside it keep the previous frame
    ctx.dispatch(W, H, 8, 16)
    ctx.sync()
    same(ctx.read_surface(W, H), got, FORMATS[-1], "a band re-rendered")
    # back to float: the format applies at the next dispatch, and rt_read_image works again
    ctx.set_surface_format(rtamd.FORMAT_RGBA32F)
    assert ctx.surface_format() == rtamd.FORMAT_RGBA32F
    img = ctx.render(W, H)
    assert img.dtype == np.float32 and np.array_equal(img, ref32)
    assert np.array_equal(ctx.read_surface(W, H), ref32)


def test_own_surface_supersampled(ctx, T):
    W, H = load(ctx, CAR)
    ctx.set_samples(2)
    ref32 = ctx.render(W, H)
    got = ctx.render(W, H, fmt=rtamd.FORMAT_SRGBA8)
    same(got, fmt_ref.convert(ref32, rtamd.FORMAT_SRGBA8, T), rtamd.FORMAT_SRGBA8, "own surface, 2 x 2 samples")


# --------------------------------------------------------------------------
# 7. the conversion on values no frame holds
@functools.lru_cache(maxsize=None)
def special_values():
    """(343, 1024, 4) float32 pixels whose R, G, B hold: the hand-made vector of tests/test_formats_cpu.py, every sRGB
    threshold with both neighbours, the 8-bit grid with its ties and their neighbours, the
    half format's edges, uniform values in [0, 1) and 2^19 random bit patterns (NaNs of both
    kinds, infinities, subnormals, huge and negative values among them)."""
    T = rtamd.srgb_thresholds()
    one, zero = np.float32(1), np.float32(0)
    k = np.arange(0, 256, dtype=np.float32)
    grid = np.concatenate([k / np.float32(255), (k + np.float32(0.5)) / np.float32(255)])
    half_edges = np.float32([65504, 65519.99, 65520, 65536, 1e-8, 2.0 ** -24, 2.0 ** -25, 2.9802325e-08, 2.0 ** -14,
                             6.1e-5, 1.0009766, 1.0004883, 1.0014648, -65520, 3.4e38, -3.4e38])
    parts = [np.float32([0, 1, -1, 2, np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 65504, 65520, 1e-8, -0.0]),
             T, np.nextafter(T, zero), np.nextafter(T, one),
             grid, np.nextafter(grid, zero), np.nextafter(grid, one), half_edges,
             np.float32([0.0031308, 0.0031309, 0.0031307, 0.04045 / 12.92])]
    rng = np.random.default_rng(20261020)
    parts.append(rng.random(1 << 19, dtype=np.float32))
    parts.append(rng.integers(0, 1 << 32, 1 << 19, dtype=np.uint64).astype(np.uint32).view(np.float32))
    v = np.concatenate([p.astype(np.float32) for p in parts])
    # three values to a pixel (R, G, B; alpha is not converted), rows of 1024 pixels
    W = 1024
    rows = -(-v.size // (3 * W))
    rgb = np.full(rows * W * 3, 0.5, np.float32)
    rgb[:v.size] = v
    out = np.ones((rows, W, 4), np.float32)
    out[..., :3] = rgb.reshape(rows, W, 3)
    out[..., 3] = np.resize(v, rows * W).reshape(rows, W)  # anything: the stored alpha is fixed
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
def test_conversion_of_special_values(ctx, T, fmt):
    """store_display, the one conversion every kernel's store calls, through the filter kernel's
    instance of it (rt_debug_convert) on caller data. Alpha is not converted: it is the fixed
    255 / 0x3C00 whatever the source holds."""
    vals = special_values()
    rows, W, _ = vals.shape
    src = torch.from_numpy(np.array(vals)).cuda()
    out = poisoned(rows, W * fmt_ref.BYTES[fmt])
    torch.cuda.synchronize()
    ctx.debug_convert(src.data_ptr(), W * 16, out.data_ptr(), out.shape[1], W, rows, fmt)
    ctx.sync()
    got = decode(out, W, fmt)
    ref = fmt_ref.convert(vals, fmt, T)
    if fmt == rtamd.FORMAT_RGBA16F:
        ok = np.where(np.isnan(ref), np.isnan(got), got.view(np.uint16) == ref.view(np.uint16))
    else:
        ok = got == ref
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (f"{len(bad)} of {ok.size} values differ; first: source "
                           f"{vals[tuple(bad[0])]!r} (bits {vals.view(np.uint32)[tuple(bad[0])]:#010x}) -> "
                           f"{got[tuple(bad[0])]!r}, expected {ref[tuple(bad[0])]!r}")


# --------------------------------------------------------------------------
# 8. refusals: RT_ERR_INVALID before anything is launched
@pytest.mark.parametrize("fmt", FORMATS, ids=FNAME.get)
def test_misaligned_or_short_destinations_are_refused(ctx, fmt):
    W, H = load(ctx, MONKEY)
    bpp = fmt_ref.BYTES[fmt]
    out = poisoned(H + 1, W * bpp + 16)
    base, pitch = out.data_ptr(), out.shape[1]
    assert base % 8 == 0 and pitch % 8 == 0
    bad = [("dst off by half its alignment", base + bpp // 2, pitch),
           ("dst off by one byte", base + 1, pitch),
           ("pitch off by half its alignment", base, pitch - bpp // 2),
           ("pitch one pixel short", base, (W - 1) * bpp),
           ("null dst", 0, pitch)]
    for what, ptr, p in bad:
        with pytest.raises(rtamd.RTError) as e:
            ctx.dispatch_rows_ex(W, H, 0, 1, 1, H, ptr, p, fmt=fmt)
        assert e.value.code == RT_ERR_INVALID, what
    ctx.sync()
    assert bool((out == POISON).all()), "a refused dispatch wrote to its destination"
    # the smallest valid pitch is accepted
    ctx.dispatch_rows_ex(W, H, 0, 1, 1, H, base, W * bpp, fmt=fmt)
    ctx.sync()
    raw = out.cpu().numpy().reshape(-1)
    assert (raw[:H * W * bpp] != POISON).any() and (raw[H * W * bpp:] == POISON).all()


@pytest.mark.parametrize("fmt", [6, 7, 255, -1, 1 << 20])
def test_unknown_formats_are_refused(ctx, fmt):
    W, H = load(ctx, MONKEY)
    out = poisoned(H, W * 16)
    with pytest.raises(rtamd.RTError) as e:
        ctx.dispatch_rows_ex(W, H, 0, 1, 1, H, out.data_ptr(), W * 16, fmt=fmt)
    assert e.value.code == RT_ERR_INVALID
    ctx.sync()
    assert bool((out == POISON).all())
    with pytest.raises(rtamd.RTError) as e:
        ctx.set_surface_format(fmt)
    assert e.value.code == RT_ERR_INVALID


@pytest.mark.parametrize("fmt", [rtamd.FORMAT_RGB32F, rtamd.FORMAT_RGBA32F_IMAGE], ids=["rgb32f", "rgba32f_image"])
def test_surface_formats_that_are_no_surface_formats(ctx, fmt):
    with pytest.raises(rtamd.RTError) as e:
        ctx.set_surface_format(fmt)
    assert e.value.code == RT_ERR_INVALID
    assert ctx.surface_format() == rtamd.FORMAT_RGBA32F
