"""Area lights on the device (rt_set_soft_shadows): frames of one and three lights with K shadow
rays per area light against tests/soft_ref.py's numpy restatement (anchored to
tests/lights_ref.py by tests/test_soft_cpu.py); the frame kernel, the list kernel, the literal
loop and the reference tree write the same bytes; radii too small to matter give the hard frame,
radii that touch no light of the set give today's kernels and bytes; row mapping, formats and
edges; samples and adaptive samples; pending scene writes; the calls that must not see the
radii; arguments.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adaptive_ref as ar
import fmt_ref
import gbuffer_ref as gr
import lights_ref as lr
import rtamd
import shade_ref as sr
import soft_ref as sf
import ss_ref
import trace_rays as tr
from test_gpu_lights import BYTES, FILL, as_rgba, bits, device_shade, frame, near_reference, rows_frame

pytestmark = pytest.mark.gpu
W0, H0 = gr.W0, gr.H0
MIXED = (2.0, 0.0, 0.5)  # an area light, a point light, a smaller area light
# (lights, radii): one area light; the mixed set of three
SETS = {1: (2.0,), 3: MIXED}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def defaults(ctx):
    """Every test leaves the context's default switches."""
    yield
    ctx.set_soft_shadows(None)
    ctx.set_samples(1)
    ctx.set_adaptive(-1.0)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_tree(rtamd.TREE_SCENE)
    ctx.set_animated(np.zeros(0, np.int32))


def prepare(ctx, fs, mt=False, W=W0, H=H0, kernel=rtamd.KERNEL_AUTO, tree=rtamd.TREE_SCENE, bounces=3, bvh=True,
            fresnel=False, lights=None, radii=None, K=16):
    ctx.upload(fs)  # sets the scene's own light: one light
    ctx.set_animated(np.zeros(0, np.int32))
    ctx.set_params(W, H, bounces, bvh, fresnel, mt)
    ctx.set_kernel(kernel)
    ctx.set_tree(tree)
    ctx.set_samples(1)
    if lights is not None:
        ctx.set_lights(lights)
    ctx.set_soft_shadows(radii, K)


def soft_kind(ctx, W=W0, H=H0):
    """What last_kernel reports for a soft frame: RT_KERNEL_SOFT where the hard frame of one light
    is the accelerated kernel's, RT_KERNEL_LANE where it is not. Leaves the settings in force."""
    lights, (radii, K) = ctx.get_lights(), ctx.get_soft_shadows()
    ctx.set_lights(lights[:1])
    ctx.set_soft_shadows(None)
    frame(ctx, W, H)
    one = ctx.accel_info()["last_kernel"]
    ctx.set_lights(lights)
    ctx.set_soft_shadows(radii, K)
    return rtamd.KERNEL_SOFT if one == rtamd.KERNEL_ACCEL else rtamd.KERNEL_LANE


@functools.lru_cache(maxsize=None)
def reference(key, W, H, count, radii, K, mt, fresnel):
    """soft_ref's frame of the first `count` fixed lights with `radii`; computed once, read-only."""
    fs = gr.scene(key)
    o, d = gr.rays(key, W, H)
    out = sf.shade(fs, o, d, sr.frame_sky(W, H), lr.fixed_lights(fs, count), radii, K, 3, bool(fresnel), bool(mt))
    out.setflags(write=False)
    return out


def same_floats(got, want):
    """Equal as floats, NaN exactly where `want` has NaN."""
    return np.array_equal(np.isnan(got), np.isnan(want)) and bool(((got == want) | np.isnan(want)).all())


# --------------------------------------------------------------------------
# 1. frames against the reference
def check_frame(ctx, name, count, K, mt, fresnel):
    fs = tr.scene(name)
    prepare(ctx, fs, mt, fresnel=fresnel, lights=lr.fixed_lights(fs, count), radii=SETS[count], K=K)
    kind = soft_kind(ctx)
    assert kind == rtamd.KERNEL_SOFT or name not in ("cfg2", "cfg3")  # the generator's scenes: the new frame kernel
    got = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == kind
    assert (got[:, 3] == 1).all()
    near_reference(got, reference(name, W0, H0, count, SETS[count], K, mt, fresnel),
                   f"{name} L{count} K{K} mt{mt} f{fresnel}")


@pytest.mark.parametrize("fresnel", [0, 1])
@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("name", tr.SCENES)
def test_frames_against_the_reference(ctx, name, count, K, mt, fresnel):
    check_frame(ctx, name, count, K, mt, fresnel)


def test_sixty_four_samples_against_the_reference(ctx):
    check_frame(ctx, "cfg3", 3, 64, 0, 0)


# --------------------------------------------------------------------------
# 2. every path gives the same bytes
@pytest.mark.parametrize("bvh", [1, 0])
@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", ["cfg3", "soup1"])
def test_every_path_gives_the_same_bytes(ctx, name, mt, bvh):
    fs = tr.scene(name)
    lights = lr.fixed_lights(fs, 3)
    prepare(ctx, fs, mt, bvh=bool(bvh), lights=lights, radii=MIXED, K=5)
    want = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT  # frame mode is what this test compares
    ctx.set_soft_shadows(None)
    hard = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS
    assert not np.array_equal(bits(want), bits(hard))
    # the tiny-radius anchor on this branch too (the brute-force branch has no numpy reference)
    ctx.set_soft_shadows((1e-30,) * 3, 5)
    tiny = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT
    assert same_floats(tiny, hard)
    ctx.set_soft_shadows(MIXED, 5)
    rays = ctx.camera_rays(W0, H0)
    listed = device_shade(ctx, rays)
    assert (listed[-1] == FILL).all()
    assert np.array_equal(bits(as_rgba(listed[:-1])), bits(want)), "rt_shade_rays over rt_camera_rays"
    ctx.set_kernel(rtamd.KERNEL_LANE)
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(want)), "the literal loop's frame"
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LANE
    assert np.array_equal(bits(as_rgba(device_shade(ctx, rays)[:-1])), bits(want)), "the literal loop's list"
    ctx.set_kernel(rtamd.KERNEL_PACKET)
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(want)), "RT_KERNEL_PACKET takes the literal loop"
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LANE
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_tree(rtamd.TREE_REFERENCE)
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(want)), "RT_TREE_REFERENCE"
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT


@pytest.mark.parametrize("fresnel", [0, 1])
@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", ["cfg3", "soup1"])
def test_repacked_samples_give_the_same_bytes(ctx, name, mt, fresnel):
    """rt_debug_soft: later bounces' sample rays repacked over the wave (form 1) and per live lane
    (form 2) write the frame's and the list's bytes, with K = 5 (h K no multiple of 64) and 64
    (the most items), and in a display format; the frame really has later bounces."""
    fs = tr.scene(name)
    prepare(ctx, fs, mt, fresnel=fresnel, lights=lr.fixed_lights(fs, 3), radii=MIXED, K=5)
    rays = ctx.camera_rays(W0, H0)
    try:
        for K in (5, 64):
            ctx.set_soft_shadows(MIXED, K)
            got = {}
            for form in (2, 1):
                ctx.debug_soft(form)
                got[form] = (frame(ctx, W0, H0), device_shade(ctx, rays),
                             rows_frame(ctx, W0, H0, rtamd.FORMAT_SRGBA8))
                assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT
            for a, b in zip(got[1], got[2]):
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), K
            ctx.set_params(W0, H0, 1, True, fresnel, mt)
            assert not np.array_equal(bits(frame(ctx, W0, H0)), bits(got[1][0])), "no later bounce in the frame"
            ctx.set_params(W0, H0, 3, True, fresnel, mt)
    finally:
        ctx.debug_soft(0)
    lib = rtamd.rt_lib()
    assert lib.rt_debug_soft(ctx._h, 3) == -1 and lib.rt_debug_soft(ctx._h, -1) == -1
    assert lib.rt_debug_soft(None, 1) == -1


def test_far_camera_takes_the_literal_loop(ctx):
    """A camera beyond the accelerator's origin bound: k_soft_ref renders the frame, and the list
    form over the accelerator gives the same bytes."""
    fs = gr.scene("cfg3:far")
    prepare(ctx, fs, lights=lr.fixed_lights(fs, 3), radii=MIXED, K=16)
    got = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LANE
    near_reference(got, reference("cfg3:far", W0, H0, 3, MIXED, 16, 0, 0), "far camera")
    assert np.array_equal(bits(as_rgba(device_shade(ctx, ctx.camera_rays(W0, H0))[:-1])), bits(got))


# --------------------------------------------------------------------------
# 3. device anchors
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
def test_tiny_radii_are_the_hard_frame(ctx, name, count):
    """Radii of 1e-30, K = 16, from the new kernels: the hard frame of the same lights from the
    existing kernels, as floats -- for one light too, whose hard frame is k_accel's."""
    fs = tr.scene(name)
    hard_kind = rtamd.KERNEL_ACCEL if count == 1 else rtamd.KERNEL_LIGHTS
    prepare(ctx, fs, lights=lr.fixed_lights(fs, count))
    hard = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == hard_kind
    rays = ctx.camera_rays(W0, H0)
    for kernel, kind in ((rtamd.KERNEL_AUTO, rtamd.KERNEL_SOFT), (rtamd.KERNEL_LANE, rtamd.KERNEL_LANE)):
        ctx.set_kernel(kernel)
        ctx.set_soft_shadows((1e-30,) * count, 16)
        tiny = frame(ctx, W0, H0)
        assert ctx.accel_info()["last_kernel"] == kind
        assert same_floats(tiny, hard), (name, count, kernel)
        assert np.array_equal(bits(as_rgba(device_shade(ctx, rays)[:-1])), bits(tiny))
        ctx.set_soft_shadows(None)


@pytest.mark.parametrize("count", [1, 3])
def test_radii_that_touch_no_light_change_nothing(ctx, count):
    """Radii cleared, all 0, or positive only at indices >= L: RT_KERNEL_ACCEL / RT_KERNEL_LIGHTS
    and the bytes of the frame and the list before the call; the setting survives rt_set_lights,
    rt_set_light and rt_upload_scene, and applies once a light reaches its index."""
    fs = tr.scene("cfg3")
    lights = lr.fixed_lights(fs, 4)
    hard_kind = rtamd.KERNEL_ACCEL if count == 1 else rtamd.KERNEL_LIGHTS
    prepare(ctx, fs, lights=lights[:count])
    today = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == hard_kind
    rays = ctx.camera_rays(W0, H0)
    listed = device_shade(ctx, rays)
    for radii in ((0.0,) * count, (0.0,) * count + (1.5,), (0.0,) * 7 + (3.0,), None):
        ctx.set_soft_shadows(radii, 16)
        assert np.array_equal(bits(frame(ctx, W0, H0)), bits(today)), radii
        assert ctx.accel_info()["last_kernel"] == hard_kind, radii
        assert np.array_equal(device_shade(ctx, rays), listed), radii
    # a radius waiting at index `count`: soft once the set grows to it, through every setter
    ctx.set_soft_shadows((0.0,) * count + (1.5,), 16)
    ctx.upload(fs)
    ctx.set_lights(lights[:count])
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(today))
    assert ctx.accel_info()["last_kernel"] == hard_kind
    ctx.set_lights(lights[:count + 1])
    grown = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT
    radii, K = ctx.get_soft_shadows()
    assert radii.tolist() == [0.0] * count + [1.5] and K == 16
    ctx.set_soft_shadows(None)
    assert not np.array_equal(bits(frame(ctx, W0, H0)), bits(grown))
    ctx.set_soft_shadows((2.0,), 16)
    ctx.set_light(lights[:1])
    frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT  # one light is soft too


# --------------------------------------------------------------------------
# 4. row mapping, formats, edges
@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
@pytest.mark.parametrize("size", gr.EDGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_rows_formats_and_edges(ctx, size, kernel):
    """Every edge size: the full frame against the reference; a striped dispatch (stripe 2, period
    6, y0 = 1, rows running past the frame) is the full frame's rows, rows past `height`, the
    bytes after `width` and the row after the last untouched; every other format is
    tests/fmt_ref.py's conversion of the float frame."""
    W, H = size
    fs = tr.scene("cfg3")
    prepare(ctx, fs, W=W, H=H, kernel=kernel, lights=lr.fixed_lights(fs, 3), radii=MIXED, K=16)
    full = frame(ctx, W, H)
    assert ctx.accel_info()["last_kernel"] == (rtamd.KERNEL_SOFT if kernel == rtamd.KERNEL_AUTO else rtamd.KERNEL_LANE)
    near_reference(full, reference("cfg3", W, H, 3, MIXED, 16, 0, 0), f"{W}x{H} kernel {kernel}")
    full = full.reshape(H, W, 4)
    T = rtamd.srgb_thresholds()
    y0, stripe, period = 1, 2, 6
    out_rows = 2 * ((H + period - 1) // period + 1)  # the last stripe lies past the frame
    inside = gr.dispatch_rows(H, y0, stripe, period, out_rows)
    assert len(inside) < out_rows
    for fmt in BYTES:
        px = BYTES[fmt]
        if fmt == rtamd.FORMAT_RGBA32F:
            want = full
        elif fmt == rtamd.FORMAT_RGB32F:
            want = full[..., :3]
        else:
            want = fmt_ref.convert(full, fmt, T)
        want = np.ascontiguousarray(want).view(np.uint8).reshape(H, W * px)
        whole = rows_frame(ctx, W, H, fmt, extra=1)
        assert np.array_equal(whole[:H, :W * px], want), (size, kernel, fmt)
        assert (whole[:, W * px:] == FILL).all() and (whole[H] == FILL).all(), (size, kernel, fmt)
        raw = rows_frame(ctx, W, H, fmt, y0, stripe, period, out_rows, extra=1)
        for r, y in inside:
            assert np.array_equal(raw[r, :W * px], want[y]), (size, kernel, fmt, r, y)
        untouched = sorted(set(range(out_rows + 1)) - {r for r, _ in inside})
        assert (raw[untouched] == FILL).all() and (raw[:, W * px:] == FILL).all(), (size, kernel, fmt)


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
def test_list_lengths_around_the_wave(ctx, kernel):
    """rt_shade_rays with the mixed set at n = 1, 63, 64, 65 and 257: the frame's first n pixels,
    the pixel after the last keeps its fill, in a float and a display format."""
    fs = tr.scene("cfg3")
    prepare(ctx, fs, kernel=kernel, lights=lr.fixed_lights(fs, 3), radii=MIXED, K=16)
    # rows 20.. of the frame: the car, not the sky
    rays = ctx.camera_rays(W0, H0, 20, 3)
    want = frame(ctx, W0, H0)[20 * W0:]
    T = rtamd.srgb_thresholds()
    for n in (1, 63, 64, 65, 257):
        got = device_shade(ctx, rays[:n], fill=0x5C)
        assert (got[n] == 0x5C).all(), (kernel, n)
        assert np.array_equal(bits(as_rgba(got[:n])), bits(want[:n])), (kernel, n)
        got8 = device_shade(ctx, rays[:n], rtamd.FORMAT_SRGBA8, fill=0x5C)
        assert (got8[n] == 0x5C).all(), (kernel, n)
        assert np.array_equal(got8[:n], fmt_ref.convert(want[:n], rtamd.FORMAT_SRGBA8, T)), (kernel, n)


# --------------------------------------------------------------------------
# 5. samples
@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
def test_samples_and_adaptive_samples(ctx, kernel):
    """A 48x27 output with rt_set_samples(2) and the mixed set is tests/ss_ref.py's box filter of
    the device's own 96x54 soft frame (resX, resY doubled), bit for bit; with
    rt_set_adaptive(1/16) it is tests/adaptive_ref.py's composition of the device's own B and S."""
    W, H, n = W0 // 2, H0 // 2, 2
    fs = tr.scene("cfg3")
    lights = lr.fixed_lights(fs, 3)
    kind = rtamd.KERNEL_SOFT if kernel == rtamd.KERNEL_AUTO else rtamd.KERNEL_LANE
    prepare(ctx, fs, W=W0, H=H0, kernel=kernel, lights=lights, radii=MIXED, K=16)
    fine = frame(ctx, W0, H0).reshape(H0, W0, 4)
    prepare(ctx, fs, W=W, H=H, kernel=kernel, lights=lights, radii=MIXED, K=16)
    B = frame(ctx, W, H).reshape(H, W, 4)
    ctx.set_samples(n)
    S = frame(ctx, W, H).reshape(H, W, 4)
    assert ctx.accel_info()["last_kernel"] == kind
    assert np.array_equal(bits(S), bits(ss_ref.box(fine, n)))
    assert not np.array_equal(bits(S), bits(B))
    raw = rows_frame(ctx, W, H, rtamd.FORMAT_RGBA16F)[:, :W * BYTES[rtamd.FORMAT_RGBA16F]]
    assert np.array_equal(raw, fmt_ref.convert(S, rtamd.FORMAT_RGBA16F).view(np.uint8).reshape(H, -1))
    ctx.set_adaptive(float(ar.THRESHOLD))
    m = ar.mask(B, np.arange(H), ar.THRESHOLD)
    assert 0 < m.mean() < 1, "both branches must run"
    got = frame(ctx, W, H).reshape(H, W, 4)
    assert ctx.accel_info()["last_kernel"] == kind
    assert np.array_equal(bits(got), bits(ar.compose(B, S, m)))
    assert ctx.adaptive_stats() == (int(m.sum()), W * H)


# --------------------------------------------------------------------------
# 6. pending updates and neutrality
@pytest.mark.parametrize("mt", [0, 1])
def test_pending_updates_are_applied(ctx, mt):
    """The car's wheels moved through rt_update_shapes + rt_update_nodes, then a soft frame: the
    frame of a fresh upload of the moved scene."""
    moved = gr.scene("cfg3:anim")
    lights = lr.fixed_lights(tr.scene("cfg3"), 2)
    prepare(ctx, moved, mt, lights=lights, radii=(2.0, 0.5), K=8)
    want = frame(ctx, W0, H0)
    ids, rec = gr.wheel_move()
    prepare(ctx, tr.scene("cfg3"), mt, lights=lights, radii=(2.0, 0.5), K=8)
    still = frame(ctx, W0, H0)
    assert not np.array_equal(bits(still), bits(want))
    ctx.update_shapes(int(ids[0]), rec)  # the wheels' records are contiguous
    ctx.update_nodes(moved.nodes)
    got = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT
    assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).any(axis=1).sum()} pixels differ"


def test_queries_and_stats_do_not_see_the_radii(ctx):
    """rt_trace_pixels, rt_gbuffer_host, rt_ao_host, rt_camera_rays and rt_collect_stats answer
    the same before and after rt_set_soft_shadows; a soft dispatch is one rt_kernel_times entry."""
    fs = tr.scene("cfg3")
    lights = lr.fixed_lights(fs, 3)
    xy = [(x, y) for y in range(0, H0, 5) for x in range(0, W0, 7)]

    def answers():
        return (ctx.trace_pixels(W0, H0, xy), ctx.gbuffer(W0, H0), ctx.ao(W0, H0, 8, 2.0),
                ctx.camera_rays(W0, H0))

    prepare(ctx, fs, lights=lights)
    before = answers()
    stats = ctx.collect_stats(W0, H0)
    ctx.set_soft_shadows(MIXED, 16)
    after = answers()
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
    for i in (1, 2):
        for k in before[i]:
            assert np.array_equal(before[i][k].view(np.uint8), after[i][k].view(np.uint8)), k
    assert np.array_equal(before[3].view(np.uint8), after[3].view(np.uint8))
    assert ctx.collect_stats(W0, H0) == stats
    frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT
    ctx.kernel_times()
    ctx.render(W0, H0)
    assert len(ctx.kernel_times()) == 1  # one entry per dispatch
    ctx.sync_frame()


# --------------------------------------------------------------------------
# 7. arguments
def test_arguments(ctx):
    lib = rtamd.rt_lib()
    fs = tr.scene("cfg3")
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    A = lambda *v: np.array(v, np.float32)  # noqa: E731
    prepare(ctx, fs, lights=lr.fixed_lights(fs, 3), radii=MIXED, K=7)
    want = frame(ctx, W0, H0)
    good, nine = A(1.0, 1.0, 1.0), A(*([1.0] * 9))
    refused = ((None, 2, 16), (good, -1, 16), (nine, 9, 16), (good, 1 << 20, 16), (good, 3, 0), (good, 3, -4),
               (good, 3, 65), (A(1.0, -0.5, 1.0), 3, 16), (A(1.0, np.nan), 2, 16), (A(np.inf), 1, 16),
               (A(1.0, -np.inf), 2, 16), (A(-1e-30), 1, 16))
    for args in refused:
        assert lib.rt_set_soft_shadows(ctx._h, None if args[0] is None else P(args[0]), *args[1:]) == -1, args
        radii, K = ctx.get_soft_shadows()  # the previous setting stays in force
        assert radii.tolist() == list(MIXED) and K == 7, args
    assert lib.rt_set_soft_shadows(None, P(good), 3, 16) == -1
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(want))
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_SOFT
    # rt_get_soft_shadows: a small cap, any pointer NULL
    out = np.full(8, 77, np.float32)
    n, k = C.c_int(-5), C.c_int(-5)
    assert lib.rt_get_soft_shadows(ctx._h, P(out), 2, C.byref(n), C.byref(k)) == 0 and (n.value, k.value) == (3, 7)
    assert out[:2].tolist() == list(MIXED[:2]) and (out[2:] == 77).all()
    n, k = C.c_int(-5), C.c_int(-5)
    assert lib.rt_get_soft_shadows(ctx._h, None, -1, C.byref(n), None) == 0 and n.value == 3
    assert lib.rt_get_soft_shadows(ctx._h, None, 0, None, C.byref(k)) == 0 and k.value == 7
    assert lib.rt_get_soft_shadows(ctx._h, P(out), 8, None, None) == 0 and out[:3].tolist() == list(MIXED)
    assert lib.rt_get_soft_shadows(ctx._h, None, 0, None, None) == 0
    assert lib.rt_get_soft_shadows(None, P(out), 8, C.byref(n), C.byref(k)) == -1
    assert lib.rt_get_soft_shadows(ctx._h, P(out), -1, C.byref(n), C.byref(k)) == -1
    assert lib.rt_set_kernel(ctx._h, rtamd.KERNEL_SOFT) == -1  # reported only
    # the limits themselves are taken; count 0 clears whatever the other arguments are
    eight = A(*([0.5] * 8))
    assert lib.rt_set_soft_shadows(ctx._h, P(eight), 8, 64) == 0
    assert ctx.get_soft_shadows()[1] == 64 and len(ctx.get_soft_shadows()[0]) == 8
    assert lib.rt_set_soft_shadows(ctx._h, P(good), 3, 1) == 0
    assert lib.rt_set_soft_shadows(ctx._h, None, 0, -99) == 0
    radii, K = ctx.get_soft_shadows()
    assert len(radii) == 0 and K == 0
    frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS
    ctx.set_soft_shadows([], 3)
    assert len(ctx.get_soft_shadows()[0]) == 0
    fresh = rtamd.ComputeShader(0)
    try:
        assert len(fresh.get_soft_shadows()[0]) == 0  # off is the default
    finally:
        fresh.close()
