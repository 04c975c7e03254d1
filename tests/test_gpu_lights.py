"""More than one point light on the device (rt_set_lights): frames of 2, 3 and 8 lights against
tests/lights_ref.py's numpy restatement (anchored to the oracle by tests/test_lights_cpu.py);
the frame kernel, the list kernel, the literal loop and the reference tree write the same
bytes; one light is today's frame and today's kernel; row mapping, formats and edges; samples
and adaptive samples; pending scene writes; the calls that must not see the lights; arguments.
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
import ss_ref
import trace_rays as tr
from test_gpu_shade import TOL  # the project's tolerance for shaded rays: TOL * max(1, |reference|)

pytestmark = pytest.mark.gpu
W0, H0 = gr.W0, gr.H0
FILL = 0xAB
PAD = 16  # guard bytes after each row (keeps every format's pitch alignment)
BYTES = {rtamd.FORMAT_RGBA32F: 16, rtamd.FORMAT_RGB32F: 12, rtamd.FORMAT_RGBA8: 4, rtamd.FORMAT_SRGBA8: 4,
         rtamd.FORMAT_RGBA16F: 8}


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
    ctx.set_samples(1)
    ctx.set_adaptive(-1.0)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_tree(rtamd.TREE_SCENE)
    ctx.set_animated(np.zeros(0, np.int32))


def prepare(ctx, fs, mt=False, W=W0, H=H0, kernel=rtamd.KERNEL_AUTO, tree=rtamd.TREE_SCENE, bounces=3, bvh=True,
            fresnel=False, lights=None):
    ctx.upload(fs)  # sets the scene's own light: one light
    ctx.set_animated(np.zeros(0, np.int32))
    ctx.set_params(W, H, bounces, bvh, fresnel, mt)
    ctx.set_kernel(kernel)
    ctx.set_tree(tree)
    ctx.set_samples(1)
    if lights is not None:
        ctx.set_lights(lights)


def lights_kind(ctx, W=W0, H=H0):
    """What last_kernel reports for a frame of several lights: RT_KERNEL_LIGHTS where the one-light
    frame is the accelerated kernel's, RT_KERNEL_LANE where it is not. Leaves the set in force."""
    held = ctx.get_lights()
    ctx.set_lights(held[:1])
    frame(ctx, W, H)
    one = ctx.accel_info()["last_kernel"]
    ctx.set_lights(held)
    return rtamd.KERNEL_LIGHTS if one == rtamd.KERNEL_ACCEL else rtamd.KERNEL_LANE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_frame(ctx, W, H, fmt=rtamd.FORMAT_RGBA32F, y0=0, stripe=1, period=1, out_rows=None, extra=0):
    """rt_dispatch_rows_ex into a buffer pre-filled with FILL: raw bytes [out_rows + extra, W * px + PAD]."""
    out_rows = H if out_rows is None else out_rows
    pitch = W * BYTES[fmt] + PAD
    t = torch.full(((out_rows + extra) * pitch,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # the context's stream does not wait on torch's
    ctx.dispatch_rows_ex(W, H, y0, stripe, period, out_rows, t.data_ptr(), pitch, fmt=fmt)
    ctx.sync()
    return t.cpu().numpy().reshape(out_rows + extra, pitch)


def frame(ctx, W, H):
    """The whole frame through rt_dispatch_rows in RGBA32F: [H * W, 4] float32, guards checked."""
    pitch = W * 16 + PAD
    t = torch.full((H * pitch,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.dispatch_rows(W, H, 0, 1, 1, H, t.data_ptr(), pitch)
    ctx.sync()
    raw = t.cpu().numpy().reshape(H, pitch)
    assert (raw[:, W * 16:] == FILL).all()
    return np.ascontiguousarray(raw[:, :W * 16]).view(np.float32).reshape(H * W, 4)


def device_shade(ctx, rays, fmt=rtamd.FORMAT_RGBA32F, fill=FILL):
    """rt_shade_rays on torch buffers: raw bytes [n + 1, bytes per pixel], the last one a guard."""
    n, px = len(rays), BYTES[fmt]
    r = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.full(((n + 1) * px,), fill, dtype=torch.uint8, device="cuda")
    assert r.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.shade_rays_device(r.data_ptr(), n, out.data_ptr(), fmt)
    ctx.sync()
    return out.cpu().numpy().reshape(n + 1, px)


def as_rgba(raw):
    return np.ascontiguousarray(raw).view(np.float32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def reference(key, W, H, count, mt, fresnel):
    """lights_ref's frame of the first `count` fixed lights; computed once, read-only."""
    fs = gr.scene(key)
    o, d = gr.rays(key, W, H)
    out = lr.shade(fs, o, d, sr.frame_sky(W, H), lr.fixed_lights(fs, count), 3, bool(fresnel), bool(mt))
    out.setflags(write=False)
    return out


def near_reference(px, want, what):
    """Every pixel within TOL * max(1, |reference|), NaN exactly where the reference has NaN.
    Returns the largest |difference| / max(1, |reference|)."""
    assert px.shape == want.shape, what
    assert np.array_equal(np.isnan(px), np.isnan(want)), f"{what}: NaN in other places"
    with np.errstate(all="ignore"):
        err = np.abs(px.astype(np.float64) - want.astype(np.float64)) / np.maximum(1.0, np.abs(want.astype(np.float64)))
        ok = (px == want) | (err <= TOL) | np.isnan(want)
    worst = float(np.nanmax(np.where(px == want, 0.0, err)))
    print(f"{what}: max |device - reference| / max(1, |reference|) = {worst:.3g}")
    assert ok.all(), f"{what}: {(~ok).any(axis=1).sum()} pixels off the reference, worst {worst:.3g}"
    return worst


# --------------------------------------------------------------------------
# 1. frames against the reference
@pytest.mark.parametrize("fresnel", [0, 1])
@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("count", [2, 3, 8])
@pytest.mark.parametrize("name", tr.SCENES)
def test_frames_against_the_reference(ctx, name, count, mt, fresnel):
    fs = tr.scene(name)
    prepare(ctx, fs, mt, fresnel=fresnel, lights=lr.fixed_lights(fs, count))
    kind = lights_kind(ctx)
    assert kind == rtamd.KERNEL_LIGHTS or name not in ("cfg2", "cfg3")  # the generator's scenes: the new frame kernel
    got = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == kind
    assert (got[:, 3] == 1).all()
    near_reference(got, reference(name, W0, H0, count, mt, fresnel), f"{name} L{count} mt{mt} f{fresnel}")


# --------------------------------------------------------------------------
# 2. every path gives the same bytes
@pytest.mark.parametrize("bvh", [1, 0])
@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", ["cfg3", "soup1"])
def test_every_path_gives_the_same_bytes(ctx, name, mt, bvh):
    fs = tr.scene(name)
    lights = lr.fixed_lights(fs, 3)
    prepare(ctx, fs, mt, bvh=bool(bvh), lights=lights)
    want = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS  # frame mode is what this test compares
    # the zero-colour anchor on this branch too (the brute-force branch has no numpy reference)
    black = np.concatenate([lights[:1], lights[1:2]])
    black["color"][1] = 0
    ctx.set_lights(black)
    two = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS
    ctx.set_lights(lights[:1])
    one = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
    assert np.array_equal(np.isnan(two), np.isnan(one)) and ((two == one) | np.isnan(one)).all()
    assert not np.array_equal(bits(want), bits(one))
    ctx.set_lights(lights)
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
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS


def test_far_camera_takes_the_literal_loop(ctx):
    """A camera beyond the accelerator's origin bound: k_lights_ref renders the frame, and the
    list form over the accelerator gives the same bytes."""
    fs = gr.scene("cfg3:far")
    prepare(ctx, fs, lights=lr.fixed_lights(fs, 3))
    got = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LANE
    near_reference(got, reference("cfg3:far", W0, H0, 3, 0, 0), "far camera")
    assert np.array_equal(bits(as_rgba(device_shade(ctx, ctx.camera_rays(W0, H0))[:-1])), bits(got))


# --------------------------------------------------------------------------
# 3. L = 1 is today's frame
@pytest.mark.parametrize("name", ["cfg3", "cfg2"])
def test_one_light_is_todays_frame(ctx, name):
    fs = tr.scene(name)
    prepare(ctx, fs)
    today = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
    own = rtamd.as_records(fs.light, rtamd.LIGHT_DTYPE).reshape(-1)[:1]
    ctx.set_lights(own)
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(today))
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
    ctx.set_lights(lr.fixed_lights(fs, 3))
    three = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS
    assert not np.array_equal(bits(three), bits(today))
    ctx.set_light(fs.light)
    assert len(ctx.get_lights()) == 1
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(today))
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
    # a second light of colour 0, from the new kernels: the one-light frame as floats
    black = np.concatenate([own, lr.fixed_lights(fs, 2)[1:]])
    black["color"][1] = 0
    for kernel, kind in ((rtamd.KERNEL_AUTO, rtamd.KERNEL_LIGHTS), (rtamd.KERNEL_LANE, rtamd.KERNEL_LANE)):
        ctx.set_kernel(kernel)
        ctx.set_lights(black)
        two = frame(ctx, W0, H0)
        assert ctx.accel_info()["last_kernel"] == kind
        assert np.array_equal(np.isnan(two), np.isnan(today)) and ((two == today) | np.isnan(today)).all(), kernel
        rays = ctx.camera_rays(W0, H0)
        assert np.array_equal(bits(as_rgba(device_shade(ctx, rays)[:-1])), bits(two))


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
    prepare(ctx, fs, W=W, H=H, kernel=kernel, lights=lr.fixed_lights(fs, 3))
    full = frame(ctx, W, H)
    assert ctx.accel_info()["last_kernel"] == (rtamd.KERNEL_LIGHTS if kernel == rtamd.KERNEL_AUTO else rtamd.KERNEL_LANE)
    near_reference(full, reference("cfg3", W, H, 3, 0, 0), f"{W}x{H} kernel {kernel}")
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
    """rt_shade_rays with three lights at n = 1, 63, 64, 65 and 257: the frame's first n pixels,
    the pixel after the last keeps its fill, in a float and a display format."""
    fs = tr.scene("cfg3")
    prepare(ctx, fs, kernel=kernel, lights=lr.fixed_lights(fs, 3))
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
    """A 48x27 output with rt_set_samples(2) and three lights is tests/ss_ref.py's box filter of
    the device's own 96x54 three-light frame (resX, resY doubled), bit for bit; with
    rt_set_adaptive(1/16) it is tests/adaptive_ref.py's composition of the device's own B and S."""
    W, H, n = W0 // 2, H0 // 2, 2
    fs = tr.scene("cfg3")
    lights = lr.fixed_lights(fs, 3)
    kind = rtamd.KERNEL_LIGHTS if kernel == rtamd.KERNEL_AUTO else rtamd.KERNEL_LANE
    prepare(ctx, fs, W=W0, H=H0, kernel=kernel, lights=lights)
    fine = frame(ctx, W0, H0).reshape(H0, W0, 4)
    prepare(ctx, fs, W=W, H=H, kernel=kernel, lights=lights)
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
    """The car's wheels moved through rt_update_shapes + rt_update_nodes, then a two-light frame:
    the frame of a fresh upload of the moved scene."""
    moved = gr.scene("cfg3:anim")
    lights = lr.fixed_lights(tr.scene("cfg3"), 2)
    prepare(ctx, moved, mt, lights=lights)
    want = frame(ctx, W0, H0)
    ids, rec = gr.wheel_move()
    prepare(ctx, tr.scene("cfg3"), mt, lights=lights)
    still = frame(ctx, W0, H0)
    assert not np.array_equal(bits(still), bits(want))
    ctx.update_shapes(int(ids[0]), rec)  # the wheels' records are contiguous
    ctx.update_nodes(moved.nodes)
    got = frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS
    assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).any(axis=1).sum()} pixels differ"


def test_queries_and_stats_do_not_see_the_lights(ctx):
    """rt_trace_pixels, rt_gbuffer_host and rt_ao_host answer the same before and after
    rt_set_lights; rt_collect_stats counts the one-light frame of light 0."""
    fs = tr.scene("cfg3")
    lights = lr.fixed_lights(fs, 3)
    xy = [(x, y) for y in range(0, H0, 5) for x in range(0, W0, 7)]

    def answers():
        return (ctx.trace_pixels(W0, H0, xy), ctx.gbuffer(W0, H0), ctx.ao(W0, H0, 8, 2.0),
                ctx.camera_rays(W0, H0))

    prepare(ctx, fs)
    ctx.set_light(lights[:1])
    before = answers()
    stats = ctx.collect_stats(W0, H0)
    ctx.set_lights(lights)
    after = answers()
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
    for i in (1, 2):
        for k in before[i]:
            assert np.array_equal(before[i][k].view(np.uint8), after[i][k].view(np.uint8)), k
    assert np.array_equal(before[3].view(np.uint8), after[3].view(np.uint8))
    assert ctx.collect_stats(W0, H0) == stats
    frame(ctx, W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_LIGHTS
    ctx.kernel_times()
    ctx.render(W0, H0)
    assert len(ctx.kernel_times()) == 1  # one entry per dispatch
    ctx.sync_frame()


# --------------------------------------------------------------------------
# 7. arguments
def test_arguments(ctx):
    lib = rtamd.rt_lib()
    fs = tr.scene("cfg3")
    lights = lr.fixed_lights(fs, 8)
    nine = np.concatenate([lights, lights[:1]])
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    prepare(ctx, fs, lights=lights[:3])
    want = frame(ctx, W0, H0)
    for args in ((None, 2), (P(lights), 0), (P(lights), -1), (P(nine), 9), (P(lights), 1 << 20)):
        assert lib.rt_set_lights(ctx._h, *args) == -1, args
    assert lib.rt_set_lights(None, P(lights), 2) == -1
    assert lib.rt_set_light(ctx._h, None) == -1
    got = ctx.get_lights()
    assert got.tobytes() == lights[:3].tobytes()
    assert np.array_equal(bits(frame(ctx, W0, H0)), bits(want))  # the previous set stays in force
    # rt_get_lights: a small cap, either pointer NULL
    out = np.zeros(8, rtamd.LIGHT_DTYPE)
    out["position"] = 77
    n = C.c_int(-5)
    assert lib.rt_get_lights(ctx._h, P(out), 2, C.byref(n)) == 0 and n.value == 3
    assert out[:2].tobytes() == lights[:2].tobytes() and (out["position"][2:] == 77).all()
    n = C.c_int(-5)
    assert lib.rt_get_lights(ctx._h, None, 0, C.byref(n)) == 0 and n.value == 3
    assert lib.rt_get_lights(ctx._h, P(out), 8, None) == 0 and out[:3].tobytes() == lights[:3].tobytes()
    assert lib.rt_get_lights(ctx._h, None, 0, None) == 0
    assert lib.rt_get_lights(None, P(out), 8, C.byref(n)) == -1
    assert lib.rt_get_lights(ctx._h, P(out), -1, C.byref(n)) == -1
    assert lib.rt_set_kernel(ctx._h, rtamd.KERNEL_LIGHTS) == -1  # reported only
    ctx.set_lights(lights)
    assert ctx.get_lights().tobytes() == lights.tobytes()
    fresh = rtamd.ComputeShader(0)
    try:
        assert len(fresh.get_lights()) == 0
    finally:
        fresh.close()
