"""Shaded rays on the device (rt_shade_rays / rt_shade_rays_host / rt_camera_rays): the camera
rays rt_camera_rays generates are the oracle's, bit for bit; shading them gives the bytes of the
frame rt_dispatch_rows renders (every scene, triangle test, Fresnel, bounce count and useBVH
branch), whatever camera the context holds; any other ray gets the same bytes from k_shade and
from the literal loop (k_shade_ref) and the value of tests/shade_ref.py's numpy restatement, which
tests/test_shade_cpu.py ties to the oracle's frame on the CPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fmt_ref
import gbuffer_ref as gr
import oracle
import rtamd
import shade_ref as sr
import trace_rays as tr
from frame_check import close_to_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-4
W0, H0 = gr.W0, gr.H0
FILL = 0xAB
BYTES = {rtamd.FORMAT_RGBA32F: 16, rtamd.FORMAT_RGB32F: 12, rtamd.FORMAT_RGBA8: 4, rtamd.FORMAT_SRGBA8: 4,
         rtamd.FORMAT_RGBA16F: 8}
UNIT_SETS = ("camera", "random", "axis", "far", "grazing")
REF_RAYS = 2000


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


def prepare(ctx, fs, mt=False, W=W0, H=H0, kernel=rtamd.KERNEL_AUTO, tree=rtamd.TREE_SCENE, bounces=3, bvh=True,
            fresnel=False):
    ctx.upload(fs)
    ctx.set_animated(np.zeros(0, np.int32))
    ctx.set_params(W, H, bounces, bvh, fresnel, mt)
    ctx.set_kernel(kernel)
    ctx.set_tree(tree)
    ctx.set_samples(1)
    ctx.debug_shade(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def device_camera_rays(ctx, W, H, y0=0, rows=None, extra=1, fill=FILL):
    """rt_camera_rays on a torch buffer pre-filled with `fill`: raw bytes [W * rows + extra, 32]."""
    rows = H - y0 if rows is None else rows
    t = torch.full(((W * rows + extra) * 32,), fill, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # the context's stream does not wait on torch's
    ctx.camera_rays_device(W, H, y0, rows, t.data_ptr())
    ctx.sync()
    return t.cpu().numpy().reshape(W * rows + extra, 32)


def device_shade(ctx, rays, fmt=rtamd.FORMAT_RGBA32F, extra=1, fill=FILL):
    """rt_shade_rays on torch buffers: the pixels as raw bytes [n + extra, bytes per pixel], the
    buffer pre-filled with `fill`."""
    n, px = len(rays), BYTES[fmt]
    r = to_device(rays) if n else None
    out = torch.full(((n + extra) * px,), fill, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.shade_rays_device(r.data_ptr() if n else 0, n, out.data_ptr(), fmt)
    ctx.sync()
    return out.cpu().numpy().reshape(n + extra, px)


def frame(ctx, W, H):
    """rt_dispatch_rows of the whole frame in RGBA32F, as raw bytes [W * H, 16]."""
    out = torch.full((W * H * 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
    ctx.sync()
    return out.cpu().numpy().reshape(W * H, 16)


def as_rays(raw):
    return np.ascontiguousarray(raw).view(rtamd.VIEW_RAY_DTYPE).reshape(-1)


def as_rgba(raw):
    return np.ascontiguousarray(raw).view(np.float32).reshape(-1, 4)


def near_oracle(px, ref, what):
    close_to_oracle(px, ref.reshape(-1, 4), TOL, what)


@pytest.mark.parametrize("size", [(W0, H0)] + list(gr.EDGE_SIZES), ids=lambda s: "%dx%d" % s)
def test_camera_rays_are_the_oracles(ctx, size):
    """1. rt_camera_rays: origin and direction of the oracle's get_ray, sky = f32(y) / f32(resY),
    reserved 0, on their bytes; a band; the record after the last keeps its fill."""
    W, H = size
    prepare(ctx, tr.scene("cfg3"), W=W, H=H)
    o, d = gr.rays("cfg3", W, H)
    want = rtamd.ComputeShader.make_view_rays(o, d, sr.frame_sky(W, H))
    raw = device_camera_rays(ctx, W, H)
    assert (raw[-1] == FILL).all()
    assert np.array_equal(raw[:-1].reshape(-1), want.view(np.uint8).reshape(-1))
    assert np.array_equal(ctx.camera_rays(W, H).view(np.uint8), want.view(np.uint8))
    if H > 14:
        band = device_camera_rays(ctx, W, H, 5, 9, fill=0x5C)
        assert (band[-1] == 0x5C).all()
        assert np.array_equal(band[:-1], raw[5 * W:14 * W])
        assert np.array_equal(ctx.camera_rays(W, H, 5, 9).view(np.uint8).reshape(-1, 32), band[:-1])


FRAME_CASES = [(n, 3, True, f, m) for n in tr.SCENES for m in (0, 1) for f in (0, 1)] + \
              [("cfg3", 0, True, 0, 0), ("cfg3", 1, True, 0, 0), ("cfg3", 1, True, 1, 1),
               ("cfg2", 3, False, 0, 0), ("cfg2", 3, False, 1, 1), ("cfg3", 3, False, 0, 0), ("cfg3", 3, False, 1, 1)]


@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: "%s_b%d_bvh%d_f%d_mt%d" % c)
def test_shaded_camera_rays_are_the_frame(ctx, case):
    """2. rt_shade_rays(rt_camera_rays(...)) in RGBA32F equals rt_dispatch_rows of the same
    context byte for byte, and lies within 1e-4 of oracle.render."""
    name, bounces, bvh, fresnel, mt = case
    fs = tr.scene(name)
    prepare(ctx, fs, mt, bounces=bounces, bvh=bvh, fresnel=fresnel)
    rays = as_rays(device_camera_rays(ctx, W0, H0, extra=0))
    got = device_shade(ctx, rays)
    assert (got[-1] == FILL).all()
    want = frame(ctx, W0, H0)
    assert np.array_equal(got[:-1], want), f"{case}: {(got[:-1] != want).any(axis=1).sum()} pixels differ from the frame"
    ref, _ = oracle.render(fs, W0, H0, oracle.params(W0, H0, bounces, bvh, fresnel, mt))
    near_oracle(as_rgba(got[:-1]), ref, str(case))
    assert (as_rgba(got[:-1])[:, 3] == 1).all()
    # the literal loop gives the same bytes
    ctx.set_kernel(rtamd.KERNEL_LANE)
    assert np.array_equal(device_shade(ctx, rays), got)
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def test_the_camera_plays_no_part(ctx):
    """3. Rays of cfg3:far's camera and of a shifted camera, shaded while the scene's own camera
    is set, equal the frames rendered with those cameras (the far one by the packet kernel)."""
    fs = tr.scene("cfg3")
    far = np.array(gr.scene("cfg3:far").camera, rtamd.CAMERA_DTYPE).reshape(-1)[:1].copy()
    shifted = np.array(fs.camera, rtamd.CAMERA_DTYPE).reshape(-1)[:1].copy()
    shifted["Position"][0] = shifted["Position"][0] + np.float32(0.4) * shifted["Right"][0] + \
        np.float32(0.25) * shifted["Up"][0]
    prepare(ctx, fs)
    own = frame(ctx, W0, H0)
    lists, frames = [], []
    for cam, kind in ((far, rtamd.KERNEL_PACKET), (shifted, rtamd.KERNEL_ACCEL)):
        ctx.set_camera(cam)
        lists.append(as_rays(device_camera_rays(ctx, W0, H0, extra=0)))
        frames.append(frame(ctx, W0, H0))
        assert ctx.accel_info()["last_kernel"] == kind
    assert not np.array_equal(frames[0], own) and not np.array_equal(frames[1], own)
    ctx.set_camera(fs.camera)
    assert ctx.accel_info()["built"] == 1
    for rays, want in zip(lists, frames):
        assert np.array_equal(device_shade(ctx, rays, extra=0), want)
    assert np.array_equal(frame(ctx, W0, H0), own)


def set_rays(name):
    """{set: VIEW_RAY_DTYPE records} of trace_rays.ray_sets(name), sky uniform in [0, 1)."""
    rng = np.random.default_rng(11)
    return {k: rtamd.ComputeShader.make_view_rays(o, d, rng.random(len(o), dtype=np.float32))
            for k, (o, d) in tr.ray_sets(name).items()}


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_any_ray_every_kernel(ctx, name, mt):
    """4. Every ray set: RT_KERNEL_AUTO, RT_KERNEL_LANE and RT_KERNEL_PACKET write byte-identical
    pixels, over both trees; a seeded choice of at most 2,000 rays of each unit-direction set is
    within 1e-4 * max(1, |reference|) of tests/shade_ref.py, NaN exactly where it has NaN."""
    fs = tr.scene(name)
    sets = set_rays(name)
    got = {}
    for tree in (rtamd.TREE_SCENE, rtamd.TREE_REFERENCE):
        prepare(ctx, fs, mt, tree=tree)
        for k, rays in sets.items():
            auto = device_shade(ctx, rays, extra=0)
            got.setdefault(k, auto)
            assert np.array_equal(auto, got[k]), f"{name} mt {mt} {k}: the trees differ"
        for kernel in (rtamd.KERNEL_LANE, rtamd.KERNEL_PACKET):
            ctx.set_kernel(kernel)
            for k, rays in sets.items():
                other = device_shade(ctx, rays, extra=0)
                bad = (other != got[k]).any(axis=1).sum()
                assert bad == 0, f"{name} mt {mt} {k} tree {tree}: kernel {kernel} differs in {bad} pixels"
        ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_tree(rtamd.TREE_SCENE)
    rng = np.random.default_rng(13)
    for k in UNIT_SETS:
        if k not in sets:
            continue
        rays = sets[k]
        pick = np.sort(rng.permutation(len(rays))[:REF_RAYS])
        want = sr.shade(fs, rays["origin"][pick], rays["dir"][pick], rays["sky"][pick], 3, False, bool(mt))
        px = as_rgba(got[k])[pick]
        assert np.array_equal(np.isnan(px), np.isnan(want)), f"{name} mt {mt} {k}: NaN in other places"
        with np.errstate(all="ignore"):
            ok = (px == want) | (np.abs(px - want) <= TOL * np.maximum(1.0, np.abs(want))) | np.isnan(want)
        assert ok.all(), (f"{name} mt {mt} {k}: {(~ok).any(axis=1).sum()} rays off the reference, e.g. ray "
                          f"{pick[np.where(~ok)[0][0]]}: {px[np.where(~ok)[0][0]]} vs {want[np.where(~ok)[0][0]]}")


def test_formats(ctx):
    """5. The four non-float32 formats of a shaded camera list are tests/fmt_ref.py's conversion
    of the RGBA32F list, bit for bit (RGB32F: the first three floats)."""
    T = rtamd.srgb_thresholds()
    for name, mt in (("cfg3", 0), ("cfg2", 1)):
        prepare(ctx, tr.scene(name), mt)
        rays = ctx.camera_rays(W0, H0)
        for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
            ctx.set_kernel(kernel)
            rgba = as_rgba(device_shade(ctx, rays, extra=0))
            rgb = device_shade(ctx, rays, rtamd.FORMAT_RGB32F)
            assert (rgb[-1] == FILL).all()
            assert np.array_equal(rgb[:-1].view(np.uint32), bits(rgba[:, :3]))
            for fmt in (rtamd.FORMAT_RGBA8, rtamd.FORMAT_SRGBA8, rtamd.FORMAT_RGBA16F):
                raw = device_shade(ctx, rays, fmt)
                assert (raw[-1] == FILL).all()
                want = fmt_ref.convert(rgba, fmt, T)
                assert np.array_equal(raw[:-1], want.view(np.uint8).reshape(len(rays), -1)), (name, kernel, fmt)
        ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
def test_wave_and_block_edges(ctx, kernel):
    """6. Prefixes of one shuffled ray list on the car around the wave (64) and the literal
    kernel's block (256): the common prefix is identical, pixel n keeps its fill, n = 0 writes
    nothing."""
    sets = set_rays("cfg3")
    rays = np.concatenate(list(sets.values()))
    rays = rays[np.random.default_rng(3).permutation(len(rays))[:1025]]
    prepare(ctx, tr.scene("cfg3"), kernel=kernel)
    for fmt in (rtamd.FORMAT_RGBA32F, rtamd.FORMAT_RGB32F, rtamd.FORMAT_RGBA8):
        full = device_shade(ctx, rays, fmt)
        assert (full[-1] == FILL).all()
        for n in (1, 63, 64, 65, 255, 256, 257):
            part = device_shade(ctx, rays[:n], fmt, fill=0x5C)
            assert np.array_equal(part[:n], full[:n]), (kernel, fmt, n)
            assert (part[n] == 0x5C).all(), (kernel, fmt, n)
        assert (device_shade(ctx, rays[:0], fmt) == FILL).all()
    assert ctx.shade_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 4)
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("path", ["animate", "update"])
@pytest.mark.parametrize("mt", [0, 1])
def test_pending_updates_are_applied(ctx, mt, path):
    """7a. The car's wheels moved (rt_animate, or rt_update_shapes + rt_update_nodes), then a
    shade call with no dispatch in between: the frame of cfg3:anim, after one refit."""
    moved = gr.scene("cfg3:anim")
    prepare(ctx, moved, mt)
    want = frame(ctx, W0, H0)
    ids, rec = gr.wheel_move()
    prepare(ctx, tr.scene("cfg3"), mt)
    rays = ctx.camera_rays(W0, H0)
    still = device_shade(ctx, rays, extra=0)  # Moller-Trumbore: its accelerator exists from here on, and refits
    assert not np.array_equal(still, want)
    r0 = ctx.debug_refits()
    if path == "animate":
        ctx.set_animated(ids)
        ctx.animate(rec)
    else:
        ctx.update_shapes(int(ids[0]), rec)  # the wheels' records are contiguous
        ctx.update_nodes(moved.nodes)
        assert ctx.debug_refits() == r0
    got = device_shade(ctx, rays, extra=0)
    assert ctx.debug_refits() == r0 + 1
    assert np.array_equal(got, want), f"{(got != want).any(axis=1).sum()} pixels differ from the moved scene's frame"
    ctx.set_kernel(rtamd.KERNEL_LANE)
    assert np.array_equal(device_shade(ctx, rays, extra=0), want)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    assert ctx.debug_refits() == r0 + 1
    ctx.set_animated(np.zeros(0, np.int32))


def test_shading_leaves_the_renderer_alone(ctx):
    """7b. Shade calls between two frames: the surface, rt_accel_info::last_kernel, the record of
    rt_kernel_times / rt_last_kernel_ms and the tile cost order stay as the frame left them, and
    the next frame is byte-identical."""
    W, H = 160, 90
    fs = rtamd.generate(3, 0, W, H)
    prepare(ctx, fs, False, W, H)
    ctx.kernel_times()
    first = ctx.render(W, H)
    before = ctx.accel_info()["last_kernel"], ctx.last_kernel_ms()
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    order = ctx.debug_sched_order(tiles)
    assert before[0] == rtamd.KERNEL_ACCEL and len(order) == tiles
    sets = set_rays("cfg3")
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        ctx.set_kernel(kernel)
        rays = ctx.camera_rays(W, H)
        ctx.shade_rays(rays, None)
        device_shade(ctx, sets["random"], rtamd.FORMAT_RGBA8)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    assert (ctx.accel_info()["last_kernel"], ctx.last_kernel_ms()) == before
    times = ctx.kernel_times()
    assert len(times) == 1 and times[0] == np.float32(before[1])  # the frame's dispatch, nothing else
    assert np.array_equal(ctx.debug_sched_order(tiles), order)
    assert np.array_equal(bits(ctx.read_image(W, H)), bits(first))  # the surface
    ctx.sync_frame()
    second = ctx.render(W, H)
    assert np.array_equal(bits(first), bits(second))
    assert len(ctx.kernel_times()) == 1


def test_host_forms_and_arguments(ctx):
    """8. The host forms give the device forms' bytes; every listed error returns its code and
    writes nothing; a scene without nodes gives every ray its background."""
    lib = rtamd.rt_lib()
    fs = tr.scene("cfg3")
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    V = C.c_void_p
    n = 100

    prepare(ctx, fs)
    dev = device_camera_rays(ctx, W0, H0, extra=0)
    rays = ctx.camera_rays(W0, H0)
    assert np.array_equal(rays.view(np.uint8).reshape(-1, 32), dev)
    for fmt in BYTES:
        host = ctx.shade_rays(rays, None, fmt=fmt)
        assert np.array_equal(host.view(np.uint8).reshape(len(rays), -1), device_shade(ctx, rays, fmt, extra=0)), fmt
    few = np.ascontiguousarray(rays[:n])
    host_px = np.full((n + 1) * 16, FILL, np.uint8)

    fresh = rtamd.ComputeShader(0)
    try:
        host_rays = np.zeros(W0 * H0, rtamd.VIEW_RAY_DTYPE)
        assert lib.rt_shade_rays_host(fresh._h, P(few), n, P(host_px), 0) == -4
        assert lib.rt_camera_rays_host(fresh._h, W0, H0, 0, H0, P(host_rays)) == -4
        assert lib.rt_shade_rays_host(fresh._h, P(few), -1, P(host_px), 0) == -1
        rc = lib.rt_upload_scene(fresh._h, P(fs.shapes), len(fs.shapes), P(fs.nodes), len(fs.nodes), P(fs.indices),
                                 len(fs.indices))
        assert rc == 0
        assert lib.rt_shade_rays_host(fresh._h, P(few), n, P(host_px), 0) == -4  # no light, no params
        fresh.set_light(fs.light)
        assert lib.rt_shade_rays_host(fresh._h, P(few), n, P(host_px), 0) == -4  # no params
        assert (host_px == FILL).all()
        fresh.set_params(W0, H0)
        assert lib.rt_camera_rays_host(fresh._h, W0, H0, 0, H0, P(host_rays)) == -4  # no camera
        # a camera is not needed to shade
        assert lib.rt_shade_rays_host(fresh._h, P(few), n, P(host_px), 0) == 0
        assert (host_px[n * 16:] == FILL).all()
        assert np.array_equal(host_px[:n * 16].reshape(n, 16), device_shade(ctx, few, extra=0))
        fresh.set_camera(fs.camera)
        assert lib.rt_camera_rays_host(fresh._h, W0, H0, 0, H0, P(host_rays)) == 0
        assert np.array_equal(host_rays, rays)
    finally:
        fresh.close()
    # camera rays need no scene
    bare = rtamd.ComputeShader(0)
    try:
        bare.set_camera(fs.camera)
        host_rays = np.zeros(W0 * H0, rtamd.VIEW_RAY_DTYPE)
        assert lib.rt_camera_rays_host(bare._h, W0, H0, 0, H0, P(host_rays)) == -4  # no params
        bare.set_params(W0, H0)
        assert lib.rt_camera_rays_host(bare._h, W0, H0, 0, H0, P(host_rays)) == 0
        assert np.array_equal(host_rays, rays)
    finally:
        bare.close()

    r = to_device(few)
    r4 = torch.zeros(len(r) + 16, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + 1) * 16,), FILL, dtype=torch.uint8, device="cuda")
    cam = torch.full(((W0 * H0 + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dr, do, dc = r.data_ptr(), out.data_ptr(), cam.data_ptr()
    assert dr % 16 == 0 and do % 16 == 0 and dc % 16 == 0 and r4.data_ptr() % 16 == 0
    assert lib.rt_shade_rays(None, V(dr), n, V(do), 0) == -1
    assert lib.rt_shade_rays_host(None, P(few), n, P(host_px), 0) == -1
    for args in ((None, n, V(do), 0), (V(dr), n, None, 0), (V(dr), -1, V(do), 0),
                 (V(dr), n, V(do), rtamd.FORMAT_RGBA32F_IMAGE), (V(dr), n, V(do), 6), (V(dr), n, V(do), -1),
                 (V(r4.data_ptr() + 4), n, V(do), 0), (V(dr), n, V(do + 4), 0), (V(dr), n, V(do + 8), 0),
                 (V(dr), n, V(do + 2), rtamd.FORMAT_RGB32F), (V(dr), n, V(do + 2), rtamd.FORMAT_RGBA8),
                 (V(dr), n, V(do + 1), rtamd.FORMAT_SRGBA8), (V(dr), n, V(do + 4), rtamd.FORMAT_RGBA16F),
                 (V(dr), 0, V(do), 6)):
        assert lib.rt_shade_rays(ctx._h, *args) == -1, args
    for args in ((None, n, P(host_px), 0), (P(few), n, None, 0), (P(few), -5, P(host_px), 0),
                 (P(few), n, P(host_px), 2), (P(few), n, P(host_px), 7)):
        assert lib.rt_shade_rays_host(ctx._h, *args) == -1, args
    assert lib.rt_shade_rays(ctx._h, None, 0, None, 0) == 0
    assert lib.rt_shade_rays_host(ctx._h, None, 0, None, rtamd.FORMAT_RGBA8) == 0
    assert lib.rt_camera_rays(None, W0, H0, 0, H0, V(dc)) == -1
    for args in ((0, H0, 0, H0, V(dc)), (W0, 0, 0, 1, V(dc)), (W0, H0, 0, 0, V(dc)), (W0, H0, 0, -2, V(dc)),
                 (W0, H0, -1, 4, V(dc)), (W0, H0, 1, H0, V(dc)), (W0, H0, H0, 1, V(dc)), (W0, H0, 0, H0, None),
                 (W0, H0, 0, H0, V(dc + 4)), (1 << 16, 1 << 15, 0, 1 << 15, V(dc))):
        assert lib.rt_camera_rays(ctx._h, *args) == -1, args
    host_rays = np.full(W0 * H0 * 32, FILL, np.uint8)
    for args in ((W0, H0, 0, H0 + 1, P(host_rays)), (W0, H0, 0, H0, None), (-3, H0, 0, H0, P(host_rays))):
        assert lib.rt_camera_rays_host(ctx._h, *args) == -1, args
    ctx.sync()
    assert (out.cpu().numpy() == FILL).all() and (cam.cpu().numpy() == FILL).all()  # nothing was written
    assert (host_px[n * 16:] == FILL).all() and (host_rays == FILL).all()

    # N = 0: the BVH branch sees no shape, every ray takes its own background
    import test_gpu_parity as tg
    sky = np.random.default_rng(5).random(n, dtype=np.float32)
    o, d = gr.rays("cfg3", W0, H0)
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, tg._empty_scene(W0, H0), kernel=kernel)
        px = ctx.shade_rays(o[:n], d[:n], sky)
        assert np.array_equal(bits(px[:, :3]), bits(sr.background(sky))) and (px[:, 3] == 1).all()
    ctx.set_kernel(rtamd.KERNEL_AUTO)
