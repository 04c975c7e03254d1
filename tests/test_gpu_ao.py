"""Ambient occlusion on the device (rt_dispatch_ao / rt_ao_host): every pixel's count equals the
reference of tests/ao_ref.py (include/rt_api.h's definition restated in numpy over the oracle's
geometry buffer, the counts from the oracle's own occlusion walk) and every visibility its bit
pattern -- from the repacked kernel, its per-hit-lane form and the literal walk, barycentric and
Moller-Trumbore, over both trees. tests/test_ao_cpu.py shows on the CPU that these rays are
ones the accelerated walk answers exactly.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ao_ref as ar
import gbuffer_ref as gr
import rtamd
import trace_rays as tr

pytestmark = pytest.mark.gpu
W0, H0, W1, H1 = ar.W0, ar.H0, ar.W1, ar.H1
PX = {"count": 1, "visibility": 4}
K0, BIAS = ar.K0, ar.BIAS
FILL = 0xAB
INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


def prepare(ctx, fs, mt=False, W=W0, H=H0, kernel=rtamd.KERNEL_AUTO, tree=rtamd.TREE_SCENE):
    ctx.upload(fs)
    ctx.set_animated(np.zeros(0, np.int32))
    ctx.set_params(W, H, 3, True, False, mt)
    ctx.set_kernel(kernel)
    ctx.set_tree(tree)
    ctx.debug_ao(0, 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dispatch(ctx, W, H, K=K0, radius=2.0, y0=0, stripe=1, period=1, out_rows=None, planes=ar.PLANES, pad=0, extra=0):
    """rt_dispatch_ao into torch buffers pre-filled with FILL: per plane the raw bytes
    [out_rows + extra, pitch], pitch = the row's bytes + pad."""
    out_rows = H if out_rows is None else out_rows
    bufs, args = {}, {}
    for name in planes:
        pitch = W * PX[name] + pad
        t = torch.full(((out_rows + extra) * pitch,), FILL, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        bufs[name] = (t, pitch)
        args[name] = (t.data_ptr(), pitch)
    torch.cuda.synchronize()  # the context's stream does not wait on torch's
    ctx.ao_device(W, H, y0, stripe, period, out_rows, K, radius, BIAS, **args)
    ctx.sync()
    return {name: t.cpu().numpy().reshape(out_rows + extra, pitch) for name, (t, pitch) in bufs.items()}


def typed(raw, name, W):
    """The first W pixels of every row of a plane's raw bytes, as rt_api.h types them."""
    a = np.ascontiguousarray(raw[:, :W * PX[name]])
    return a if name == "count" else a.view(np.float32)


def expect(raw, ref, W, what, rows=None):
    """Raw planes of a dispatch against the reference frame, every pixel: count for equality,
    visibility on its bits; rows: [(compact r, image y)]."""
    for name, bytes_ in raw.items():
        got, want = typed(bytes_, name, W), ref[name]
        if rows is not None:
            got, want = got[[r for r, _ in rows]], want[[y for _, y in rows]]
        g, w = (got, want) if name == "count" else (bits(got), bits(want))
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what} {name}: {len(bad)} pixels differ, e.g. at {tuple(bad[0])}: "
                               f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_exact_against_the_oracle(ctx, name, mt):
    """1. Both planes equal the reference for every pixel of a 96x54 frame, K = 16, radius 2.0
    and +inf, both tree modes; misses hold 0 and 1.0f."""
    miss = gr.reference(name, W0, H0, mt)["shape"] < 0
    for tree in (rtamd.TREE_SCENE, rtamd.TREE_REFERENCE):
        prepare(ctx, tr.scene(name), mt, tree=tree)
        for radius in ar.RADII:
            ref = ar.reference(name, W0, H0, mt, K0, radius)
            raw = dispatch(ctx, W0, H0, K0, radius)
            expect(raw, ref, W0, f"{name} mt {mt} tree {tree} radius {radius}")
            count, vis = typed(raw["count"], "count", W0), typed(raw["visibility"], "visibility", W0)
            assert not count[miss].any() and (bits(vis[miss]) == bits(np.float32(1.0))).all()
            assert (count > 0).sum() >= 50
        info = ctx.accel_info()
        assert info["built"] == 1 and info["scene_tree"] == 1
    ctx.set_tree(rtamd.TREE_SCENE)


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_every_form_writes_the_same_bytes(ctx, name, mt):
    """2. RT_KERNEL_AUTO, RT_KERNEL_LANE and RT_KERNEL_PACKET (the literal walk), both
    rt_debug_ao forms at 1, 2 and 4 waves per block, and the host form: byte-identical planes."""
    prepare(ctx, tr.scene(name), mt)
    auto = dispatch(ctx, W0, H0)
    expect(auto, ar.reference(name, W0, H0, mt, K0, 2.0), W0, f"{name} mt {mt}")
    for kernel in (rtamd.KERNEL_LANE, rtamd.KERNEL_PACKET):
        ctx.set_kernel(kernel)
        other = dispatch(ctx, W0, H0)
        for p in ar.PLANES:
            assert np.array_equal(auto[p], other[p]), f"{name} mt {mt}: kernel {kernel} differs in {p}"
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    for form in (1, 2):
        for waves in (1, 2, 4):
            ctx.debug_ao(form, waves)
            other = dispatch(ctx, W0, H0)
            for p in ar.PLANES:
                assert np.array_equal(auto[p], other[p]), f"{name} mt {mt}: form {form} waves {waves} differs in {p}"
    ctx.debug_ao(0, 0)
    host = ctx.ao(W0, H0, K0, 2.0, BIAS)
    assert host["count"].dtype == np.uint8 and host["visibility"].dtype == np.float32
    for p in ar.PLANES:
        assert np.array_equal(host[p].view(np.uint8).reshape(H0, -1), auto[p]), p


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_the_composed_path_agrees(ctx, name, mt):
    """3. rt_dispatch_gbuffer's planes read back, the rays of ao_ref built from them,
    rt_trace_rays(RT_TRACE_ANY) and a sum per pixel: the sums equal `count`."""
    prepare(ctx, tr.scene(name), mt)
    count = ctx.ao(W0, H0, K0, 2.0, BIAS, planes=("count",))["count"].reshape(-1)
    g = ctx.gbuffer(W0, H0, planes=("shape", "normal", "position"))
    _, d = gr.rays(name, W0, H0)
    idx = np.where(g["shape"].reshape(-1) >= 0)[0]
    assert len(idx) > 1000
    o, dirs = ar.build_rays(g["position"].reshape(-1, 4)[idx, :3], g["normal"].reshape(-1, 4)[idx, :3], d[idx],
                            idx % W0, idx // W0, K0, BIAS)
    ro, rd = ar.flat_rays(o, dirs)
    _, _, occluded = ctx.trace_rays(ro, rd, np.full(len(ro), 2.0, np.float32), any_hit=True)
    want = np.zeros(W0 * H0, np.int64)
    want[idx] = (occluded != 0).reshape(len(idx), K0).sum(axis=1)
    assert np.array_equal(count.astype(np.int64), want)


@pytest.mark.parametrize("K", [1, 5, 64])
def test_ray_counts(ctx, K):
    """4. K = 1, 5 and 64: each equals the reference's sum over the first K of the 64 rays (the
    prefix property), from both forms and the literal walk. With K = 1 and 5 most tiles' h * K
    work items are no multiple of 64: the repacked form's last round is partial."""
    hit = gr.reference("cfg3", W0, H0, 0)["shape"] >= 0
    h = np.array([hit[y:y + 8, x:x + 8].sum() for y in range(0, H0, 8) for x in range(0, W0, 8)])
    if K != 64:  # h * 64 is always whole rounds; K = 5 has tiles of several rounds, the last one partial
        assert ((h * K) % 64 != 0).sum() >= 10 and (K == 1 or ((h * K > 64) & ((h * K) % 64 != 0)).any())
    prepare(ctx, tr.scene("cfg3"))
    for radius in ar.RADII:
        ref = ar.reference("cfg3", W0, H0, 0, K, radius)
        assert ref["count"].max() <= K and (ref["count"] > 0).sum() >= 10
        for form in (1, 2):
            ctx.debug_ao(form, 0)
            expect(dispatch(ctx, W0, H0, K, radius), ref, W0, f"K {K} radius {radius} form {form}")
        ctx.debug_ao(0, 0)
    ctx.set_kernel(rtamd.KERNEL_LANE)
    expect(dispatch(ctx, W0, H0, K, 2.0), ar.reference("cfg3", W0, H0, 0, K, 2.0), W0, f"K {K} literal")
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("rows", [(8, 8, 24, 24), (0, 3, 7, 24), (16, 8, 16, 20), (53, 1, 1, 3)])
def test_stripes(ctx, rows):
    """5a. Compact row r of a striped dispatch is row y(r) of the full frame's planes (the
    rotation of step 4 follows the image row, not the compact row), into planes with 5 pad
    bytes a row (count) and one row more than out_rows: every byte outside the written pixels
    keeps its fill. Both planes together and one at a time."""
    y0, stripe, period, out_rows = rows
    ref = ar.reference("cfg3", W0, H0, 0, K0, 2.0)
    inside = gr.dispatch_rows(H0, y0, stripe, period, out_rows)
    assert 0 < len(inside) and (len(inside) < out_rows) == (rows in ((8, 8, 24, 24), (53, 1, 1, 3)))
    untouched = sorted(set(range(out_rows + 1)) - {r for r, _ in inside})
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, tr.scene("cfg3"), kernel=kernel)
        for planes, pad in ((ar.PLANES, 8), (("count",), 5), (("visibility",), 4)):
            raw = dispatch(ctx, W0, H0, K0, 2.0, y0, stripe, period, out_rows, planes=planes, pad=pad, extra=1)
            assert sorted(raw) == sorted(planes)
            expect(raw, ref, W0, f"stripes {rows} kernel {kernel} planes {planes}", rows=inside)
            for p, b in raw.items():
                assert (b[untouched] == FILL).all(), (rows, kernel, p)
                assert (b[:, W0 * PX[p]:] == FILL).all(), (rows, kernel, p, "pad bytes")
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
def test_edges_of_the_frame_and_of_memory(ctx, kernel):
    """5b. Frames of 1x1, 8x8, 9x1, 1x9 and 41x27 into planes with odd pad bytes per row and two
    rows more than out_rows, all pre-filled: the written pixels are the reference, every other
    byte keeps the fill (the count plane is written bytewise); rows past the frame too."""
    fs = tr.scene("cfg3")
    for W, H in gr.EDGE_SIZES:
        prepare(ctx, fs, False, W, H, kernel=kernel)
        ref = ar.reference("cfg3", W, H, 0, K0, 2.0)
        for planes, pad in ((ar.PLANES, 12), (("count",), 3)):
            for form in (1, 2):
                ctx.debug_ao(form, 0)
                raw = dispatch(ctx, W, H, K0, 2.0, planes=planes, pad=pad, extra=2)
                expect({p: b[:H] for p, b in raw.items()}, ref, W, f"{W}x{H} kernel {kernel} form {form}")
                for p, b in raw.items():
                    assert (b[:, W * PX[p]:] == FILL).all(), (W, H, p, "pad bytes")
                    assert (b[H:] == FILL).all(), (W, H, p, "rows after out_rows")
    ctx.debug_ao(0, 0)
    raw = dispatch(ctx, W1, H1, K0, 2.0, y0=20, out_rows=12, pad=4, extra=2)
    expect({p: b[:7] for p, b in raw.items()}, ref, W1, "rows past the frame", rows=[(r, 20 + r) for r in range(7)])
    for p, b in raw.items():
        assert (b[7:] == FILL).all() and (b[:, W1 * PX[p]:] == FILL).all(), p
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("mt", [0, 1])
def test_far_camera(ctx, mt):
    """6a. cfg3:far, the camera beyond the accelerator's origin bound: the camera rays walk per
    lane; both forms of the occlusion walk and the literal walk give the reference."""
    ref = ar.reference("cfg3:far", W0, H0, mt, K0, 2.0)
    prepare(ctx, gr.scene("cfg3:far"), mt)
    ctx.render(W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_PACKET
    for form in (1, 2):
        ctx.debug_ao(form, 0)
        expect(dispatch(ctx, W0, H0), ref, W0, f"far mt {mt} form {form}")
    ctx.debug_ao(0, 0)
    expect(dispatch(ctx, W0, H0, K0, INF), ar.reference("cfg3:far", W0, H0, mt, K0, INF), W0, f"far mt {mt} inf")


@pytest.mark.parametrize("mt", [0, 1])
def test_animated_scene_is_seen_without_a_dispatch(ctx, mt):
    """6b. cfg3:anim: the car's wheels moved through rt_animate and left pending; the planes are
    the reference over the moved shapes and updateBVH's nodes, after exactly one refit."""
    ids, rec = gr.wheel_move()
    W, H = ar.WA, ar.HA
    ref = ar.reference("cfg3:anim", W, H, mt, K0, 2.0)
    prepare(ctx, tr.scene("cfg3"), mt, W, H)
    ctx.gbuffer(W, H, planes=("shape",))  # Moller-Trumbore: its accelerator exists from here on
    r0 = ctx.debug_refits()
    ctx.set_animated(ids)
    ctx.animate(rec)
    expect(dispatch(ctx, W, H), ref, W, f"animated mt {mt}")
    assert ctx.debug_refits() == r0 + 1
    ctx.set_kernel(rtamd.KERNEL_LANE)
    expect(dispatch(ctx, W, H), ref, W, f"animated mt {mt} literal")
    assert ctx.debug_refits() == r0 + 1
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_animated(np.zeros(0, np.int32))


def test_ties(ctx):
    """6c. cfg3:ties, every shape twice: the same counts as the single scene, as the oracle says."""
    ref, single = ar.reference("cfg3:ties", W0, H0, 0, K0, 2.0), ar.reference("cfg3", W0, H0, 0, K0, 2.0)
    assert np.array_equal(ref["count"], single["count"])
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, gr.scene("cfg3:ties"), kernel=kernel)
        expect(dispatch(ctx, W0, H0), ref, W0, f"ties kernel {kernel}")
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def test_arguments(ctx):
    """7. Every error of rt_api.h returns its code and leaves pre-filled planes untouched;
    RT_ERR_NO_SCENE before the upload and without params; out_rows == 0 is RT_OK. All refusals
    happen on the host: no bad pointer reaches a kernel."""
    lib = rtamd.rt_lib()
    fs = tr.scene("cfg3")
    W, H = W0, H0
    host = {p: np.full((H, W * PX[p]), FILL, np.uint8) for p in ar.PLANES}

    def ao(planes, **over):
        g = rtamd.rt_ao()
        for p, (ptr, pitch) in planes.items():
            setattr(g, p, ptr)
            setattr(g, p + "_pitch", pitch)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def par(rays=K0, radius=2.0, bias=BIAS, reserved=0):
        return rtamd.rt_ao_params(rays, radius, bias, reserved)

    hostg = {p: (a.ctypes.data, W * PX[p]) for p, a in host.items()}
    fresh = rtamd.ComputeShader(0)
    try:
        assert lib.rt_ao_host(fresh._h, W, H, C.byref(par()), C.byref(ao(hostg))) == -4
        assert lib.rt_dispatch_ao(fresh._h, W, H, 0, 1, 1, H, C.byref(par()), C.byref(ao(hostg))) == -4
        assert lib.rt_ao_host(fresh._h, W, H, C.byref(par()), None) == -1
        fresh.upload(fs)  # scene, camera and light
        assert lib.rt_ao_host(fresh._h, W, H, C.byref(par()), C.byref(ao(hostg))) == -4  # no params
        assert all((a == FILL).all() for a in host.values())
        fresh.set_params(W, H)
        assert lib.rt_ao_host(fresh._h, W, H, C.byref(par()), C.byref(ao(hostg))) == 0
        expect(host, ar.reference("cfg3", W, H, 0, K0, 2.0), W, "host form of a fresh context")
    finally:
        fresh.close()
    for arr in host.values():
        arr[:] = FILL  # the refusals below must leave them so

    prepare(ctx, fs)
    dev = {p: torch.full((H * W * PX[p] + 64,), FILL, dtype=torch.uint8, device="cuda") for p in ar.PLANES}
    torch.cuda.synchronize()
    ok = {p: (t.data_ptr(), W * PX[p]) for p, t in dev.items()}
    big = {p: (ptr, 65536 * 4) for p, (ptr, _) in ok.items()}  # pitches that pass for any width tried below
    cptr, cpitch = ok["count"]
    vptr, vpitch = ok["visibility"]

    def call(g, p=par(), w=W, h=H, y0=0, stripe=1, period=1, rows=H):
        return lib.rt_dispatch_ao(ctx._h, w, h, y0, stripe, period, rows, C.byref(p) if p is not None else None,
                                  C.byref(g) if g is not None else None)

    invalid = [
        ("out NULL", lambda: call(None)),
        ("params NULL", lambda: call(ao(ok), None)),
        ("both planes NULL", lambda: call(ao({}))),
        ("both planes NULL, pitches set", lambda: call(ao({}, count_pitch=W, visibility_pitch=4 * W))),
        ("width 0", lambda: call(ao(ok), w=0)),
        ("width < 0", lambda: call(ao(ok), w=-W)),
        ("height 0", lambda: call(ao(ok), h=0)),
        ("height < 0", lambda: call(ao(ok), h=-1)),
        ("y0 < 0", lambda: call(ao(ok), y0=-1)),
        ("stripe 0", lambda: call(ao(ok), stripe=0, period=0)),
        ("stripe < 0", lambda: call(ao(ok), stripe=-1)),
        ("out_rows < 0", lambda: call(ao(ok), rows=-1)),
        ("period < stripe", lambda: call(ao(ok), stripe=8, period=7)),
        ("too many tile rows", lambda: call(ao(big), w=1, h=10, rows=8 * 65535 + 1)),
        ("width * out_rows = 2^32", lambda: call(ao(big), w=65536, h=10, rows=65536)),
        ("rays 0", lambda: call(ao(ok), par(rays=0))),
        ("rays < 0", lambda: call(ao(ok), par(rays=-1))),
        ("rays 65", lambda: call(ao(ok), par(rays=65))),
        ("radius NaN", lambda: call(ao(ok), par(radius=math.nan))),
        ("radius 0", lambda: call(ao(ok), par(radius=0.0))),
        ("radius < 0", lambda: call(ao(ok), par(radius=-2.0))),
        ("radius -inf", lambda: call(ao(ok), par(radius=-INF))),
        ("bias NaN", lambda: call(ao(ok), par(bias=math.nan))),
        ("bias < 0", lambda: call(ao(ok), par(bias=-1e-3))),
        ("bias inf", lambda: call(ao(ok), par(bias=INF))),
        ("reserved", lambda: call(ao(ok), par(reserved=1))),
        ("count pitch short", lambda: call(ao({**ok, "count": (cptr, W - 1)}))),
        ("count alone, pitch short", lambda: call(ao({"count": (cptr, W - 1)}))),
        ("visibility pitch short", lambda: call(ao({**ok, "visibility": (vptr, vpitch - 4)}))),
        ("visibility pitch unaligned", lambda: call(ao({**ok, "visibility": (vptr, vpitch + 2)}))),
        ("visibility pointer unaligned", lambda: call(ao({**ok, "visibility": (vptr + 2, vpitch)}))),
        ("visibility alone, pitch short", lambda: call(ao({"visibility": (vptr, vpitch - 4)}))),
    ]
    for what, fn in invalid:
        assert fn() == -1, what
    # the host form checks the same way
    for p, g in ((par(), None), (None, ao(hostg)), (par(), ao({})), (par(rays=65), ao(hostg)),
                 (par(radius=0.0), ao(hostg)), (par(), ao({**hostg, "count": (hostg["count"][0], W - 1)})),
                 (par(), ao({**hostg, "visibility": (hostg["visibility"][0] + 2, 4 * W)}))):
        assert lib.rt_ao_host(ctx._h, W, H, C.byref(p) if p is not None else None,
                              C.byref(g) if g is not None else None) == -1
    assert lib.rt_ao_host(ctx._h, 0, H, C.byref(par()), C.byref(ao(hostg))) == -1
    assert lib.rt_ao_host(ctx._h, W, -1, C.byref(par()), C.byref(ao(hostg))) == -1
    # out_rows == 0: RT_OK, nothing launched; +inf radius, zero bias and an odd count pitch are accepted
    assert call(ao(ok), rows=0) == 0
    ctx.sync()
    assert all((t.cpu().numpy() == FILL).all() for t in dev.values())  # none of these calls wrote a byte
    assert all((a == FILL).all() for a in host.values())
    assert call(ao(ok), par(radius=INF, bias=0.0)) == 0
    assert call(ao({"count": (cptr + 1, W + 1)}), rows=H - 1) == 0
    ctx.sync()

    import test_gpu_parity as tg
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, tg._empty_scene(W, H), kernel=kernel)
        raw = dispatch(ctx, W, H)
        assert not raw["count"].any()
        assert (bits(typed(raw["visibility"], "visibility", W)) == bits(np.float32(1.0))).all()
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def test_the_renderer_is_left_alone(ctx):
    """8. Dispatches between two adaptively supersampled frames: last_kernel, the record of
    rt_kernel_times, rt_adaptive_stats and the surface stay as the frame left them, the next
    frame is byte-identical, and the planes are those taken with rt_set_samples(1)."""
    prepare(ctx, tr.scene("cfg3"))
    one = dispatch(ctx, W0, H0)
    try:
        ctx.set_samples(4)
        ctx.set_adaptive(1.0 / 16)
        ctx.kernel_times()
        first = ctx.render(W0, H0)
        before = ctx.accel_info()["last_kernel"], ctx.last_kernel_ms(), ctx.adaptive_stats()
        assert before[0] == rtamd.KERNEL_ACCEL and 0 < before[2][0] < before[2][1] == W0 * H0
        tiles = ((W0 + 7) // 8) * ((H0 + 7) // 8)
        order = ctx.debug_sched_order(tiles)
        for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
            ctx.set_kernel(kernel)
            dev = dispatch(ctx, W0, H0)
            host = ctx.ao(W0, H0, K0, 2.0, BIAS)
            for p in ar.PLANES:
                assert np.array_equal(dev[p], one[p]) and np.array_equal(host[p].view(np.uint8).reshape(H0, -1), one[p])
        ctx.set_kernel(rtamd.KERNEL_AUTO)
        assert (ctx.accel_info()["last_kernel"], ctx.last_kernel_ms(), ctx.adaptive_stats()) == before
        assert np.array_equal(bits(ctx.read_image(W0, H0)), bits(first))
        times = ctx.kernel_times()
        assert len(times) == 1 and times[0] == np.float32(before[1])  # the frame's dispatch, nothing else
        assert np.array_equal(ctx.debug_sched_order(tiles), order)
        ctx.sync_frame()
        second = ctx.render(W0, H0)
        assert np.array_equal(bits(first), bits(second))
        assert len(ctx.kernel_times()) == 1
    finally:
        ctx.set_samples(1)
        ctx.set_adaptive(-1.0)
        ctx.set_kernel(rtamd.KERNEL_AUTO)
