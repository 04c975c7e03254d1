"""Geometry buffers on the device (rt_dispatch_gbuffer / rt_gbuffer_host): every pixel's shape,
depth, normal and position equal the reference of tests/gbuffer_ref.py (the oracle's walk and
intersection, the normal restated in float32) -- shape and depth for equality, normal and
position on their bit patterns -- from the packet kernel, its per-lane form and the literal
walk, barycentric and Moller-Trumbore, over both trees. tests/test_gbuffer_cpu.py shows on the
CPU that the reference is the oracle's own and that these camera rays are ones the accelerated
walk is exact for.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gbuffer_ref as gr
import rtamd
import trace_rays as tr

pytestmark = pytest.mark.gpu
W0, H0, W1, H1 = gr.W0, gr.H0, gr.W1, gr.H1
PX = {"shape": 4, "depth": 4, "normal": 16, "position": 16}
FILL = 0xAB


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
    ctx.debug_gbuffer(0, 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dispatch(ctx, W, H, y0=0, stripe=1, period=1, out_rows=None, planes=gr.PLANES, pad=0, extra=0):
    """rt_dispatch_gbuffer into torch buffers pre-filled with FILL: per plane the raw bytes
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
    ctx.gbuffer_device(W, H, y0, stripe, period, out_rows, **args)
    ctx.sync()
    return {name: t.cpu().numpy().reshape(out_rows + extra, pitch) for name, (t, pitch) in bufs.items()}


def typed(raw, name, W):
    """The first W pixels of every row of a plane's raw bytes, as rt_api.h types them."""
    a = np.ascontiguousarray(raw[:, :W * PX[name]])
    if name == "shape":
        return a.view(np.int32)
    a = a.view(np.float32)
    return a if name == "depth" else a.reshape(len(a), W, 4)


def same(got, want, what):
    """One plane against the reference: every pixel, integers for equality, floats on their bits."""
    g = got if got.dtype == np.int32 else bits(got)
    w = want if want.dtype == np.int32 else bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, e.g. at {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def expect(raw, ref, W, what, rows=None):
    """Raw planes of a dispatch against the reference frame; rows: [(compact r, image y)]."""
    for name, bytes_ in raw.items():
        got, want = typed(bytes_, name, W), ref[name]
        if rows is None:
            same(got, want, f"{what} {name}")
        else:
            r, y = [r for r, _ in rows], [y for _, y in rows]
            same(got[r], want[y], f"{what} {name}")


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_exact_against_the_oracle(ctx, name, mt):
    """1. All four planes equal the reference for every pixel of a 96x54 frame (a partial last
    tile row), both tree modes; misses hold -1, 1e20f and zeros; position.w is the hit mask."""
    ref = gr.reference(name, W0, H0, mt)
    for tree in (rtamd.TREE_SCENE, rtamd.TREE_REFERENCE):
        prepare(ctx, tr.scene(name), mt, tree=tree)
        raw = dispatch(ctx, W0, H0)
        expect(raw, ref, W0, f"{name} mt {mt} tree {tree}")
        info = ctx.accel_info()
        assert info["built"] == 1 and info["scene_tree"] == 1
        shape, depth = typed(raw["shape"], "shape", W0), typed(raw["depth"], "depth", W0)
        normal, position = typed(raw["normal"], "normal", W0), typed(raw["position"], "position", W0)
        miss = shape < 0
        assert (shape[miss] == -1).all() and (bits(depth[miss]) == bits(np.float32(1e20))).all()
        assert not bits(normal[miss]).any() and not bits(position[miss]).any()
        assert np.array_equal(position[..., 3], (~miss).astype(np.float32)) and not bits(normal[..., 3]).any()
        assert (~miss).sum() > 1000
    ctx.set_tree(rtamd.TREE_SCENE)


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_kernel_variants_write_the_same_bytes(ctx, name, mt):
    """2. RT_KERNEL_AUTO (packets), RT_KERNEL_LANE and RT_KERNEL_PACKET (the literal walk), the
    accelerated per-lane form and the other block shapes give byte-identical planes, the host
    form too; rt_trace_pixels over all pixels returns the same shape and distance."""
    prepare(ctx, tr.scene(name), mt)
    auto = dispatch(ctx, W0, H0)
    for kernel in (rtamd.KERNEL_LANE, rtamd.KERNEL_PACKET):
        ctx.set_kernel(kernel)
        other = dispatch(ctx, W0, H0)
        for p in gr.PLANES:
            assert np.array_equal(auto[p], other[p]), f"{name} mt {mt}: kernel {kernel} differs in {p}"
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    for walk, waves in ((1, 0), (1, 4), (0, 2), (0, 4)):
        ctx.debug_gbuffer(walk, waves)
        other = dispatch(ctx, W0, H0)
        for p in gr.PLANES:
            assert np.array_equal(auto[p], other[p]), f"{name} mt {mt}: walk {walk} waves {waves} differs in {p}"
    ctx.debug_gbuffer(0, 0)
    host = ctx.gbuffer(W0, H0)
    for p in gr.PLANES:
        assert np.array_equal(host[p].view(np.uint8).reshape(H0, -1), auto[p]), p
    xy = np.array([(x, y) for y in range(H0) for x in range(W0)], np.int32)
    shape, dist, _ = ctx.trace_pixels(W0, H0, xy)
    assert np.array_equal(shape.reshape(H0, W0), host["shape"])
    assert np.array_equal(bits(dist).reshape(H0, W0), bits(host["depth"]))


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_far_camera(ctx, name, mt):
    """3. The camera 2,000 units back with fov 1: beyond the accelerator's origin bound (an
    ordinary frame falls to RT_KERNEL_PACKET), so the planes come from the per-lane walk."""
    fs = gr.scene(name + ":far")
    ref = gr.reference(name + ":far", W0, H0, mt)
    if not mt:
        assert (ref["shape"] >= 0).sum() == {"cfg2": 5184, "cfg3": 2301, "cfg5": 2974, "soup1": 5184}[name]
    prepare(ctx, fs, mt)
    ctx.render(W0, H0)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_PACKET
    expect(dispatch(ctx, W0, H0), ref, W0, f"{name} far mt {mt}")


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
def test_edges_of_the_frame_and_of_memory(ctx, kernel):
    """4. Frames of 1x1, 8x8, 9x1, 1x9 and 41x27 into planes with 48 pad bytes per row and two
    rows more than out_rows, all pre-filled: the written region is the reference, every pad
    byte and extra row keeps the fill; rows past the frame's height too."""
    fs = tr.scene("cfg3")
    for W, H in gr.EDGE_SIZES:
        prepare(ctx, fs, False, W, H, kernel=kernel)
        ref = gr.reference("cfg3", W, H, 0)
        raw = dispatch(ctx, W, H, pad=48, extra=2)
        expect({p: b[:H] for p, b in raw.items()}, ref, W, f"{W}x{H} kernel {kernel}")
        for p, b in raw.items():
            assert (b[:, W * PX[p]:] == FILL).all(), (W, H, p, "pad bytes")
            assert (b[H:] == FILL).all(), (W, H, p, "rows after out_rows")
    # y0 + out_rows > height: compact rows 7.. have no image row
    raw = dispatch(ctx, W1, H1, y0=20, out_rows=12, pad=48, extra=2)
    expect({p: b[:7] for p, b in raw.items()}, ref, W1, "rows past the frame", rows=[(r, 20 + r) for r in range(7)])
    for p, b in raw.items():
        assert (b[7:] == FILL).all() and (b[:, W1 * PX[p]:] == FILL).all(), p
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def test_planes_are_independent(ctx):
    """5. Each of the 15 non-empty subsets of the planes: every plane it has is byte-identical
    to that plane of the all-four dispatch."""
    prepare(ctx, tr.scene("cfg3"), False, W1, H1)
    full = dispatch(ctx, W1, H1)
    expect(full, gr.reference("cfg3", W1, H1, 0), W1, "all four")
    subsets = [s for n in range(1, 5) for s in itertools.combinations(gr.PLANES, n)]
    assert len(subsets) == 15
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        ctx.set_kernel(kernel)
        for s in subsets:
            part = dispatch(ctx, W1, H1, planes=s)
            assert sorted(part) == sorted(s)
            for p in s:
                assert np.array_equal(part[p], full[p]), (kernel, s, p)
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("rows", [(8, 8, 24, 24), (0, 3, 7, 24), (16, 8, 16, 20)])
def test_stripes(ctx, rows):
    """6. Compact row r of a striped dispatch is row y(r) of the full-frame planes: whole-tile
    stripes, stripes that cut through tiles, and a last stripe off the frame."""
    y0, stripe, period, out_rows = rows
    ref = gr.reference("cfg3", W0, H0, 0)
    inside = gr.dispatch_rows(H0, y0, stripe, period, out_rows)
    assert 0 < len(inside) and (len(inside) < out_rows) == (rows == (8, 8, 24, 24))
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, tr.scene("cfg3"), kernel=kernel)
        raw = dispatch(ctx, W0, H0, y0, stripe, period, out_rows, extra=1)
        expect(raw, ref, W0, f"stripes {rows} kernel {kernel}", rows=inside)
        untouched = sorted(set(range(out_rows + 1)) - {r for r, _ in inside})
        for p, b in raw.items():
            assert (b[untouched] == FILL).all(), (rows, kernel, p)
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("path", ["animate", "update"])
@pytest.mark.parametrize("mt", [0, 1])
def test_animated_scene_is_seen_without_a_dispatch(ctx, mt, path):
    """7. The car's wheels moved (rt_animate, or rt_update_shapes + rt_update_nodes), then a
    geometry buffer with no frame in between: the reference over the moved shapes and
    updateBVH's nodes, after exactly one refit."""
    fs = tr.scene("cfg3")
    host = gr.scene("cfg3:anim")
    ids, rec = gr.wheel_move()
    W, H = gr.WA, gr.HA
    ref, still = gr.reference("cfg3:anim", W, H, mt), gr.reference("cfg3", W, H, mt)
    assert (ref["shape"] != still["shape"]).any()  # the move matters to this frame: a stale scene would be seen
    prepare(ctx, fs, mt, W, H)
    expect(dispatch(ctx, W, H), still, W, f"before the move mt {mt}")  # Moller-Trumbore: its accelerator exists from here on
    r0 = ctx.debug_refits()
    if path == "animate":
        ctx.set_animated(ids)
        ctx.animate(rec)
    else:
        ctx.update_shapes(int(ids[0]), rec)  # the wheels' records are contiguous
        ctx.update_nodes(host.nodes)
        assert ctx.debug_refits() == r0  # pending until something reads the device scene
    expect(dispatch(ctx, W, H), ref, W, f"animated mt {mt} {path}")
    assert ctx.debug_refits() == r0 + 1
    ctx.set_kernel(rtamd.KERNEL_LANE)
    expect(dispatch(ctx, W, H), ref, W, f"animated mt {mt} {path} literal")
    assert ctx.debug_refits() == r0 + 1
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_animated(np.zeros(0, np.int32))


def test_the_renderer_is_left_alone(ctx):
    """8. Geometry buffers between two adaptively supersampled frames: last_kernel, the record
    of rt_kernel_times, rt_adaptive_stats and the surface stay as the frame left them, the next
    frame is byte-identical, and the buffer is the one taken with rt_set_samples(1)."""
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
            host = ctx.gbuffer(W0, H0)
            for p in gr.PLANES:
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


def test_arguments(ctx):
    """9. Every RT_ERR_INVALID case of rt_api.h against pre-filled planes that stay untouched;
    RT_ERR_NO_SCENE before the upload, without a camera and without params; out_rows == 0; an
    empty scene. All refusals happen on the host: no bad pointer reaches a kernel."""
    lib = rtamd.rt_lib()
    fs = tr.scene("cfg3")
    W, H = W0, H0
    P = lambda a: a.ctypes.data  # noqa: E731
    host = {p: np.full((H, W * PX[p]), FILL, np.uint8) for p in gr.PLANES}

    def gbuf(planes, **over):
        g = rtamd.rt_gbuffer()
        for p, (ptr, pitch) in planes.items():
            setattr(g, p, ptr)
            setattr(g, p + "_pitch", pitch)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    hostg = {p: (P(a), W * PX[p]) for p, a in host.items()}
    fresh = rtamd.ComputeShader(0)
    try:
        assert lib.rt_gbuffer_host(fresh._h, W, H, C.byref(gbuf(hostg))) == -4
        assert lib.rt_dispatch_gbuffer(fresh._h, W, H, 0, 1, 1, H, C.byref(gbuf(hostg))) == -4
        assert lib.rt_gbuffer_host(fresh._h, W, H, None) == -1
        rc = lib.rt_upload_scene(fresh._h, C.c_void_p(P(fs.shapes)), len(fs.shapes), C.c_void_p(P(fs.nodes)),
                                 len(fs.nodes), C.c_void_p(P(fs.indices)), len(fs.indices))
        assert rc == 0
        assert lib.rt_gbuffer_host(fresh._h, W, H, C.byref(gbuf(hostg))) == -4  # neither camera nor params
        fresh.set_params(W, H)
        assert lib.rt_gbuffer_host(fresh._h, W, H, C.byref(gbuf(hostg))) == -4  # no camera
        assert all((a == FILL).all() for a in host.values())
    finally:
        fresh.close()
    fresh = rtamd.ComputeShader(0)
    try:
        fresh.upload(fs)  # scene, camera and light
        assert lib.rt_gbuffer_host(fresh._h, W, H, C.byref(gbuf(hostg))) == -4  # no params
        assert all((a == FILL).all() for a in host.values())
        fresh.set_params(W, H)
        assert lib.rt_gbuffer_host(fresh._h, W, H, C.byref(gbuf(hostg))) == 0
        ref = gr.reference("cfg3", W, H, 0)
        expect(host, ref, W, "host form of a fresh context")
    finally:
        fresh.close()
    for arr in host.values():
        arr[:] = FILL  # the refusals below must leave them so

    prepare(ctx, fs)
    dev = {p: torch.full((H * W * PX[p] + 64,), FILL, dtype=torch.uint8, device="cuda") for p in gr.PLANES}
    torch.cuda.synchronize()
    ok = {p: (t.data_ptr(), W * PX[p]) for p, t in dev.items()}
    assert all(ptr % 16 == 0 for ptr, _ in ok.values())
    big = {p: (ptr, 65536 * 16) for p, (ptr, _) in ok.items()}  # pitches that pass for any width tried below
    call = lambda g, w=W, h=H, y0=0, stripe=1, period=1, rows=H: lib.rt_dispatch_gbuffer(  # noqa: E731
        ctx._h, w, h, y0, stripe, period, rows, C.byref(g) if g is not None else None)
    invalid = [
        ("out NULL", lambda: call(None)),
        ("all planes NULL", lambda: call(gbuf({}))),
        ("all planes NULL, pitches set", lambda: call(gbuf({}, shape_pitch=4 * W, normal_pitch=16 * W))),
        ("width 0", lambda: call(gbuf(ok), w=0)),
        ("width < 0", lambda: call(gbuf(ok), w=-W)),
        ("height 0", lambda: call(gbuf(ok), h=0)),
        ("height < 0", lambda: call(gbuf(ok), h=-1)),
        ("y0 < 0", lambda: call(gbuf(ok), y0=-1)),
        ("stripe 0", lambda: call(gbuf(ok), stripe=0, period=0)),
        ("stripe < 0", lambda: call(gbuf(ok), stripe=-1)),
        ("out_rows < 0", lambda: call(gbuf(ok), rows=-1)),
        ("period < stripe", lambda: call(gbuf(ok), stripe=8, period=7)),
        ("too many tile rows", lambda: call(gbuf(big), w=1, h=10, rows=8 * 65535 + 1)),
        ("width * out_rows = 2^32", lambda: call(gbuf(big), w=65536, h=10, rows=65536)),
    ]
    for p in gr.PLANES:
        ptr, pitch = ok[p]
        a = PX[p]
        invalid += [
            (f"{p} pitch short", lambda p=p, ptr=ptr, pitch=pitch, a=a: call(gbuf({**ok, p: (ptr, pitch - a)}))),
            (f"{p} pitch unaligned", lambda p=p, ptr=ptr, pitch=pitch, a=a: call(gbuf({**ok, p: (ptr, pitch + a // 2)}))),
            (f"{p} pointer unaligned", lambda p=p, ptr=ptr, pitch=pitch, a=a: call(gbuf({**ok, p: (ptr + a // 2, pitch)}))),
            (f"{p} alone, pitch short", lambda p=p, ptr=ptr, pitch=pitch, a=a: call(gbuf({p: (ptr, pitch - a)}))),
        ]
    for what, fn in invalid:
        assert fn() == -1, what
    # the host form checks the same way
    for g in (None, gbuf({}), gbuf({**hostg, "depth": (hostg["depth"][0], 4 * W - 4)}),
              gbuf({**hostg, "normal": (hostg["normal"][0] + 8, 16 * W)})):
        assert lib.rt_gbuffer_host(ctx._h, W, H, C.byref(g) if g is not None else None) == -1
    assert lib.rt_gbuffer_host(ctx._h, 0, H, C.byref(gbuf(hostg))) == -1
    assert lib.rt_gbuffer_host(ctx._h, W, -1, C.byref(gbuf(hostg))) == -1
    # out_rows == 0: RT_OK, nothing launched
    assert call(gbuf(ok), rows=0) == 0
    ctx.sync()
    assert all((t.cpu().numpy() == FILL).all() for t in dev.values())  # none of these calls wrote a byte
    assert all((a == FILL).all() for a in host.values())

    import test_gpu_parity as tg
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, tg._empty_scene(W, H), kernel=kernel)
        raw = dispatch(ctx, W, H)
        assert (typed(raw["shape"], "shape", W) == -1).all()
        assert (bits(typed(raw["depth"], "depth", W)) == bits(np.float32(1e20))).all()
        assert not raw["normal"].any() and not raw["position"].any()
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def test_ties_go_to_the_first_in_walk_order(ctx):
    """10. Every shape twice (tests/test_accel_cpu.py::test_accel_ties): each hit is a two-way
    tie, and `shape` is the first in the reference's walk order, as the oracle says."""
    fs2 = gr.scene("cfg3:ties")
    ref, single = gr.reference("cfg3:ties", W0, H0, 0), gr.reference("cfg3", W0, H0, 0)
    S = len(tr.scene("cfg3").shapes)
    hit = ref["shape"] >= 0
    assert hit.sum() > 500 and np.array_equal(hit, single["shape"] >= 0)
    assert np.array_equal(ref["shape"][hit] % S, single["shape"][hit])
    assert np.array_equal(bits(ref["depth"]), bits(single["depth"]))
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, fs2, kernel=kernel)
        expect(dispatch(ctx, W0, H0), ref, W0, f"ties kernel {kernel}")
    ctx.set_kernel(rtamd.KERNEL_AUTO)
