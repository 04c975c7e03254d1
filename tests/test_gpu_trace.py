"""Ray queries on the device (rt_trace_rays / rt_trace_rays_host / rt_trace_pixels): every ray
of tests/trace_rays.py gets the oracle's reference-walk answer (orc_trace_rays_mt) -- shape
and occlusion exactly, distance bit for bit -- from the accelerated walk (k_trace) and from
the literal walk (k_trace_ref), barycentric and Moller-Trumbore, over the scene tree and the
reference tree. tests/test_trace_cpu.py shows on the CPU that these inputs are ones for which
the accelerated walk and the reference agree.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bench
import oracle
import rtamd
import trace_rays as tr

pytestmark = pytest.mark.gpu
TOL = 1e-4  # frames against the oracle, as tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


def prepare(ctx, fs, mt=False, W=tr.CAM_W, H=tr.CAM_H, kernel=rtamd.KERNEL_AUTO, tree=rtamd.TREE_SCENE):
    ctx.upload(fs)
    ctx.set_animated(np.zeros(0, np.int32))
    ctx.set_params(W, H, 3, True, False, mt)
    ctx.set_kernel(kernel)
    ctx.set_tree(tree)


def device_hits(ctx, rays, mode, extra=0, fill=0xAB):
    """rt_trace_rays on torch buffers: the hit records as raw bytes [n + extra, 16], the
    buffer pre-filled with `fill`."""
    n = len(rays)
    r = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    h = torch.full(((n + extra) * 16,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the context's stream does not wait on torch's
    ctx.trace_rays_device(r.data_ptr() if n else 0, n, h.data_ptr(), mode)
    ctx.sync()
    return h.cpu().numpy().reshape(n + extra, 16)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expect(got, want, lim, what, any_hit=False):
    """got = (shape, distance, occluded) of a query, want the oracle's: every ray, exactly."""
    shape, dist, occ = got
    oshape, odist, oshadow = want
    assert len(shape) == len(oshape), what
    bad = np.where(occ != oshadow)[0]
    assert bad.size == 0, f"{what}: {bad.size} occlusion mismatches, e.g. ray {bad[0]}"
    if any_hit:
        assert (shape == -1).all() and (bits(dist) == bits(np.float32(1e20))).all(), what
        return
    bad = np.where(shape != oshape)[0]
    assert bad.size == 0, f"{what}: {bad.size} shape mismatches, e.g. ray {bad[0]}: {shape[bad[0]]} vs {oshape[bad[0]]}"
    bad = np.where(bits(dist) != bits(odist))[0]
    assert bad.size == 0, (f"{what}: {bad.size} distances differ in their bits, e.g. ray {bad[0]}: "
                           f"{dist[bad[0]]!r} vs {odist[bad[0]]!r}")


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_exact_against_the_oracle(ctx, name, mt):
    """1. Closest mode returns the oracle's shape, distance bits and shadow answer for every ray
    of every set; any mode the shadow answer. Both tree modes."""
    fs = tr.scene(name)
    o, d, lim = tr.all_rays(name)
    want = tr.oracle_all(name, mt)
    for tree in (rtamd.TREE_SCENE, rtamd.TREE_REFERENCE):
        prepare(ctx, fs, mt, tree=tree)
        expect(ctx.trace_rays(o, d, lim), want, lim, f"{name} mt {mt} tree {tree} closest")
        expect(ctx.trace_rays(o, d, lim, any_hit=True), want, lim, f"{name} mt {mt} tree {tree} any", any_hit=True)
        info = ctx.accel_info()
        assert info["built"] == 1 and info["scene_tree"] == 1
    ctx.set_tree(rtamd.TREE_SCENE)


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_literal_walk_gives_the_same_bytes(ctx, name, mt):
    """2. Device A/B: rt_set_kernel(RT_KERNEL_LANE) answers the same rays through the literal
    reference walk; the hit buffers are byte-identical (and equal the oracle)."""
    fs = tr.scene(name)
    o, d, lim = tr.all_rays(name)
    rays = ctx.make_rays(o, d, lim)
    want = tr.oracle_all(name, mt)
    for mode in (rtamd.TRACE_CLOSEST, rtamd.TRACE_ANY):
        prepare(ctx, fs, mt)
        fast = device_hits(ctx, rays, mode)
        ctx.set_kernel(rtamd.KERNEL_LANE)
        literal = device_hits(ctx, rays, mode)
        ctx.set_kernel(rtamd.KERNEL_PACKET)
        packet = device_hits(ctx, rays, mode)
        assert np.array_equal(fast, literal), f"{name} mt {mt} mode {mode}: accelerated and literal hits differ"
        assert np.array_equal(packet, literal)
        h = np.ascontiguousarray(literal).view(rtamd.HIT_DTYPE).reshape(-1)
        assert (h["reserved"] == 0).all()
        expect((h["shape"], h["distance"], h["occluded"]), want, lim, f"{name} literal mode {mode}",
               any_hit=mode == rtamd.TRACE_ANY)
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE])
def test_wave_and_block_edges(ctx, kernel):
    """3. Prefixes of one ray set on the car, around the wave (64) and the literal kernel's block
    (256): the common prefix's hits are identical, the record after the last ray is untouched."""
    o, d, lim = tr.all_rays("cfg3")
    pick = np.random.default_rng(3).permutation(len(o))[:4097]
    rays = ctx.make_rays(o[pick], d[pick], lim[pick])
    prepare(ctx, tr.scene("cfg3"), kernel=kernel)
    for mode in (rtamd.TRACE_CLOSEST, rtamd.TRACE_ANY):
        full = device_hits(ctx, rays, mode, extra=1)
        assert (full[-1] == 0xAB).all()
        for n in (1, 63, 64, 65, 255, 256, 257):
            part = device_hits(ctx, rays[:n], mode, extra=1, fill=0x5C)
            assert np.array_equal(part[:n], full[:n]), (kernel, mode, n)
            assert (part[n] == 0x5C).all(), (kernel, mode, n)
        # n = 0: RT_OK, nothing written
        assert (device_hits(ctx, rays[:0], mode, extra=1) == 0xAB).all()
    s, dist, occ = ctx.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(s) == len(dist) == len(occ) == 0
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def test_ties_go_to_the_first_in_walk_order(ctx):
    """4. Every shape twice (tests/test_accel_cpu.py::test_accel_ties): equal distances, and the
    first shape the reference walk finds wins, as the oracle says."""
    fs = tr.scene("cfg3")
    shapes = np.concatenate([fs.shapes, fs.shapes.copy()])
    nodes, idx = oracle.build_bvh(shapes, 25)
    fs2 = rtamd.FlatScene(shapes, nodes, idx, fs.camera, fs.light)
    o, d = tr.ray_sets("cfg3")["camera"]
    lim = np.full(len(o), 50.0, np.float32)
    want = tr.oracle_trace(fs2, o, d, lim, 0)
    # every hit is a two-way tie: the single scene's winner or its copy, at the same distance
    S, n = len(fs.shapes), len(o)
    single = tr.oracle_all("cfg3", 0)  # the camera set comes first in all_rays
    hit = want[0] >= 0
    assert hit.sum() > 500 and np.array_equal(hit, single[0][:n] >= 0)
    assert np.array_equal(want[0][hit] % S, single[0][:n][hit]) and np.array_equal(bits(want[1]), bits(single[1][:n]))
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, fs2, kernel=kernel)
        expect(ctx.trace_rays(o, d, lim), want, lim, f"ties kernel {kernel}")
    ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("path", ["animate", "update"])
@pytest.mark.parametrize("mt", [0, 1])
def test_animated_scene_is_seen_without_a_dispatch(ctx, mt, path):
    """5. The car's wheels moved (rt_animate, or the reference's own rt_update_shapes +
    rt_update_nodes), then a query with no dispatch in between: the oracle's answers over the
    moved shapes and updateBVH's nodes, after one refit; the frame after it matches the oracle
    frame and refits nothing again."""
    W, H = 160, 90
    fs = rtamd.generate(3, 0, W, H)
    ids, frames = bench.wheel_frames(fs, 30)
    rec = frames[-1]  # half a radian
    host = rtamd.FlatScene(fs.shapes.copy(), fs.nodes.copy(), fs.indices, fs.camera, fs.light)
    host.shapes[ids] = rec
    oracle.update_bvh(host, ids)
    # the shared rays, and rays aimed at the moved triangles
    o, d, lim = tr.all_rays("cfg3")
    rng = np.random.default_rng(5)
    k = rng.integers(0, len(ids), 2000)
    tgt = (rec["triP1"][k].astype(np.float64) + rec["triP2"][k] + rec["triP3"][k]) / 3
    src = tgt + rng.normal(size=(2000, 3)) * 8
    o = np.concatenate([o, src.astype(np.float32)])
    d = np.concatenate([d, ((tgt - src) / np.linalg.norm(tgt - src, axis=1, keepdims=True)).astype(np.float32)])
    lim = np.concatenate([lim, rng.uniform(1, 40, 2000).astype(np.float32)])
    want = tr.oracle_trace(host, o, d, lim, mt)
    still = tr.oracle_trace(fs, o, d, lim, mt)
    assert (want[0] != still[0]).sum() > 100  # the move matters to these rays

    prepare(ctx, fs, mt, W, H)
    ctx.trace_rays(o[:64], d[:64], lim[:64])  # Moller-Trumbore: its accelerator exists from here on, and refits
    r0 = ctx.debug_refits()
    if path == "animate":
        ctx.set_animated(ids)
        ctx.animate(rec)
    else:
        ctx.update_shapes(int(ids[0]), rec)  # the wheels' records are contiguous
        ctx.update_nodes(host.nodes)
        assert ctx.debug_refits() == r0  # pending until something reads the device scene
    expect(ctx.trace_rays(o, d, lim), want, lim, f"animated mt {mt} {path} closest")
    assert ctx.debug_refits() == r0 + 1
    expect(ctx.trace_rays(o, d, lim, any_hit=True), want, lim, f"animated mt {mt} {path} any", any_hit=True)
    img = ctx.render(W, H)
    ref, _ = oracle.render(host, W, H, oracle.params(W, H, 3, True, False, mt))
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    assert int((diff > TOL).any(axis=-1).sum()) == 0, float(diff.max())
    assert ctx.debug_refits() == r0 + 1
    ctx.set_animated(np.zeros(0, np.int32))


@pytest.mark.parametrize("mt", [0, 1])
def test_picking(ctx, mt):
    """6. rt_trace_pixels for 500 random pixels and the four corners of a 160x90 car frame: the
    oracle's answer for the reference's camera ray of each pixel (NDC in float32, as the shader
    computes it); pixels it calls a miss hold exactly the background in the rendered frame."""
    W, H = 160, 90
    fs = rtamd.generate(3, 0, W, H)
    prepare(ctx, fs, mt, W, H)
    rng = np.random.default_rng(9)
    xy = np.stack([rng.integers(0, W, 500), rng.integers(0, H, 500)], 1)
    xy = np.concatenate([xy, [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]]).astype(np.int32)
    o, d = tr.pixel_rays(fs, W, H, xy)
    lim = np.full(len(o), np.inf, np.float32)
    want = tr.oracle_trace(fs, o, d, lim, mt)
    got = ctx.trace_pixels(W, H, xy)
    expect(got, want, lim, f"picking mt {mt}")
    miss = got[0] < 0
    assert 20 < miss.sum() < len(xy) - 20 and np.array_equal(got[2], (~miss).astype(np.int32))
    img = ctx.render(W, H)
    f = np.float32
    a = xy[miss, 1].astype(np.float32) / f(H)
    lo, hi = np.array([0.05, 0.07, 0.1], np.float32), np.array([0.5, 0.7, 1.0], np.float32)
    bg = lo[None, :] + a[:, None] * (hi - lo)[None, :]  # gpu_shader.comp:436, mix() in float32
    px = img[xy[miss, 1], xy[miss, 0]]
    assert np.array_equal(bits(px[:, :3]), bits(bg)) and (px[:, 3] == 1.0).all()
    # with the literal walk too
    ctx.set_kernel(rtamd.KERNEL_LANE)
    expect(ctx.trace_pixels(W, H, xy), want, lim, f"picking literal mt {mt}")
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    for bad in ((W, 0), (0, H), (-1, 3), (3, -1)):
        with pytest.raises(rtamd.RTError) as e:
            ctx.trace_pixels(W, H, [[1, 1], bad])
        assert e.value.code == -1


def test_queries_leave_the_renderer_alone(ctx):
    """7. Queries between two frames: rt_accel_info::last_kernel, the record of rt_kernel_times /
    rt_last_kernel_ms and the tile cost order stay as the frame left them, and the next frame
    is byte-identical."""
    W, H = 160, 90
    fs = rtamd.generate(3, 0, W, H)
    prepare(ctx, fs, False, W, H)
    ctx.kernel_times()
    first = ctx.render(W, H)
    before = ctx.accel_info()["last_kernel"], ctx.last_kernel_ms()
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    order = ctx.debug_sched_order(tiles)
    assert before[0] == rtamd.KERNEL_ACCEL and len(order) == tiles
    o, d, lim = tr.all_rays("cfg3")
    xy = np.stack(np.meshgrid(np.arange(0, W, 7), np.arange(0, H, 5)), -1).reshape(-1, 2)
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        ctx.set_kernel(kernel)
        ctx.trace_rays(o, d, lim)
        ctx.trace_rays(o, d, lim, any_hit=True)
        ctx.trace_pixels(W, H, xy)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    assert (ctx.accel_info()["last_kernel"], ctx.last_kernel_ms()) == before
    times = ctx.kernel_times()
    assert len(times) == 1 and times[0] == np.float32(before[1])  # the frame's dispatch, nothing else
    assert np.array_equal(ctx.debug_sched_order(tiles), order)
    ctx.sync_frame()
    second = ctx.render(W, H)
    assert np.array_equal(bits(first), bits(second))
    assert len(ctx.kernel_times()) == 1


def test_arguments(ctx):
    """8. Bad arguments answer RT_ERR_INVALID and launch nothing; a query before the upload
    RT_ERR_NO_SCENE (rt_trace_pixels also without a camera or params); an empty scene answers
    every ray with a miss."""
    lib = rtamd.rt_lib()
    fs = tr.scene("cfg3")
    o, d, lim = (a[:100] for a in tr.all_rays("cfg3"))
    rays = ctx.make_rays(o, d, lim)
    host_hits = np.zeros(100, rtamd.HIT_DTYPE)
    xy = np.zeros((100, 2), np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    fresh = rtamd.ComputeShader(0)
    try:
        assert lib.rt_trace_rays_host(fresh._h, P(rays), 100, P(host_hits), 0) == -4
        assert lib.rt_trace_pixels(fresh._h, 96, 54, P(xy), 100, P(host_hits)) == -4
        assert lib.rt_trace_rays_host(fresh._h, P(rays), -1, P(host_hits), 0) == -1
        # a scene, but neither camera nor params: rays are answered, pixels are not
        rc = lib.rt_upload_scene(fresh._h, P(fs.shapes), len(fs.shapes), P(fs.nodes), len(fs.nodes), P(fs.indices),
                                 len(fs.indices))
        assert rc == 0
        assert lib.rt_trace_rays_host(fresh._h, P(rays), 100, P(host_hits), 0) == 0
        want = tr.oracle_trace(fs, o, d, lim, 0)
        expect((host_hits["shape"], host_hits["distance"], host_hits["occluded"]), want, lim, "no params: barycentric")
        assert lib.rt_trace_pixels(fresh._h, 96, 54, P(xy), 100, P(host_hits)) == -4
        fresh.set_camera(fs.camera)
        assert lib.rt_trace_pixels(fresh._h, 96, 54, P(xy), 100, P(host_hits)) == -4
        fresh.set_params(96, 54)
        assert lib.rt_trace_pixels(fresh._h, 96, 54, P(xy), 100, P(host_hits)) == 0
    finally:
        fresh.close()

    prepare(ctx, fs)
    r = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    r4 = torch.zeros(len(r) + 16, dtype=torch.uint8, device="cuda")
    h = torch.full((101 * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dr, dh = r.data_ptr(), h.data_ptr()
    assert dr % 16 == 0 and dh % 16 == 0 and r4.data_ptr() % 16 == 0
    V = C.c_void_p
    for args in ((None, 100, V(dh), 0), (V(dr), 100, None, 0), (V(dr), -1, V(dh), 0), (V(dr), 100, V(dh), 2),
                 (V(dr), 100, V(dh), -1), (V(r4.data_ptr() + 4), 100, V(dh), 0), (V(dr), 100, V(dh + 4), 0),
                 (V(dr), 100, V(dh + 4), 1)):
        assert lib.rt_trace_rays(ctx._h, *args) == -1, args
    for args in ((None, 100, P(host_hits), 0), (P(rays), 100, None, 1), (P(rays), -5, P(host_hits), 0),
                 (P(rays), 100, P(host_hits), 7)):
        assert lib.rt_trace_rays_host(ctx._h, *args) == -1, args
    for args in ((96, 54, None, 100, P(host_hits)), (96, 54, P(xy), 100, None), (96, 54, P(xy), -1, P(host_hits)),
                 (0, 54, P(xy), 100, P(host_hits)), (96, -3, P(xy), 100, P(host_hits))):
        assert lib.rt_trace_pixels(ctx._h, *args) == -1, args
    assert lib.rt_trace_rays(ctx._h, None, 0, None, 0) == 0
    assert lib.rt_trace_rays_host(ctx._h, None, 0, None, 1) == 0
    assert lib.rt_trace_pixels(ctx._h, 96, 54, None, 0, None) == 0
    ctx.sync()
    assert (h.cpu().numpy() == 0xAB).all()  # none of the refused calls wrote a hit

    import test_gpu_parity as tg
    for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
        prepare(ctx, tg._empty_scene(96, 54), kernel=kernel)
        for any_hit in (False, True):
            s, dist, occ = ctx.trace_rays(o, d, lim, any_hit=any_hit)
            assert (s == -1).all() and (bits(dist) == bits(np.float32(1e20))).all() and (occ == 0).all()
        s, dist, occ = ctx.trace_pixels(96, 54, xy)
        assert (s == -1).all() and (occ == 0).all()
    ctx.set_kernel(rtamd.KERNEL_AUTO)
