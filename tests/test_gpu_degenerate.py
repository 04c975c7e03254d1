"""Degenerate and non-finite shape records on the device (-m gpu; needs an MI355X).

The scenes of tests/degenerate_scenes.py -- NaN, infinite and 3e38 coordinates, zero and negative
radii, zero-area triangles, stored planes scaled, shifted and tilted to the classify thresholds,
walls without a basis or an extent, unknown types, magnitudes that overflow -- through every query
form: frames of the three render kernels against the oracle, the walk switches, ray queries,
geometry buffers, ambient occlusion, shaded rays, supersampled and display-format frames, and the
refit into and out of each class (rt_animate, and rt_update_shapes + rt_update_nodes).
Every dispatch is 60x44, which is off the 8x8 tile grid in x and y. Frames are compared with
tests/frame_check.py, which sees a NaN the oracle does not have. tests/test_degenerate_cpu.py
shows on the CPU that these inputs are ones for which the accelerated walk's rules hold.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ao_ref as ar
import degenerate_scenes as dg
import fmt_ref
import gbuffer_ref as gr
import oracle
import rtamd
import ss_ref
import trace_rays as tr
from frame_check import close_to_oracle, same_frame

pytestmark = pytest.mark.gpu
TOL = 1e-4  # BASELINE.json north_star, as tests/test_gpu_parity.py
W, H = dg.W, dg.H
KERNELS = (rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET, rtamd.KERNEL_LANE)
KNAME = {rtamd.KERNEL_ACCEL: "accel", rtamd.KERNEL_PACKET: "packet", rtamd.KERNEL_LANE: "lane"}
# (maxBounces, useBVH, fresnel, mt)
PLAIN = (3, 1, 0, 0)
FRAME_PARAMS = (PLAIN, (3, 1, 1, 1), (3, 0, 0, 0), (2, 0, 1, 1))
ACCEL_OF = {(1, 0): "own", (1, 1): "mtc", (0, 0): "brute", (0, 1): None}  # by (useBVH, mt)
SEED = dg.SEEDS[0]  # the tests that run one seed
CASES = [(f, s, d) for f in dg.FAMILIES for s in dg.SEEDS for d in dg.DEPTHS]
ONE_SEED = [(f, SEED, d) for f in dg.FAMILIES for d in dg.DEPTHS]
ids_of = lambda cases: ["%s-s%d-d%d" % c for c in cases]  # noqa: E731
POISON = -7.0  # no pixel of a frame: an unwritten one fails every comparison


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """A second context, for "the same arrays uploaded whole"."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


def load(c, fs, params=PLAIN, kernel=rtamd.KERNEL_AUTO):
    c.upload(fs)
    c.set_animated(np.zeros(0, np.int32))
    c.set_params(W, H, *params)
    c.set_kernel(kernel)
    c.set_tree(rtamd.TREE_SCENE)
    c.set_samples(1)


def frame(c, w=W, h=H):
    """rt_dispatch_rows of the whole frame into a poisoned surface."""
    out = torch.full((h, w, 4), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # the renderer's stream does not wait on torch's
    c.dispatch_rows(w, h, 0, 1, 1, h, out.data_ptr(), w * 16)
    c.sync()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def oracle_frame(case, params):
    img, _ = oracle.render(dg.scene(*case), W, H, oracle.params(W, H, *params))
    img.setflags(write=False)
    return img


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def built(c, which, family):
    """Whether the accelerator a frame or query of this kind walks exists: the context's own
    ("own"), its Moller-Trumbore ("mtc") or its brute-force ("brute") sub-context's. Only the huge
    scenes may be without one."""
    ok = c.accel_info()["built"] == 1 if which == "own" else c.debug_accel_dump(which)["built"] == 1
    assert ok or family == "huge", f"{family}: no accelerator was built ({which})"
    return ok


def rebuild_state(c):
    fn = c._lib.rt_debug_rebuild_state
    fn.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(4, np.int32)
    assert fn(c._h, out.ctypes.data) == 0
    return dict(zip(["running", "requested", "swapped", "suspended"], out.tolist()))


def settle(c):
    """Lets every rebuild that the refits so far ask for start, finish and land. The rebuild runs
    on a host thread (the default, rt_debug_async_rebuild 1), and a request is only seen by a
    flush after the k_refit that reports it has run, so how many flushes that takes depends on
    the thread. Each round waits for the stream (the refits have run, their reports can be read)
    and flushes (rt_accel_info_get: reads the reports, which may start a rebuild, and lands a
    finished one, whose refit may report again). Done after two rounds in a row with no rebuild
    pending; the records do not change meanwhile, so the rebuild that lands last was built from
    them and its refit reports nothing."""
    quiet = 0
    for _ in range(10000):
        c.sync()
        c.accel_info()
        quiet = 0 if rebuild_state(c)["running"] else quiet + 1
        if quiet == 2:
            return
    raise AssertionError(f"the rebuilds do not come to rest: {rebuild_state(c)}")


def same_floats(got, want, what):
    """Bit for bit, but for NaN, which only has to be NaN in both."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} values differ, first at {at}: {got[at]!r} vs {want[at]!r}")


# --------------------------------------------------------------------------
# 1. Frames against the oracle, the three kernels against each other

@pytest.mark.parametrize("case", CASES, ids=ids_of(CASES))
def test_frames_match_the_oracle(ctx, case):
    load(ctx, dg.scene(*case))
    for params in FRAME_PARAMS:
        ref = oracle_frame(case, params)
        ctx.set_params(W, H, *params)
        imgs = {}
        for k in KERNELS:
            ctx.set_kernel(k)
            imgs[k] = frame(ctx)
            what = f"{case} params {params} kernel {KNAME[k]}"
            if k == rtamd.KERNEL_ACCEL:
                # what was compared: the accelerated kernel, but for a huge scene whose accelerator
                # (the context's own, or the sub-context's of the brute or the Moller-Trumbore
                # branch) could not be built; the brute branch's own MT sub-context is not exposed
                last = ctx.accel_info()["last_kernel"]
                which = ACCEL_OF[params[1], params[3]]
                if case[0] != "huge" or (which is not None and built(ctx, which, case[0])):
                    assert last == rtamd.KERNEL_ACCEL, what
            close_to_oracle(imgs[k], ref, TOL, what)
        for k in (rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET):
            same_frame(imgs[k], imgs[rtamd.KERNEL_LANE], f"{case} params {params}: {KNAME[k]} vs lane")
    ctx.set_kernel(rtamd.KERNEL_AUTO)


# --------------------------------------------------------------------------
# 2. The walk switches render the default frame

@pytest.mark.parametrize("family", dg.FAMILIES)
def test_switches_render_the_default_frame(ctx, family):
    case = (family, SEED, 1)
    load(ctx, dg.scene(*case), kernel=rtamd.KERNEL_ACCEL)
    default = frame(ctx)
    close_to_oracle(default, oracle_frame(case, PLAIN), TOL, f"{case} default switches")
    try:
        ctx.set_tree(rtamd.TREE_REFERENCE)
        same_frame(frame(ctx), default, f"{case} reference tree")
        ctx.set_tree(rtamd.TREE_SCENE)
        for walk in (0, 1, 99):
            ctx.set_walk(walk)
            same_frame(frame(ctx), default, f"{case} walk {walk}")
        ctx.set_walk(-1)
        for tail in (0, 2):
            ctx.set_tail(tail)
            same_frame(frame(ctx), default, f"{case} tail {tail}")
        ctx.set_tail(-1)
        ctx.set_latency_mode(1)
        for i in range(2):  # the second frame runs with the first one's cost order
            same_frame(frame(ctx), default, f"{case} latency mode, frame {i}")
    finally:
        ctx.set_tree(rtamd.TREE_SCENE)
        ctx.set_walk(-1)
        ctx.set_tail(-1)
        ctx.set_latency_mode(0)
        ctx.set_kernel(rtamd.KERNEL_AUTO)


# --------------------------------------------------------------------------
# 3. Ray queries

@pytest.mark.parametrize("case", CASES, ids=ids_of(CASES))
def test_ray_queries_match_the_oracle(ctx, case):
    """rt_trace_rays over the camera and random rays, accelerated (k_trace) and literal
    (k_trace_ref), barycentric and Moller-Trumbore: the oracle's shape, distance (bit for bit,
    NaN for NaN) and occlusion answer for every ray. rt_trace_rays takes k_trace exactly when the
    kernel is RT_KERNEL_AUTO and the accelerator of the triangle test exists (it records no
    last_kernel), so the test asserts that it exists."""
    o, d, lim = dg.rays(case[0], case[1])
    fs = dg.scene(*case)
    try:
        for mt in (0, 1):
            want = tr.oracle_trace(fs, o, d, lim, mt)
            load(ctx, fs, (3, 1, 0, mt))
            for kernel in (rtamd.KERNEL_AUTO, rtamd.KERNEL_LANE):
                ctx.set_kernel(kernel)
                what = f"{case} mt {mt} kernel {kernel}"
                shape, dist, occ = ctx.trace_rays(o, d, lim)
                assert len(shape) == len(dist) == len(occ) == len(o), what
                bad = np.where(shape != want[0])[0]
                assert bad.size == 0, f"{what}: {bad.size} shapes differ, e.g. ray {bad[0]}: {shape[bad[0]]} vs {want[0][bad[0]]}"
                same_floats(dist, want[1], f"{what} distance")
                bad = np.where(occ != want[2])[0]
                assert bad.size == 0, f"{what}: {bad.size} occlusion answers differ, e.g. ray {bad[0]}"
                _, _, any_occ = ctx.trace_rays(o, d, lim, any_hit=True)
                bad = np.where(any_occ != want[2])[0]
                assert bad.size == 0, f"{what}: {bad.size} any-hit answers differ, e.g. ray {bad[0]}"
                if kernel == rtamd.KERNEL_AUTO:  # after a query: the Moller-Trumbore sub-context exists
                    built(ctx, "mtc" if mt else "own", case[0])
    finally:
        ctx.set_kernel(rtamd.KERNEL_AUTO)


# --------------------------------------------------------------------------
# 4. Geometry buffer and ambient occlusion

@pytest.mark.parametrize("case", ONE_SEED, ids=ids_of(ONE_SEED))
def test_gbuffer_and_ao_match_their_references(ctx, case):
    """rt_gbuffer_host's four planes against tests/gbuffer_ref.py and rt_ao_host (16 rays, radius
    2.0) against tests/ao_ref.py: integers for equality, floats bit for bit, NaN for NaN."""
    key = dg.key(*case)
    for mt in (0, 1):
        load(ctx, dg.scene(*case), (3, 1, 0, mt))
        ref = gr.reference(key, W, H, mt)
        got = ctx.gbuffer(W, H)
        assert np.array_equal(got["shape"], ref["shape"]), (
            f"{case} mt {mt}: {int((got['shape'] != ref['shape']).sum())} shapes differ")
        for plane in ("depth", "normal", "position"):
            same_floats(got[plane], ref[plane], f"{case} mt {mt} {plane}")
        want = ar.reference(key, W, H, mt, K=16, radius=2.0)
        ao = ctx.ao(W, H, 16, 2.0, ar.BIAS)
        bad = np.argwhere(ao["count"] != want["count"])
        assert bad.size == 0, (f"{case} mt {mt}: {len(bad)} ambient-occlusion counts differ, e.g. at {tuple(bad[0])}: "
                               f"{ao['count'][tuple(bad[0])]} vs {want['count'][tuple(bad[0])]}")
        same_floats(ao["visibility"], want["visibility"], f"{case} mt {mt} visibility")


# --------------------------------------------------------------------------
# 5. Shaded rays

@pytest.mark.parametrize("case", ONE_SEED, ids=ids_of(ONE_SEED))
def test_shaded_camera_rays_are_the_frame(ctx, case):
    """rt_shade_rays_host over rt_camera_rays_host of the frame gives rt_dispatch_rows' pixels."""
    for mt in (0, 1):
        load(ctx, dg.scene(*case), (3, 1, 0, mt))
        img = frame(ctx)
        rays = ctx.camera_rays(W, H)
        assert len(rays) == W * H
        px = ctx.shade_rays(rays, None)
        same_frame(px.reshape(H, W, 4), img, f"{case} mt {mt}: shaded camera rays vs the frame")
        close_to_oracle(img, oracle_frame(case, (3, 1, 0, mt)), TOL, f"{case} mt {mt}")


# --------------------------------------------------------------------------
# 6. Supersampling and display formats

@pytest.mark.parametrize("family", dg.FAMILIES)
def test_supersampled_frame_is_the_box_filter(ctx, family):
    """rt_set_samples(2): the box filter (tests/ss_ref.py) of the renderer's own 120x88 frame; a
    NaN sample makes its pixel NaN."""
    fs = dg.scene(family, SEED, 1)
    try:
        for kernel in (rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET):
            load(ctx, fs, kernel=kernel)
            ctx.set_params(2 * W, 2 * H, *PLAIN)
            want = ss_ref.box(frame(ctx, 2 * W, 2 * H), 2)
            ctx.set_params(W, H, *PLAIN)
            ctx.set_samples(2)
            same_frame(frame(ctx), want, f"{family} kernel {KNAME[kernel]}: 2x2 samples vs the box filter")
    finally:
        ctx.set_samples(1)
        ctx.set_kernel(rtamd.KERNEL_AUTO)


@pytest.mark.parametrize("family", dg.FAMILIES)
def test_display_formats_convert_the_float_frame(ctx, family):
    """RT_FORMAT_RGBA8 and RT_FORMAT_RGBA16F equal tests/fmt_ref.py of the float frame (NaN gives
    0 in RGBA8 and stays NaN in RGBA16F)."""
    load(ctx, dg.scene(family, SEED, 1), kernel=rtamd.KERNEL_ACCEL)
    try:
        img = frame(ctx)
        for fmt in (rtamd.FORMAT_RGBA8, rtamd.FORMAT_RGBA16F):
            px = fmt_ref.BYTES[fmt]
            out = torch.full((H, W * px), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.dispatch_rows_ex(W, H, 0, 1, 1, H, out.data_ptr(), W * px, fmt=fmt)
            ctx.sync()
            got = out.cpu().numpy().view(fmt_ref.DTYPE[fmt]).reshape(H, W, 4)
            want = fmt_ref.convert(img, fmt)
            if fmt == rtamd.FORMAT_RGBA16F:
                ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint16) == want.view(np.uint16))
            else:
                ok = got == want
            assert ok.all(), f"{family} format {fmt}: {int((~ok).any(axis=-1).sum())} pixels differ from fmt_ref"
    finally:
        ctx.set_kernel(rtamd.KERNEL_AUTO)


# --------------------------------------------------------------------------
# 7. Refit into and out of each class

def _check_nodes(c, host, what):
    got = c.read_nodes(len(host.nodes))
    for f in ("boundsMin", "boundsMax"):
        same_floats(got[f], host.nodes[f], f"{what}: {f} against updateBVH")
    for f in ("leftChild", "rightChild", "startShapeIdx", "numShapes"):
        assert np.array_equal(got[f], host.nodes[f]), f"{what}: {f}"


@pytest.mark.parametrize("path", ["animate", "update"])
@pytest.mark.parametrize("case", CASES, ids=ids_of(CASES))
def test_refit_into_and_out_of_each_class(ctx, fresh, case, path):
    """From the base scene: the family's records, the base records again, the family's records
    again -- by rt_animate (the device's updateBVH) or by rt_update_shapes + rt_update_nodes with
    oracle.update_bvh's boxes. After every step the nodes are updateBVH's (NaN for NaN), the
    accelerated and the packet frame are the oracle's of the updated scene, and both equal a fresh
    upload of the same arrays; those frames are rendered while the rebuild the step asks for may
    be running, landed or not yet asked for. Every family (all nine) changes the accel_bound.h
    class of at least one shape between its records and the base records
    (tests/test_degenerate_cpu.py::test_every_family_changes_a_class), so every step makes the host
    rebuild the accelerator: rt_debug_anim_rebuilds has risen once the step's rebuilds have landed
    (settle), and the frame through the rebuilt accelerator is the fresh upload's too."""
    family, seed, depth = case
    ids = dg.mutated_ids(family, seed)
    start = dg.base(seed, depth)
    records = (dg.scene(family, seed, depth).shapes[ids], start.shapes[ids].copy())
    host = rtamd.FlatScene(start.shapes.copy(), start.nodes.copy(), start.indices, start.camera, start.light)
    p = oracle.params(W, H, *PLAIN)
    load(ctx, start, kernel=rtamd.KERNEL_ACCEL)
    if path == "animate":
        ctx.set_animated(ids)
    frame(ctx)
    try:
        for step in range(3):
            what = f"{case} {path} step {step}"
            rebuilds = ctx.debug_anim_rebuilds()
            rec = records[step % 2]
            host.shapes[ids] = rec
            oracle.update_bvh(host, ids)
            if path == "animate":
                ctx.animate(rec)
            else:
                for i, r in zip(ids, rec):  # the reference's host: one upload per animated shape
                    ctx.update_shapes(int(i), host.shapes[i:i + 1])
                ctx.update_nodes(host.nodes)
            _check_nodes(ctx, host, what)
            want, _ = oracle.render(host, W, H, p)
            load(fresh, host, kernel=rtamd.KERNEL_ACCEL)
            for k in (rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET):
                ctx.set_kernel(k)
                fresh.set_kernel(k)
                img = frame(ctx)
                close_to_oracle(img, want, TOL, f"{what} kernel {KNAME[k]}")
                same_frame(img, frame(fresh), f"{what} kernel {KNAME[k]}: refit vs fresh upload")
            settle(ctx)
            assert ctx.debug_anim_rebuilds() > rebuilds, f"{what}: a class changed and nothing was rebuilt"
            ctx.set_kernel(rtamd.KERNEL_ACCEL)  # and through the accelerator rebuilt from these records
            fresh.set_kernel(rtamd.KERNEL_ACCEL)
            same_frame(frame(ctx), frame(fresh), f"{what}: after the rebuild vs fresh upload")
    finally:
        ctx.set_kernel(rtamd.KERNEL_AUTO)
        fresh.set_kernel(rtamd.KERNEL_AUTO)
