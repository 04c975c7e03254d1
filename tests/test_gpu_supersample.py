"""Supersampled frames (rt_set_samples; -m gpu, needs an MI355X).

The definition under test: a frame with n x n samples per pixel is the box filter, in
the fixed float32 order of tests/ss_ref.py, of the one-sample frame of n*W x n*H pixels
rendered with resX*n, resY*n. The scene always comes from rtamd.generate(cfg, 0, n*W,
n*H) and the reference is always ss_ref.box(frame(n*W, n*H, resX = n*W, resY = n*H)),
where the frame is the oracle's (tolerance 1e-4 per channel, the parity tests' own: the
filter averages values that each lie within it) or the renderer's (bit for bit).

Every destination starts NaN-poisoned, so a pixel left unwritten fails the comparison.
References are computed once per (scene, size, settings, kernel), shared read-only.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
import rtamd
import ss_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
KERNELS = [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET, rtamd.KERNEL_LANE]
KNAME = {rtamd.KERNEL_ACCEL: "accel", rtamd.KERNEL_PACKET: "packet", rtamd.KERNEL_LANE: "lane"}
RT_ERR_INVALID = -1
# (maxBounces, useBVH, useFresnel, useMollerTrumbore)
PLAIN3 = (3, True, False, False)
CFG_SET = {2: (1, True, False, False), 3: PLAIN3}


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
    ctx.debug_ss_general(0)
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.set_latency_mode(0)
    ctx.debug_heavy(-1, 4)
    ctx.set_tail(-1)
    ctx.debug_tail_lanes(64)
    ctx.set_schedule(rtamd.SCHED_COST)
    ctx.set_walk(-1)


@functools.lru_cache(maxsize=None)
def scene(cfg, sw, sh):
    return rtamd.generate(cfg, 0, sw, sh)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_box(cfg, sw, sh, n, s):
    """box(the oracle's one-sample frame of sw x sh, resX = sw, resY = sh)."""
    ref, _ = oracle.render(scene(cfg, sw, sh), sw, sh, oracle.params(sw, sh, *s))
    return frozen(ss_ref.box(ref, n))


def surface(rows, width, channels=4, fill=float("nan")):
    out = torch.full((rows, width, channels), fill, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # the renderer's stream does not wait on torch's
    return out


def load(ctx, fs, resX, resY, s, kernel):
    ctx.upload(fs)
    ctx.set_params(resX, resY, *s)
    ctx.set_kernel(kernel)


def full_frame(ctx, W, H, n):
    """The whole W x H frame with n x n samples through rt_dispatch_rows."""
    ctx.set_samples(n)
    out = surface(H, W)
    ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
    ctx.sync()
    return out.cpu().numpy()


_gpu_box = {}


def gpu_box(ctx, cfg, W, H, n, s, kernel):
    """box(the renderer's own one-sample frame of n*W x n*H with `kernel`), rendered with
    the context's default switches (call it before a test changes any)."""
    key = (cfg, W, H, n, s, kernel)
    if key not in _gpu_box:
        sw, sh = n * W, n * H
        load(ctx, scene(cfg, sw, sh), sw, sh, s, kernel)
        one = full_frame(ctx, sw, sh, 1)
        assert np.isfinite(one).all()
        _gpu_box[key] = frozen(ss_ref.box(one, n))
    return _gpu_box[key]


def same(img, ref, what):
    assert img.shape == ref.shape, what
    assert np.array_equal(img, ref), f"{what}: {int((img != ref).any(axis=-1).sum())} pixels differ"


# --------------------------------------------------------------------------
# 1. against the oracle: sample frames that are parity cases of test_gpu_parity.py
ORACLE_CASES = [
    # cfg, W, H, n, settings
    (1, 80, 60, 2, (3, True, False, False)),
    (1, 40, 30, 4, (3, True, False, False)),
    (1, 20, 15, 8, (3, True, False, False)),
    (1, 80, 60, 2, (3, False, False, False)),
    (2, 100, 75, 2, (1, True, False, False)),
    (2, 100, 75, 2, (4, True, True, False)),
    (2, 60, 45, 2, (2, False, True, True)),
]


@pytest.mark.parametrize("kernel", KERNELS, ids=KNAME.get)
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "c%d_%dx%d_n%d_b%d_bvh%d_f%d_mt%d" % (
    c[0], c[1], c[2], c[3], c[4][0], c[4][1], c[4][2], c[4][3]))
def test_against_the_oracle(ctx, case, kernel):
    cfg, W, H, n, s = case
    ref = oracle_box(cfg, n * W, n * H, n, s)
    load(ctx, scene(cfg, n * W, n * H), W, H, s, kernel)
    img = full_frame(ctx, W, H, n)
    assert np.isfinite(img).all(), "a pixel was left out"
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    print(f"cfg{cfg} {W}x{H} n={n} {KNAME[kernel]}: max |gpu - box(oracle)| = {diff.max():.3g}")
    bad = int((diff > TOL).any(axis=-1).sum())
    assert bad == 0, f"{bad} pixels over {TOL}, max diff {diff.max():.3g}"


# --------------------------------------------------------------------------
# 2. bit identity with the renderer's own one-sample frame
@pytest.mark.parametrize("kernel", KERNELS, ids=KNAME.get)
@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("cfg", [3, 2])
def test_equals_the_filtered_one_sample_frame(ctx, cfg, n, kernel):
    """51 x 37: at n = 2 and 4 the sample frame (102 x 74, 204 x 148) ends in partial
    8x8 tiles in both directions."""
    W, H, s = 51, 37, CFG_SET[cfg]
    ref = gpu_box(ctx, cfg, W, H, n, s, kernel)
    load(ctx, scene(cfg, n * W, n * H), W, H, s, kernel)
    img = full_frame(ctx, W, H, n)
    same(img, ref, f"cfg{cfg} n={n} {KNAME[kernel]}")
    if kernel == rtamd.KERNEL_ACCEL:
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
        ctx.debug_ss_general(1)
        gen = full_frame(ctx, W, H, n)
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
        same(gen, img, f"cfg{cfg} n={n}: forced general path against fused")


def test_far_camera_takes_the_general_path(ctx):
    """No usable accelerator (a camera far outside the scene): the packet kernel renders
    the sample frame and the filter kernel writes the output."""
    W, H, n, s = 32, 24, 2, (2, True, False, False)
    fs = scene(2, n * W, n * H)
    cam = fs.camera.copy()
    cam["Position"] = cam["Position"] - cam["Front"] * np.float32(60000.0)
    far = rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, cam, fs.light)
    load(ctx, far, n * W, n * H, s, rtamd.KERNEL_AUTO)
    ref = ss_ref.box(full_frame(ctx, n * W, n * H, 1), n)
    ctx.set_params(W, H, *s)
    img = full_frame(ctx, W, H, n)
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_PACKET
    same(img, ref, "far camera")


# --------------------------------------------------------------------------
# 3. bit identity under the other switches, all against one filtered frame per n
SW, SH = 96, 54


def _heavy(parts):
    def run(ctx, render):
        # the cost order exists from the second frame on; latency mode splits on the frames
        # that record no cost, the default mode on those that do (the parts' summed costs)
        ctx.set_latency_mode(1)
        ctx.debug_heavy(10 ** 6, parts)
        frames = [render() for _ in range(3)]
        ctx.set_latency_mode(0)
        ctx.debug_heavy(7, parts)
        return frames + [render() for _ in range(2)]
    return run


def _tail(ctx, render):
    ctx.set_tail(1)
    ctx.debug_tail_lanes(64)
    return [render(), render()]


def _schedule(mode):
    def run(ctx, render):
        ctx.set_schedule(mode)
        return [render() for _ in range(3)]
    return run


def _walk(depth):
    def run(ctx, render):
        ctx.set_walk(depth)
        return [render()]
    return run


SWITCHES = {"heavy2": _heavy(2), "heavy4": _heavy(4), "heavy8": _heavy(8), "tail": _tail,
            "sched_rows": _schedule(rtamd.SCHED_ROWS), "sched_cost": _schedule(rtamd.SCHED_COST),
            "sched_cost_xcd": _schedule(rtamd.SCHED_COST_XCD), "walk0": _walk(0), "walk99": _walk(99)}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@pytest.mark.parametrize("n", [2, 4])
def test_switches_do_not_change_the_frame(ctx, n, switch):
    ref = gpu_box(ctx, 3, SW, SH, n, PLAIN3, rtamd.KERNEL_ACCEL)
    load(ctx, scene(3, n * SW, n * SH), SW, SH, PLAIN3, rtamd.KERNEL_ACCEL)
    for k, img in enumerate(SWITCHES[switch](ctx, lambda: full_frame(ctx, SW, SH, n))):
        same(img, ref, f"{switch} n={n} frame {k}")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL


@pytest.mark.parametrize("s", [(3, True, False, True), (3, False, False, False)], ids=["moller_trumbore", "brute"])
@pytest.mark.parametrize("n", [2, 4])
def test_uniforms_that_change_the_frame(ctx, n, s):
    """useMollerTrumbore and useBVH = 0 are uniforms of the frame, not switches: they move
    hit points and the shadow offset, so the filtered frame they are compared with is the
    one-sample frame under the same uniforms. Both render through k_accel instances of
    their own (the MT accelerator, the brute branch's one-leaf tree)."""
    ref = gpu_box(ctx, 3, SW, SH, n, s, rtamd.KERNEL_ACCEL)
    load(ctx, scene(3, n * SW, n * SH), SW, SH, s, rtamd.KERNEL_ACCEL)
    for k in range(2):
        same(full_frame(ctx, SW, SH, n), ref, f"settings {s} n={n} frame {k}")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL


@pytest.mark.parametrize("measure", [0, 1], ids=["counters", "wall_time"])
@pytest.mark.parametrize("case", ["plain", "latency", "moller_trumbore"])
def test_cost_frames_and_ordered_frames(ctx, case, measure):
    """The supersampling k_accel instances by what the dispatch records: a cost frame (by
    either measure, rt_debug_cost_time) and then a frame in the order it left, which records
    nothing, in the default mode, in latency mode and over the Moller-Trumbore accelerator.
    76 x 44 at 2 x 2: 19 x 11 sample tiles with a partial column."""
    W, H, n = 76, 44, 2
    s = (3, True, False, True) if case == "moller_trumbore" else PLAIN3
    ref = gpu_box(ctx, 3, W, H, n, s, rtamd.KERNEL_ACCEL)
    load(ctx, scene(3, n * W, n * H), W, H, s, rtamd.KERNEL_ACCEL)
    try:
        ctx.debug_cost_time(measure)
        ctx.set_latency_mode(case == "latency")
        ctx.debug_sched_period(1)  # every dispatch a cost frame
        same(full_frame(ctx, W, H, n), ref, f"{case} measure {measure}: cost frame")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
        ctx.debug_sched_period(16)
        same(full_frame(ctx, W, H, n), ref, f"{case} measure {measure}: ordered frame")
        assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
    finally:
        ctx.debug_sched_period(16)
        ctx.debug_cost_time(-1)


# --------------------------------------------------------------------------
# 4. row forms and formats
@pytest.mark.parametrize("kernel", [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET], ids=KNAME.get)
@pytest.mark.parametrize("out_rows", [12, 20])
@pytest.mark.parametrize("n", [2, 4])
def test_stripes_and_formats(ctx, n, out_rows, kernel):
    """y0 = 8, stripe = 8, period = 24: compact row r is image row 8 + (r / 8) * 24 + r % 8,
    i.e. rows 8..15, 32..39 and 56..59; 12 rows end inside the second stripe, and of 20
    the last four lie below the 54-row frame and stay untouched."""
    ref = gpu_box(ctx, 3, SW, SH, n, PLAIN3, kernel)
    load(ctx, scene(3, n * SW, n * SH), SW, SH, PLAIN3, kernel)
    ctx.set_samples(n)
    ys = [8 + (r // 8) * 24 + r % 8 for r in range(out_rows)]
    for fmt, ch in [(rtamd.FORMAT_RGBA32F, 4), (rtamd.FORMAT_RGB32F, 3)]:
        out = surface(out_rows, SW, ch, -7.0)
        ctx.dispatch_rows_ex(SW, SH, 8, 8, 24, out_rows, out.data_ptr(), SW * 4 * ch, fmt=fmt)
        ctx.sync()
        got = out.cpu().numpy()
        for r, y in enumerate(ys):
            if y < SH:
                assert np.array_equal(got[r], ref[y, :, :ch]), f"fmt {fmt} row {r} (image row {y})"
            else:
                assert (got[r] == -7.0).all(), f"fmt {fmt} row {r} lies below the frame"
    # RT_FORMAT_RGBA32F_IMAGE: the rows land at their image rows of a whole pre-filled surface
    out = surface(SH, SW, 4, -7.0)
    ctx.dispatch_rows_ex(SW, SH, 8, 8, 24, out_rows, out.data_ptr(), SW * 16, fmt=rtamd.FORMAT_RGBA32F_IMAGE)
    ctx.sync()
    got = out.cpu().numpy()
    mine = sorted(y for y in ys if y < SH)
    assert np.array_equal(got[mine], ref[mine])
    others = [y for y in range(SH) if y not in mine]
    assert (got[others] == -7.0).all()


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_ACCEL, rtamd.KERNEL_PACKET], ids=KNAME.get)
def test_pitched_destination(ctx, kernel):
    n, pitch_px = 2, SW + 5
    ref = gpu_box(ctx, 3, SW, SH, n, PLAIN3, kernel)
    load(ctx, scene(3, n * SW, n * SH), SW, SH, PLAIN3, kernel)
    ctx.set_samples(n)
    out = surface(SH, pitch_px, 4, 9.0)
    ctx.dispatch_rows(SW, SH, 0, 1, 1, SH, out.data_ptr(), pitch_px * 16)
    ctx.sync()
    got = out.cpu().numpy()
    same(got[:, :SW], ref, "pitched")
    assert (got[:, SW:] == 9.0).all()


def test_own_surface(ctx):
    """rt_dispatch + rt_read_image: the context's surface is the W x H output."""
    n = 4
    ref = gpu_box(ctx, 3, SW, SH, n, PLAIN3, rtamd.KERNEL_ACCEL)
    load(ctx, scene(3, n * SW, n * SH), SW, SH, PLAIN3, rtamd.KERNEL_ACCEL)
    ctx.set_samples(n)
    same(ctx.render(SW, SH), ref, "own surface")


# --------------------------------------------------------------------------
# 5. state
def test_samples_one_restores_todays_frame(ctx):
    W, H = 96, 54
    fs = scene(3, W, H)
    fresh = rtamd.ComputeShader(0)
    try:
        load(fresh, fs, W, H, PLAIN3, rtamd.KERNEL_AUTO)
        want = full_frame(fresh, W, H, 1)
    finally:
        fresh.close()
    load(ctx, fs, W, H, PLAIN3, rtamd.KERNEL_AUTO)
    full_frame(ctx, W, H, 4)
    same(full_frame(ctx, W, H, 1), want, "set_samples(1) after set_samples(4)")


@pytest.mark.parametrize("n", [0, 3, 16, -1])
def test_other_sample_counts_are_refused(ctx, n):
    with pytest.raises(rtamd.RTError) as e:
        ctx.set_samples(n)
    assert e.value.code == RT_ERR_INVALID


def test_sample_frame_over_the_grid_limit_is_refused(ctx):
    """300,000 rows are 37,500 rows of tiles, a valid one-sample dispatch; with n = 2
    they are 75,000, over the grid's 65,535. The destination is allocated in full all the
    same. The refusal launches nothing and the next dispatch renders as ever."""
    W, H, n = 8, 300000, 2
    load(ctx, scene(3, n * SW, n * SH), SW, SH, PLAIN3, rtamd.KERNEL_ACCEL)
    ctx.set_samples(n)
    out = surface(H, W, 4, -7.0)
    with pytest.raises(rtamd.RTError) as e:
        ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
    assert e.value.code == RT_ERR_INVALID
    ctx.sync()
    assert bool((out == -7.0).all())
    with pytest.raises(rtamd.RTError) as e:  # a scaled value that overflows int
        ctx.dispatch_rows_ex(W, 2 ** 30, 0, 1, 1, 8, out.data_ptr(), W * 16)
    assert e.value.code == RT_ERR_INVALID
    with pytest.raises(rtamd.RTError) as e:  # negative rows stay an error
        ctx.dispatch_rows(W, 64, 0, 1, 1, -1, out.data_ptr(), W * 16)
    assert e.value.code == RT_ERR_INVALID
    del out
    ref = gpu_box(ctx, 3, SW, SH, n, PLAIN3, rtamd.KERNEL_ACCEL)
    load(ctx, scene(3, n * SW, n * SH), SW, SH, PLAIN3, rtamd.KERNEL_ACCEL)
    same(full_frame(ctx, SW, SH, n), ref, "the dispatch after a refusal")


@pytest.mark.parametrize("kernel", [rtamd.KERNEL_ACCEL, rtamd.KERNEL_LANE], ids=KNAME.get)
@pytest.mark.parametrize("n", [2, 8])
def test_alpha_is_exactly_one(ctx, n, kernel):
    W, H = 40, 24
    load(ctx, scene(2, n * W, n * H), W, H, CFG_SET[2], kernel)
    img = full_frame(ctx, W, H, n)
    assert (img[..., 3] == 1.0).all()
    assert np.isfinite(img).all()


# --------------------------------------------------------------------------
# 6. animated scene: the refit and the supersampled dispatch share the stream
def test_animated_scene(ctx):
    W, H, n = 96, 54, 2
    fs = scene(3, n * W, n * H)
    ids = np.arange(3380, 3380 + 640, dtype=np.int32)  # the car's wheel triangles (bench.wheel_frames)
    rec = fs.shapes[ids].copy()
    for f in ("triP1", "triP2", "triP3"):
        rec[f] = rec[f] + np.float32([0.25, 0.5, -0.125])
    load(ctx, rtamd.FlatScene(fs.shapes.copy(), fs.nodes.copy(), fs.indices, fs.camera, fs.light), W, H, PLAIN3,
         rtamd.KERNEL_ACCEL)
    still = full_frame(ctx, W, H, n)
    ctx.set_animated(ids)
    ctx.animate(rec)
    moved = full_frame(ctx, W, H, n)  # the refit runs ahead of this dispatch, on its stream
    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
    ctx.set_params(n * W, n * H, *PLAIN3)
    ref = ss_ref.box(full_frame(ctx, n * W, n * H, 1), n)
    same(moved, ref, "animated step")
    assert not np.array_equal(moved, still), "the step moved nothing visible"
