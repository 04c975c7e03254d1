"""The cost order (k_tile_order, k_cost_dilate, the cost recording at the end of k_accel)
against plain restatements, -m gpu.

Every permutation of the tiles renders the same image, so the frame tests cannot see a
wrong order. Here the recorded costs are read back (rt_debug_sched_cost) and compared
with the per-tile records (rt_debug_tile_times), and the order with the counting sort
the kernels' comments describe, restated in numpy: 32 half-octave buckets, heaviest
first; inside a bucket the groups of 256 tiles in order (the rank inside a group is
arbitrary); under SCHED_COST_XCD each bucket dealt to the 8 XCDs as contiguous chunks.
Every comparison is exact.
"""
import numpy as np
import pytest
import torch

import rtamd

GROUP, BUCKETS, XCDS = 256, 32, 8  # kOrderThreads, kOrderBuckets, kXcds

# W, H: 96 tiles (one group), exactly 256, 272, 13 x 10 with partial edge tiles, 920
# (four groups, the last partial)
FRAMES = [(96, 64), (128, 128), (136, 128), (100, 75), (320, 180)]
CASES = [(3, W, H) for W, H in FRAMES] + [(5, 320, 180)]
CASE_IDS = ["c%d_%dx%d" % c for c in CASES]


def bucket(c):
    """work_bucket: 0 for c < 2, else min(31, 2 * floor(log2 c) - 1 + the bit below the top bit)."""
    c = np.asarray(c, np.int64)
    l = np.frexp(np.maximum(c, 1).astype(np.float64))[1].astype(np.int64) - 1  # floor(log2 c), exact
    below = (c >> np.maximum(l - 1, 0)) & 1
    return np.where(c < 2, 0, np.minimum(BUCKETS - 1, 2 * l - 1 + below))


def test_bucket_rule_is_monotone():
    """The restated bucket rule over every cost up to 2^17: monotone, one step up at 2 and
    at every 2^l and 3 * 2^(l-1) (half octaves), nowhere else, and 31 from 2^16 on."""
    c = np.arange(0, (1 << 17) + 1)
    b = bucket(c)
    assert b[0] == b[1] == 0 and b[2] == 1 and b[3] == 2 and b[4] == 3 and b[6] == 4
    step = np.diff(b)
    assert ((step == 0) | (step == 1)).all()
    edges = sorted({2} | {1 << l for l in range(1, 17)} | {3 << (l - 1) for l in range(1, 16)})
    assert (c[1:][step == 1]).tolist() == edges
    assert b[(1 << 16) - 1] == 30 and (b[1 << 16:] == BUCKETS - 1).all()
    assert bucket(np.array([0xffffffff]))[0] == BUCKETS - 1


def undeal(order, cost):
    """SCHED_COST_XCD undone: bucket by bucket (heaviest first, sizes from the costs), slot
    base + 8k + c holds the k-th tile of chunk c, and chunks c < cnt % 8 hold one tile more."""
    counts = np.bincount(bucket(cost), minlength=BUCKETS)
    out, base = [], 0
    for b in range(BUCKETS - 1, -1, -1):
        cnt = int(counts[b])
        for c in range(XCDS):
            size = cnt // XCDS + (1 if c < cnt % XCDS else 0)
            out += [order[base + XCDS * k + c] for k in range(size)]
        base += cnt
    return np.array(out, order.dtype)


def check_order(order, cost, what, xcd=False):
    """order is the counting sort of cost: a permutation, buckets non-increasing, and inside
    a bucket the tiles' groups non-decreasing."""
    tiles = len(cost)
    assert len(order) == tiles, what
    assert np.array_equal(np.sort(order), np.arange(tiles)), f"{what}: not a permutation"
    if xcd:
        b = bucket(cost[order])
        for k in range(BUCKETS):  # every XCD (slot mod 8) gets an eighth of every bucket
            per = np.bincount(np.nonzero(b == k)[0] % XCDS, minlength=XCDS)
            assert ((per == per.sum() // XCDS) | (per == per.sum() // XCDS + 1)).all(), f"{what}: bucket {k}: {per}"
        order = undeal(order, cost)
        assert np.array_equal(np.sort(order), np.arange(tiles)), f"{what}: undealt order not a permutation"
    b = bucket(cost[order])
    up = np.nonzero(np.diff(b) > 0)[0]
    assert up.size == 0, (f"{what}: bucket rises at position {up[:1]}: tiles {order[up[:1]]}, {order[up[:1] + 1]} "
                          f"cost {cost[order[up[:1]]]}, {cost[order[up[:1] + 1]]}")
    back = np.nonzero((np.diff(b) == 0) & (np.diff(order // GROUP) < 0))[0]
    assert back.size == 0, f"{what}: group order broken at position {back[:1]}: tiles {order[back[:1]]}, " \
                           f"{order[back[:1] + 1]} of bucket {b[back[:1]]}"


def dilate(cost, tiles_x, r):
    """Each tile's largest cost within r tiles in x and y, clipped at the tile grid."""
    grid = cost.reshape(-1, tiles_x)
    ty, tx = grid.shape
    pad = np.zeros((ty + 2 * r, tx + 2 * r), cost.dtype)  # costs are unsigned: 0 never wins
    pad[r:r + ty, r:r + tx] = grid
    out = grid.copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.maximum(out, pad[dy:dy + ty, dx:dx + tx])
    return out.reshape(-1)


def test_restatements_on_known_inputs():
    """The numpy restatements themselves: check_order takes a counting sort and refuses an
    ascending one, a swapped pair of groups and a bucket edge moved; undeal inverts the
    dealing; dilate is a clipped max filter `tiles_x` wide."""
    rng = np.random.default_rng(3)
    cost = rng.integers(0, 5000, 700).astype(np.uint32)
    order = np.lexsort((np.arange(700), -bucket(cost)))  # by bucket descending, then by tile
    check_order(order, cost, "sorted")
    with pytest.raises(AssertionError):
        check_order(order[::-1].copy(), cost, "ascending")
    octave = np.where(cost < 2, 0, 2 * np.floor(np.log2(np.maximum(cost, 1))).astype(np.int64))
    with pytest.raises(AssertionError):  # whole octaves: the half-octave buckets come out mixed
        check_order(np.lexsort((np.arange(700), -octave)), cost, "octaves")
    b = bucket(cost[order])
    k = int(np.nonzero((np.diff(b) == 0) & (np.diff(order // GROUP) > 0))[0][0])
    swapped = order.copy()
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    with pytest.raises(AssertionError):
        check_order(swapped, cost, "groups swapped")
    dealt = np.empty_like(order)  # the dealing as the kernel's comment states it
    base = 0
    for cnt in np.bincount(b, minlength=BUCKETS)[::-1]:
        chunks = np.array_split(order[base:base + cnt], XCDS)  # the first cnt % 8 one longer
        for c, chunk in enumerate(chunks):
            dealt[base + c + XCDS * np.arange(len(chunk))] = chunk
        base += cnt
    assert np.array_equal(undeal(dealt, cost), order)
    check_order(dealt, cost, "dealt", xcd=True)
    g = np.arange(12, dtype=np.uint32).reshape(3, 4)
    assert dilate(g.reshape(-1), 4, 1).tolist() == [5, 6, 7, 7, 9, 10, 11, 11, 9, 10, 11, 11]
    assert dilate(g[::-1].reshape(-1), 4, 3).tolist() == [11] * 12
    one = np.zeros(12, np.uint32)
    one[4] = 9  # row 1, column 0: its neighbourhood must not wrap to the end of row 0
    assert dilate(one, 4, 1).reshape(3, 4).tolist() == [[9, 9, 0, 0], [9, 9, 0, 0], [9, 9, 0, 0]]


# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


_SCENES = {}


def start(ctx, cfg, W, H):
    """The scene uploaded, every dispatch a cost frame; returns (tiles, tiles_x)."""
    if (cfg, W, H) not in _SCENES:
        _SCENES[cfg, W, H] = rtamd.generate(cfg, 0, W, H)
    ctx.upload(_SCENES[cfg, W, H])
    ctx.set_params(W, H, 3, True)
    ctx.set_kernel(rtamd.KERNEL_ACCEL)
    ctx.debug_sched_period(1)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    return tx * ty, tx


def restore(ctx):
    ctx.debug_tile_times(0)
    ctx.debug_sched_period(16)
    ctx.debug_cost_time(-1)
    ctx.debug_cost_dilate(0)
    ctx.debug_heavy(-1, 4)
    ctx.set_latency_mode(0)
    ctx.set_schedule(rtamd.SCHED_COST)
    ctx.set_kernel(rtamd.KERNEL_AUTO)


def work(rec):
    """A tile record's node steps + tests over the wave's lanes (kTileRec fields 2, 3)."""
    return rec[:, 2] + rec[:, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", FRAMES, ids=lambda v: str(v))
def test_cost_is_the_tiles_work(ctx, W, H):
    """With the lane-work measure and no split tiles, the cost a dispatch records for a tile
    is the node steps + tests of its wave's lanes, as the per-tile records count them, for
    every tile, frame after frame.

    Two consecutive frames record identical costs once the dispatch policy is held still.
    rt_debug_heavy(0, 1) alone does not do that: the first max(64, tiles / 128) slots of the
    order also walk their camera rays' shadow rays per lane (rt_debug_lane_k, default -1),
    which counts fewer steps than the packet walk, so a tile's lane work depends on whether
    its slot is in that head. Measured on the car at these five sizes, eight frames each:
    3 to 26 tiles differ between consecutive frames under the default, every one of them a
    tile that entered or left the head; none with rt_debug_lane_k(0, 0). Both are asserted:
    under the default policy only tiles that changed sides may differ, and with the head
    off the costs repeat exactly."""
    try:
        tiles, _ = start(ctx, 3, W, H)
        ctx.debug_cost_time(0)
        ctx.debug_heavy(0, 1)
        ctx.debug_tile_times(tiles)

        def frame(what):
            ctx.render(W, H)
            cost, rec = ctx.debug_sched_cost(tiles), ctx.tile_times(tiles)
            assert len(cost) == tiles and len(rec) == tiles
            bad = np.nonzero(cost != work(rec))[0]
            assert bad.size == 0, f"{what}: {bad.size} tiles, first {bad[0]}: cost {cost[bad[0]]}, " \
                                  f"record {work(rec)[bad[0]]}"
            assert cost.max() > 0
            return cost

        lane_k = max(64, tiles // 128)
        prev = prev_head = None
        for f in range(4):
            head = set(ctx.debug_sched_order(tiles)[:lane_k].tolist())  # empty before the first order
            cost = frame(f"frame {f}")
            if prev is not None:
                moved = set(np.nonzero(cost != prev)[0].tolist())
                assert moved <= (head ^ prev_head), f"frame {f}: tiles {sorted(moved - (head ^ prev_head))} changed " \
                                                    f"cost without entering or leaving the per-lane head"
            prev, prev_head = cost, head
        ctx.debug_lane_k(0, 0)
        a, b = frame("no head, first"), frame("no head, second")
        assert np.array_equal(a, b), f"{int((a != b).sum())} tiles' costs differ between consecutive frames"
    finally:
        ctx.debug_lane_k(-1, 2)
        restore(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("k,parts", [(16, 8), (7, 2), (40, 16)])
def test_split_tiles_record_the_sum_of_their_parts(ctx, k, parts):
    """rt_debug_heavy: the k tiles at the head of the order run as `parts` waves; each
    records one cost, the sum of its parts' node steps + tests (records tiles + h * parts
    + p), and every other tile its own. Three frames running: a sum that is not reset, or
    one part's cost in place of the sum, shows."""
    W, H = 320, 180
    try:
        tiles, _ = start(ctx, 3, W, H)
        ctx.debug_cost_time(0)
        ctx.debug_heavy(k, parts)
        ctx.debug_tile_times(tiles + k * parts)
        ctx.render(W, H)  # the first order: no tile is split before one exists
        for frame in range(3):
            order = ctx.debug_sched_order(tiles)
            assert np.array_equal(np.sort(order), np.arange(tiles))
            ctx.render(W, H)
            cost, rec = ctx.debug_sched_cost(tiles), ctx.tile_times(tiles + k * parts)
            assert len(cost) == tiles and len(rec) == tiles + k * parts
            want = work(rec[:tiles])
            want[order[:k]] = work(rec[tiles:]).reshape(k, parts).sum(axis=1)
            assert (work(rec[tiles:]).reshape(k, parts).sum(axis=1) > 0).all(), "the head tiles do work"
            bad = np.nonzero(cost != want)[0]
            assert bad.size == 0, f"frame {frame}: {bad.size} tiles, first {bad[0]} (split: " \
                                  f"{bad[0] in order[:k]}): cost {cost[bad[0]]}, records {want[bad[0]]}"
            check_order(ctx.debug_sched_order(tiles), cost, f"heavy {k}x{parts} frame {frame}")
    finally:
        restore(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,W,H", CASES, ids=CASE_IDS)
def test_order_is_the_counting_sort_of_its_costs(ctx, cfg, W, H):
    """SCHED_COST with either cost measure, with and without latency mode (whose split tiles
    record sums): after every dispatch the order is the counting sort of the costs that
    dispatch recorded. The wall-time measure does not repeat from frame to frame; the order
    must still be the sort of its own dispatch's costs."""
    try:
        tiles, _ = start(ctx, cfg, W, H)
        ctx.set_schedule(rtamd.SCHED_COST)
        for measure in (0, 1):
            for latency in (0, 1):
                ctx.debug_cost_time(measure)
                ctx.set_latency_mode(latency)
                # (the first latency-mode dispatch after a change of camera ranks dilated costs)
                ctx.render(W, H)
                for frame in range(2):
                    ctx.render(W, H)
                    cost, order = ctx.debug_sched_cost(tiles), ctx.debug_sched_order(tiles)
                    assert len(cost) == tiles and cost.max() > 0
                    check_order(order, cost, f"measure {measure} latency {latency} frame {frame}")
    finally:
        restore(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,W,H", CASES, ids=CASE_IDS)
def test_xcd_order_is_the_counting_sort_dealt_in_chunks(ctx, cfg, W, H):
    """SCHED_COST_XCD: with the dealing undone the order is the same counting sort, and every
    XCD's slots hold an eighth of every bucket."""
    try:
        tiles, _ = start(ctx, cfg, W, H)
        ctx.set_schedule(rtamd.SCHED_COST_XCD)
        for measure in (0, 1):
            ctx.debug_cost_time(measure)
            for frame in range(2):
                ctx.render(W, H)
                cost, order = ctx.debug_sched_cost(tiles), ctx.debug_sched_order(tiles)
                assert len(cost) == tiles and cost.max() > 0
                check_order(order, cost, f"xcd measure {measure} frame {frame}", xcd=True)
    finally:
        restore(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("W,H", [(100, 75), (320, 180)], ids=lambda v: str(v))
def test_dilated_order_sorts_the_max_filter_of_the_costs(ctx, W, H, r):
    """rt_debug_cost_dilate: the order is the counting sort of each tile's largest raw cost
    within r tiles in x and y (a (2r+1)^2 window clipped at the frame's tile grid), and the
    costs read back stay the raw ones."""
    try:
        tiles, tx = start(ctx, 3, W, H)
        ctx.debug_cost_time(0)
        ctx.debug_heavy(0, 1)
        ctx.debug_tile_times(tiles)
        ctx.debug_cost_dilate(r)
        for frame in range(2):
            ctx.render(W, H)
            cost, order = ctx.debug_sched_cost(tiles), ctx.debug_sched_order(tiles)
            assert np.array_equal(cost, work(ctx.tile_times(tiles))), "the costs read back are the raw ones"
            wide = dilate(cost, tx, r)
            assert (bucket(wide) != bucket(cost)).any(), "the dilation must change some tile's bucket"
            check_order(order, wide, f"dilate {r} frame {frame}")
    finally:
        restore(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", [rtamd.SCHED_COST, rtamd.SCHED_COST_XCD])
def test_order_follows_a_change_of_tile_count(ctx, sched):
    """920 tiles, then 272, then 920 again on one context: every order is the counting sort
    of its own frame's costs (bucket rows left over from the other frame size would
    misplace tiles or leave slots unwritten)."""
    try:
        ctx.set_schedule(sched)
        ctx.debug_cost_time(0)
        for step, (W, H) in enumerate([(320, 180), (136, 128), (320, 180), (96, 64), (320, 180)]):
            tiles, _ = start(ctx, 3, W, H)
            for frame in range(2):
                ctx.render(W, H)
                cost, order = ctx.debug_sched_cost(tiles), ctx.debug_sched_order(tiles)
                assert len(cost) == tiles and len(order) == tiles and cost.max() > 0
                check_order(order, cost, f"step {step} {W}x{H} frame {frame}", xcd=sched == rtamd.SCHED_COST_XCD)
    finally:
        restore(ctx)
