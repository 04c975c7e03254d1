"""The refit's device state against a plain recomputation (-m gpu).

After every rt_update_shapes / rt_update_nodes / rt_animate flush the accelerator's device
arrays are read back (rt_debug_accel_dump) from the context itself, its Moller-Trumbore
sub-context and its brute-force one, and tests/refit_ref.py recomputes what each must hold from
the host's records alone: records and node-box copies bit for bit, slot boxes as the exact
float32 union of the conservative boxes below, grow-only content boxes, cone words as the
reference cone's word and never culling a direction a normal below faces, Moller-Trumbore
constants bounding their triangles within 1e-4. A frame only sees a box or cone that is too
small if a ray grazes it, and never one that is too large; these tests see both.

Scenes: the soup of test_gpu_updates.py (1,500 triangles, 30 spheres, a wall, a plane), built
with buildBVH(6) (more than 8 reference leaves: one titems record per scene-tree item) and
with buildBVH(2) (at most 8: the few-leaf titems layout, one record per leaf); the tests assert
which layout each got. The builder lists every shape in exactly one leaf (asserted), so no moved
set needs a shape listed twice. rt_debug_async_rebuild(0) throughout: a rebuild runs in the
flush that finds its report. The growth-box path of group frame slots (AF_BOX) needs a group:
tests/test_gpu_group_refit_state.py checks it with the same reference.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bench
import refit_ref as rr
import rtamd
from test_gpu_updates import _soup

pytestmark = pytest.mark.gpu
W, H = 64, 48
MODES = [1, 2, -1]
_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = {"soup6": lambda: _soup(1, 1500, 6), "soup2": lambda: _soup(1, 1500, 2),
                         "soup4k": lambda: _soup(3, 4400, 3)}[name]()
    return _SCENES[name]


def _moved(shapes, ids, rng, k):
    """test_gpu_updates.py's _moved: spheres and walls shifted, triangles shifted and turned
    about Y by 0.2 (k + 1) rad. Here the stored plane turns with the vertices (normal rotated,
    D through the new first vertex), so that the back-face cones above them change too."""
    s = shapes.copy()
    for i in ids:
        t = s["type"][i]
        d = (rng.normal(size=3) * 0.8).astype(np.float32)
        if t == 0:
            s["sphereCenter"][i] += d
        elif t == 2:
            s["wallStart"][i] += d
        elif t == 3:
            c = (s["triP1"][i].astype(np.float64) + s["triP2"][i] + s["triP3"][i]) / 3
            a = 0.2 * (k + 1)

            def turn(q):
                return np.array([q[0] * np.cos(a) - q[2] * np.sin(a), q[1], q[0] * np.sin(a) + q[2] * np.cos(a)])
            for f in ("triP1", "triP2", "triP3"):
                s[f][i] = (turn(s[f][i].astype(np.float64) - c) + c + d).astype(np.float32)
            s["planeNormal"][i] = turn(s["planeNormal"][i].astype(np.float64)).astype(np.float32)
            s["planeD"][i] = np.float32(-(s["planeNormal"][i].astype(np.float64) @ s["triP1"][i].astype(np.float64)))
    return s


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """A second context: every scene uploaded whole."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


def _async(c, on):
    fn = c._lib.rt_debug_async_rebuild
    fn.argtypes = [C.c_void_p, C.c_int]
    assert fn(c._h, int(on)) == 0


class Run:
    """One context under test with its host copy of the scene and the previous dumps."""

    def __init__(self, ctx, fresh, fs, mode, whiches=("own", "mtc", "brute")):
        self.ctx, self.fresh, self.whiches = ctx, fresh, whiches
        self.host = rtamd.FlatScene(fs.shapes.copy(), fs.nodes.copy(), fs.indices, fs.camera, fs.light)
        ctx.upload(fs)
        ctx.set_kernel(rtamd.KERNEL_AUTO)
        ctx.debug_refit(mode)
        _async(ctx, 0)
        with pytest.raises(rtamd.RTError) as e:  # no sub-context before a frame with its toggle
            ctx.debug_accel_dump("mtc")
        assert e.value.code == -1
        for bvh, mt in ((True, True), (False, False)):  # a frame each creates the sub-contexts
            if ("mtc" if mt else "brute") in whiches:
                ctx.set_params(W, H, 3, bvh, False, mt)
                ctx.render(W, H)
        ctx.set_params(W, H, 3, True)
        self.prev = {}
        self.brute_nodes = ctx.debug_accel_dump("brute")["staging_nodes"] if "brute" in whiches else None
        self.verify("as uploaded")

    def verify(self, what, built=False):
        """Every rule, on every context, after the flush the dump itself applies. built: that
        flush rebuilt the accelerator and no refit has run on it yet, so there is no previous
        dump and the cones are the build's (the rules of a fresh build, on every slot)."""
        h = self.host
        self.fresh.upload(h)
        fd = self.fresh.debug_accel_dump("own")
        out = {}
        for w in self.whiches:
            d = self.ctx.debug_accel_dump(w)
            f, nodes, idx = fd, h.nodes, h.indices
            if w == "brute":  # one leaf listing the shapes in order
                f = dict(fd, geo_leaf=fd["geo_lin"], nodes=d["nodes"])
                nodes, idx = self.brute_nodes, np.arange(len(h.shapes), dtype=np.int32)
            v = rr.check(d, h.shapes, nodes, idx, prev=None if built else self.prev.get(w), fresh=f, all_slots=built)
            assert v == [], f"{what} [{w}]: {len(v)} violations, first {v[:4]}"
            out[w] = d
        self.prev = out
        return out


def _set(fs, n, rng, under=None):
    """n shapes to move: triangles with up to three spheres and the wall (from 4 on); `under`:
    a prim range's shapes the triangles are taken from."""
    t = fs.shapes["type"]
    tri = np.where(t == 3)[0] if under is None else under[t[under] == 3]
    extra = np.concatenate([np.where(t == 0)[0][:3], np.where(t == 2)[0]]) if n >= 4 else np.zeros(0, np.int64)
    extra = np.setdiff1d(extra, tri)
    ids = np.concatenate([rng.choice(tri, n - len(extra), replace=False), extra])
    return np.sort(ids).astype(np.int32)


def _top_slot_shapes(d, least):
    """the shapes below the smallest slot whose prim range holds at least `least` triangles"""
    s = d["slots"]
    ok = np.where((s[:, 0] == 1) & ((s[:, 3] & 2) == 0) & (s[:, 2] - s[:, 1] >= least))[0]
    q = ok[np.argmin(s[ok, 2] - s[ok, 1])]
    return np.unique(d["prim_shape"][s[q, 1]:s[q, 2]])


def _longest_refit_list(d):
    """the most refit prims below one slot that is refit (a slot's list in k_refit)"""
    s = d["slots"]
    n_ref = np.concatenate([[0], np.cumsum(d["refit_of"][d["prim_shape"]] >= 0)])
    ok = (s[:, 0] == 1) & ((s[:, 3] & 2) == 0)
    return int((n_ref[s[ok, 2]] - n_ref[s[ok, 1]]).max())


@pytest.fixture
def run_factory(ctx, fresh):
    yield lambda fs, mode, **kw: Run(ctx, fresh, fs, mode, **kw)
    ctx.debug_refit(-1)
    _async(ctx, 1)
    ctx.set_animated(np.zeros(0, np.int32))


def test_layouts(ctx, fresh, run_factory):
    """Which titems layout each soup got, read from the dump; no shape is listed in two leaves."""
    for name in ("soup6", "soup2", "soup4k"):
        fs = scene(name)
        assert len(np.unique(fs.indices)) == len(fs.indices) == len(fs.shapes), name
    d6 = run_factory(scene("soup6"), -1, whiches=("own",)).prev["own"]
    assert d6["nfew"] == 0 and d6["n_titems"] > 8
    d2 = run_factory(scene("soup2"), -1, whiches=("own",)).prev["own"]
    assert 0 < d2["nfew"] == d2["n_titems"] <= 8


def test_upload_copies_the_packed_arrays():
    """A fresh upload of soup6 and of soup2 holds the host packer's arrays (accel_pack.h
    pack_accel, through refit_ref.host_dump) byte for byte, in a context and in its Moller-
    Trumbore one: anodes, wnodes, titems, lnodes with their code words, the titems' leaves, and
    the info words. (A context of its own: the others keep no Moller-Trumbore sub-context.)"""
    c = rtamd.ComputeShader(0)
    try:
        for name in ("soup6", "soup2"):
            fs = scene(name)
            c.upload(fs)
            c.set_params(W, H, 3, True, False, True)
            c.render(W, H)  # creates the Moller-Trumbore sub-context
            for w, mt in (("own", 0), ("mtc", 1)):
                d, h = c.debug_accel_dump(w), rr.host_dump(fs, mt)
                assert d["built"] == 1 and d["mt"] == mt
                for sec in ("anodes", "wnodes", "titems", "lnodes", "titem_ref", "info"):
                    assert d[sec].shape == h[sec].shape and d[sec].tobytes() == h[sec].tobytes(), (name, w, sec)
    finally:
        c.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 1100])
@pytest.mark.parametrize("name", ["soup6", "soup2"])
def test_update_shapes_and_nodes(run_factory, name, n, mode):
    """rt_update_shapes (single records and a partly unmoved range) + rt_update_nodes, three
    steps. Set sizes at the refit's loop edges: 1; 63, 64, 65 around the record role's 64-lane
    workgroups and a wave's stride over a node's list (the root lists every entry); 300
    triangles under one slot (a refit list above kBigList = 256: the workgroup path, asserted
    from the dump); 1,100 (above range4's 1,024 elements at 256 threads and, with its slots'
    lists, above kDirectReads)."""
    fs = scene(name)
    rng = np.random.default_rng(100 + n)
    r = run_factory(fs, mode)
    ids = _set(fs, n, rng, _top_slot_shapes(r.prev["own"], 340) if n == 300 else None)
    tri0 = int(ids[fs.shapes["type"][ids] == 3][0])
    for k in range(3):
        h = r.host
        h.shapes = _moved(h.shapes, ids, rng, k)
        for j in ids:
            r.ctx.update_shapes(int(j), h.shapes[j:j + 1])
        lo = min(tri0, len(h.shapes) - 3)
        r.ctx.update_shapes(lo, h.shapes[lo:lo + 3])  # a range, partly unmoved
        rtamd.update_bvh(h, ids)
        r.ctx.update_nodes(h.nodes)
        r.verify(f"{name} n {n} mode {mode} step {k}")
    st = r.ctx.debug_refit_stats()
    assert st["entries"] >= n and st["dirty_slots"] > 0
    assert _longest_refit_list(r.prev["own"]) > (256 if n >= 300 else 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 1100])
@pytest.mark.parametrize("name", ["soup6", "soup2"])
def test_animate(run_factory, name, n, mode):
    """rt_set_animated + rt_animate, three steps: the device grows the nodes listing a moved
    shape (updateBVH); every node-box copy equals the host's updateBVH of the same records."""
    fs = scene(name)
    rng = np.random.default_rng(200 + n)
    r = run_factory(fs, mode)
    ids = _set(fs, n, rng, _top_slot_shapes(r.prev["own"], 340) if n == 300 else None)
    r.ctx.set_animated(ids)
    for k in range(3):
        h = r.host
        h.shapes = _moved(h.shapes, ids, rng, k)
        r.ctx.animate(h.shapes[ids])
        rtamd.update_bvh(h, ids)
        r.verify(f"{name} n {n} mode {mode} frame {k}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["soup6", "soup2"])
def test_update_nodes_alone(run_factory, name, mode):
    """rt_update_nodes alone, grown and still nested, with and without a refit set: every
    node-box copy follows; no slot box (but the kNoPrune ones, which open), cone, Moller-
    Trumbore constant or content box changes."""
    fs = scene(name)
    rng = np.random.default_rng(5)
    r = run_factory(fs, mode, whiches=("own", "mtc"))
    ids = _set(fs, 65, rng)
    for k in range(2):
        before = r.prev
        h = r.host
        h.nodes["boundsMin"] -= np.float32(0.75)
        h.nodes["boundsMax"] += np.float32(0.75)
        r.ctx.update_nodes(h.nodes)
        after = r.verify(f"{name} mode {mode} nodes grown {k}")
        for w in after:
            a, b = after[w], before[w]
            keep = (a["slots"][:, 0] == 1) & ((a["slots"][:, 3] & 2) == 0)
            assert np.array_equal(rr.slot_boxes(a)[keep].view(np.uint32), rr.slot_boxes(b)[keep].view(np.uint32)), w
            assert np.array_equal(a["anodes"].reshape(-1, 4, 4)[:, 2:].view(np.uint32),
                                  b["anodes"].reshape(-1, 4, 4)[:, 2:].view(np.uint32)), w
            if a["mt"]:
                # Without a refit set (k = 0) no slot role runs: the whole record stays. With one,
                # the grazing cone's axis is the sum of the normals flipped towards the axis of
                # the refit before, so axis, s and slab may differ from flush to flush (the
                # reference follows them from the previous dump); the padding constants stay.
                sel = slice(0, 10) if k == 0 else slice(4, 8)
                assert np.array_equal(rr.mt_consts(a)[:, sel].view(np.uint32), rr.mt_consts(b)[:, sel].view(np.uint32)), w
            else:
                assert np.array_equal(rr.cone_words(a), rr.cone_words(b)), w
        if k == 0:  # a refit set for the second round
            h.shapes = _moved(h.shapes, ids, rng, 0)
            for j in ids:
                r.ctx.update_shapes(int(j), h.shapes[j:j + 1])
            r.verify(f"{name} mode {mode} set moved")


def _move(r, ids, rng, k, what):
    h = r.host
    h.shapes = _moved(h.shapes, ids, rng, k)
    for j in ids:
        r.ctx.update_shapes(int(j), h.shapes[j:j + 1])
    return r.verify(what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["soup6", "soup2"])
def test_set_change(run_factory, name, mode):
    """Set A moves, then a disjoint set B alone, then their union: A's entries stay in the
    refit set while B alone moves (no compaction below 4,096 stale entries), and every slot
    above them still holds the exact union of the current boxes after every flush."""
    fs = scene(name)
    rng = np.random.default_rng(9)
    r = run_factory(fs, mode)
    A = _set(fs, 65, rng)
    B = np.setdiff1d(_set(fs, 130, rng), A)[:64].astype(np.int32)
    c0 = r.ctx.debug_refit_stats()["compactions"]
    _move(r, A, rng, 0, f"{name} mode {mode} A")
    _move(r, B, rng, 1, f"{name} mode {mode} B alone")
    assert r.ctx.debug_refit_stats()["entries"] == len(A) + len(B)
    for k in range(2):
        _move(r, np.union1d(A, B), rng, 2 + k, f"{name} mode {mode} union {k}")
    assert r.ctx.debug_refit_stats()["compactions"] == c0


@pytest.mark.parametrize("mode", MODES)
def test_compaction(run_factory, mode):
    """The refit set is compacted once its stale entries outnumber 4,096 (so this soup has 4,400
    triangles): 4,150 triangles move, then a disjoint 30 alone, whose flush drops the 4,150
    (rt_debug_refit_stats). The slots above those, static now, are rebuilt from the shape_moved /
    shape_box cache into dstatic and must hold the exact union of the current boxes; then part
    of the first set joins again."""
    fs = scene("soup4k")
    rng = np.random.default_rng(9)
    r = run_factory(fs, mode, whiches=("own", "mtc"))
    tri = rng.permutation(np.where(fs.shapes["type"] == 3)[0])
    A, B = np.sort(tri[:4150]).astype(np.int32), np.sort(tri[4150:4180]).astype(np.int32)
    c0 = r.ctx.debug_refit_stats()["compactions"]
    _move(r, A, rng, 0, f"mode {mode} A")
    assert r.ctx.debug_refit_stats()["compactions"] == c0
    _move(r, B, rng, 1, f"mode {mode} B alone")
    st = r.ctx.debug_refit_stats()
    assert st["compactions"] == c0 + 1 and st["entries"] == len(B), st
    _move(r, np.union1d(A[:40], B), rng, 2, f"mode {mode} union")


def _sliver(shapes, t):
    """triangle t collapsed in place: its third vertex on the middle of its first edge"""
    shapes["triP3"][t] = shapes["triP1"][t] + (shapes["triP2"][t] - shapes["triP1"][t]) * 0.5


def _slots_above(d, t):
    """the pruning slots whose prim range holds shape t"""
    return [q for q in np.where((d["slots"][:, 0] == 1) & ((d["slots"][:, 3] & 2) == 0))[0]
            if t in d["prim_shape"][d["slots"][q, 1]:d["slots"][q, 2]]]


@pytest.mark.parametrize("mode", MODES)
def test_kind_change(run_factory, mode):
    """A moved triangle collapses to a sliver: after that flush every slot above it is infinite
    on all axes and everything else obeys the rules; the next flush rebuilds
    (debug_anim_rebuilds one higher) and the new topology passes with finite boxes. Grown back,
    the shape was unbounded at that build and contributes nothing until the next rebuild."""
    fs = scene("soup6")
    rng = np.random.default_rng(12)
    r = run_factory(fs, mode)
    ids = _set(fs, 65, rng)
    h = r.host
    h.shapes = _moved(h.shapes, ids, rng, 0)
    for j in ids:
        r.ctx.update_shapes(int(j), h.shapes[j:j + 1])
    r.verify("moved")
    t = int(ids[fs.shapes["type"][ids] == 3][0])
    good = h.shapes[t:t + 1].copy()
    _sliver(h.shapes, t)
    r0 = r.ctx.debug_anim_rebuilds()
    r.ctx.update_shapes(t, h.shapes[t:t + 1])
    out = r.verify("sliver")
    assert r.ctx.debug_anim_rebuilds() == r0
    d = out["own"]
    above = _slots_above(d, t)
    assert above, "the sliver's triangle is under no slot"
    sb = rr.slot_boxes(d)[above]
    assert np.all(sb[:, :3] == -np.inf) and np.all(sb[:, 3:] == np.inf)
    out = r.verify("rebuilt", built=True)  # this flush reads the report and rebuilds
    assert r.ctx.debug_anim_rebuilds() == r0 + 1
    d = out["own"]
    has = (d["slots"][:, 0] == 1) & ((d["slots"][:, 3] & 2) == 0)
    assert np.isfinite(rr.slot_boxes(d)[has]).all() and d["shape_cls"][t] != rr.BOUNDED
    h.shapes[t] = good[0]  # bounded again: nothing above it until the rebuild
    r.ctx.update_shapes(t, h.shapes[t:t + 1])
    r.verify("grown back")
    r.verify("rebuilt again", built=True)
    assert r.ctx.debug_anim_rebuilds() == r0 + 2
    assert r.prev["own"]["shape_cls"][t] == rr.BOUNDED


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", [3, 2])
def test_published_animations(run_factory, cfg, mode):
    """Config 3's turning wheels and config 2's bouncing spheres (bench.py's frames), four
    frames through rt_animate at their real topology, the context and its Moller-Trumbore one."""
    fs = rtamd.generate(cfg, 0, 320, 180)
    ids, frames = bench.wheel_frames(fs, 4) if cfg == 3 else bench.sphere_frames(fs, 4)
    r = run_factory(fs, mode, whiches=("own", "mtc"))
    r.ctx.set_animated(ids)
    r0 = r.ctx.debug_anim_rebuilds()
    for k in range(4):
        r.host.shapes[ids] = frames[k]
        r.ctx.animate(frames[k])
        rtamd.update_bvh(r.host, ids)
        r.verify(f"config {cfg} mode {mode} frame {k}")
    assert r.ctx.debug_anim_rebuilds() == r0
