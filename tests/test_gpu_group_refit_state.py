"""The deferred growth of a group's frame slots against a plain recomputation (-m gpu).

rt_group_animate does not refit: it writes the records on the host of every member x frame-slot
context and unions the frame's growToInclude boxes into a per-shape growth box
(rtx::animate_deferred). Each slot context refits once, at the next frame it renders, with the
union of up to F frames' boxes (k_refit's AF_BOX, read by the record role in refit mode 1 and by
the node role itself in mode 2), and the host keeps its own copy of the grown root for the sky-row
band. A frame cannot see a slot that forgot the growth of the frames it did not render; the state
can. So after every step the slot contexts are dumped (rt_debug_accel_dump) and tests/refit_ref.py
recomputes what they must hold:

* records: the latest frame's, bit for bit, against a whole upload;
* every copy of every node box: rtamd.update_bvh applied once per frame given to the group since
  the upload, in order (refit_ref.grown_nodes), the frames this slot never rendered included;
* slot boxes and pbox: the exact float32 unions of the current records' conservative boxes (no
  growth box leaks into them);
* content boxes, the refit cone's word, the Moller-Trumbore axis: against the slot's previous
  dump, where exactly one refit of the slot ran between the two (protocol A).

Frames: tests/test_group_refit_cpu.py builds them and shows that each leaves a trace in a node
box that no other frame leaves. One process, Group([0, 0], GATHER_COPY, frames=F), 64 x 48, stripe
8, rt_debug_async_rebuild(0). Member 0's slots are verified on the context, its Moller-Trumbore
and its brute-force sub-context, member 1's on the context alone.

Protocol A (waited): animate, dispatch, sync, then the slot that rendered is verified against its
previous dump; its refit count rose by exactly one and no other slot's moved. Protocol B (in
flight): F x (animate, dispatch), one sync, then every slot is verified without a previous dump
(the dump's own flush applies what is pending for the slots that rendered earlier), twice.
"""
import numpy as np
import pytest
import torch

import refit_ref as rr
import rtamd
from test_gpu_refit_state import _async, _longest_refit_list, _sliver, _slots_above, scene
from test_group_refit_cpu import case, case_ab, frames_of

pytestmark = pytest.mark.gpu
W, H, STRIPE = 64, 48, 8
SUBS = ("own", "mtc", "brute")


@pytest.fixture(scope="module")
def fresh():
    """A plain context: every expected scene uploaded whole."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = rtamd.ComputeShader(0)
    yield c
    c.close()


class GRun:
    """A group of two members x F frame slots with the host's copy of the scene, the previous
    dump of every (member, slot, context) and the refit and rebuild counts."""

    def __init__(self, fresh, fs, F, mode, subs=SUBS, camera=None):
        self.fresh, self.fs, self.F, self.subs = fresh, fs, F, subs
        self.cam = fs.camera if camera is None else camera
        self.g = g = rtamd.Group([0] * 2, rtamd.GATHER_COPY, frames=F)
        try:
            g.set_timeout(60000)
            g.upload(rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, self.cam, fs.light))
            for c in g.contexts:
                c.debug_refit(mode)
                _async(c, 0)
            self.dispatched = 0
            # a slot's sub-contexts exist once the slot has rendered a frame with their toggle
            for bvh, mt in ((True, True), (False, False)):
                if ("mtc" if mt else "brute") in subs:
                    g.set_params(W, H, 3, bvh, False, mt)
                    for _ in range(F):
                        self.dispatch()
                    g.sync()
            g.set_params(W, H, 3, True)
            self.brute_nodes = self.ctx(0, 0).debug_accel_dump("brute")["staging_nodes"] if "brute" in subs else None
            self.rebuilds0 = self.rebuilds()
            self.prev = {}
            self.verify(self.all(), fs.shapes, fs.nodes, "as uploaded", use_prev=False)
        except BaseException:
            g.close()
            raise

    def close(self):
        self.g.close()

    def ctx(self, member, slot):
        return self.g.contexts[member * self.F + slot]

    def all(self):
        return [(m, j) for m in range(2) for j in range(self.F)]

    def slot(self, j):
        return [(0, j), (1, j)]

    def dispatch(self):
        """one frame; returns the slot that renders it"""
        j = self.dispatched % self.F
        self.g.dispatch(W, H, STRIPE)
        self.dispatched += 1
        return j

    def refits(self):
        return [c.debug_refits() for c in self.g.contexts]

    def rebuilds(self):
        return [c.debug_anim_rebuilds() for c in self.g.contexts]

    def verify(self, where, shapes, nodes, what, use_prev, built=False, not_yet=None):
        """Every rule on the (member, slot) contexts `where`, which must hold the records
        `shapes` and the node boxes `nodes`, after the flush the dump itself applies. not_yet:
        shapes that joined the refit set after the last refit ran (rt_set_animated alone): the
        slots above them alone still hold the build's cones, as those above no entry do."""
        fs = self.fs
        self.fresh.upload(rtamd.FlatScene(shapes, nodes, fs.indices, self.cam, fs.light))
        fd = self.fresh.debug_accel_dump("own")
        out = {}
        for m, j in where:
            for w in (self.subs if m == 0 else ("own",)):
                d = self.ctx(m, j).debug_accel_dump(w)
                if not_yet is not None:
                    d["refit_of"][not_yet] = -1
                f, nd, idx = fd, nodes, fs.indices
                if w == "brute":  # one leaf listing the shapes in order
                    f = dict(fd, geo_leaf=fd["geo_lin"], nodes=d["nodes"])
                    nd, idx = self.brute_nodes, np.arange(len(shapes), dtype=np.int32)
                prev = self.prev.get((m, j, w)) if use_prev and not built else None
                assert prev is not None or not use_prev or built, (m, j, w)
                v = rr.check(d, shapes, nd, idx, prev=prev, fresh=f, all_slots=built)
                assert v == [], f"{what} [member {m} slot {j} {w}]: {len(v)} violations, first {v[:4]}"
                self.prev[m, j, w] = out[m, j, w] = d
        return out


@pytest.fixture
def grun(fresh):
    made = []

    def make(fs, F, mode, **kw):
        made.append(GRun(fresh, fs, F, mode, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


def _with(shapes, ids, recs):
    s = shapes.copy()
    s[ids] = recs
    return s


def _protocol_a(r, base, ids, frames, what, other=None):
    """Six waited frames. base: the scene the growth starts from. other: a second group of one
    frame slot, given the expected scene whole before every frame, whose sky-row band this group's
    must equal (the host's copy of the grown root against a root uploaded as it is); returns the
    bands."""
    g, F = r.g, r.F
    g.set_animated(ids)
    bands = []
    for k in range(6):
        shapes = _with(base.shapes, ids, frames[k])
        nodes = rr.grown_nodes(base, ids, frames[:k + 1])
        before = r.refits()
        g.animate(frames[k])
        assert r.refits() == before, f"{what} frame {k}: rt_group_animate refit a slot"
        j = r.dispatch()
        if other is not None:
            other.upload(rtamd.FlatScene(shapes, nodes, base.indices, r.cam, base.light))
            other.dispatch(W, H, STRIPE)
            bands.append((g.sky_band(), other.sky_band()))
            other.sync()
        g.sync()
        want = [n + (i % F == j) for i, n in enumerate(before)]
        assert r.refits() == want, f"{what} frame {k}: slot {j} alone refits, once for the {F} frames since its last"
        d = r.verify(r.slot(j), shapes, nodes, f"{what} frame {k}", use_prev=True)
        assert r.refits() == want, f"{what} frame {k}: the dump's own flush found growth pending"
    assert r.rebuilds() == r.rebuilds0, f"{what}: an accelerator was rebuilt"
    return d, bands


def _protocol_b(r, base, ids, frames, what):
    """Two bursts of F frames in flight, every slot verified after each."""
    g, F = r.g, r.F
    g.set_animated(ids)
    k = 0
    for burst in range(2):
        for _ in range(F):
            g.animate(frames[k])
            r.dispatch()
            k += 1
        g.sync()
        d = r.verify(r.all(), _with(base.shapes, ids, frames[k - 1]), rr.grown_nodes(base, ids, frames[:k]),
                     f"{what} burst {burst}", use_prev=False)
    assert r.rebuilds() == r.rebuilds0, f"{what}: an accelerator was rebuilt"
    return d


def _cases():
    """(scene, n, F, mode): both soups x n x F x the two modes with an AF_BOX reader each, and
    the auto policy on soup6 at F = 3."""
    out = [(name, n, F, mode) for name in ("soup6", "soup2") for n in (1, 64, 65, 300) for F in (2, 3, 4)
           for mode in (1, 2)]
    return out + [("soup6", n, 3, -1) for n in (1, 64, 65, 300)]


@pytest.mark.parametrize("name,n,F,mode", _cases())
def test_waited_frames(grun, name, n, F, mode):
    """Protocol A. 300: triangles under one slot, a refit list above kBigList = 256 (asserted)."""
    fs, ids, frames = case(name, n)
    d, _ = _protocol_a(grun(fs, F, mode), fs, ids, frames, f"{name} n {n} F {F} mode {mode}")
    assert d[0, 5 % F, "own"]["n_refit"] == n
    assert _longest_refit_list(d[0, 5 % F, "own"]) > (256 if n == 300 else 0)


@pytest.mark.parametrize("name,n,F,mode", [c for c in _cases() if c[2] >= 3])
def test_frames_in_flight(grun, name, n, F, mode):
    """Protocol B."""
    fs, ids, frames = case(name, n)
    d = _protocol_b(grun(fs, F, mode), fs, ids, frames, f"{name} n {n} F {F} mode {mode}")
    assert _longest_refit_list(d[0, 0, "own"]) > (256 if n == 300 else 0)


@pytest.mark.parametrize("mode", [1, 2, -1])
@pytest.mark.parametrize("name", ["soup6", "soup2"])
def test_entry_order_differs_from_set_order(grun, name, mode):
    """Set A moves through rt_group_update_shapes / rt_group_update_nodes and is flushed, so it
    holds the first refit entries; then the disjoint set B is animated, its ids descending. B's
    entry is nowhere its position in the animated set (asserted from the dump), so a growth box
    stored at the set position instead of the entry reaches the wrong shape's nodes."""
    h, A, B, frames = case_ab(name)
    fs = scene(name)
    r = grun(fs, 3, mode)
    for j in A:
        r.g.update_shapes(int(j), h.shapes[j:j + 1])
    r.g.update_nodes(h.nodes)
    r.verify(r.all(), h.shapes, h.nodes, f"{name} mode {mode} A moved", use_prev=False)
    d, _ = _protocol_a(r, h, B, frames, f"{name} mode {mode} B animated")
    entry = d[0, 5 % 3, "own"]["refit_of"][B]
    assert (entry >= 0).all() and not (entry == np.arange(len(B))).any(), entry
    assert (np.diff(entry) > 0).all() and (np.diff(B) < 0).all()


def _base_of(fs, shapes, nodes):
    return rtamd.FlatScene(shapes, nodes, fs.indices, fs.camera, fs.light)


@pytest.mark.parametrize("mode", [1, 2])
def test_update_nodes_after_deferred_frames(grun, mode):
    """(a) rt_group_update_nodes after two deferred frames and no dispatch: the growth applies
    first (one refit per slot, at the call), then the host's records replace every copy. The
    next two frames, deferred together, grow the host's records and nothing else."""
    fs, ids, frames = case("soup6", 64)
    r = grun(fs, 3, mode)
    g = r.g
    g.set_animated(ids)
    g.animate(frames[0])
    g.animate(frames[1])
    before = r.refits()
    X = fs.nodes.copy()
    X["boundsMin"] -= np.float32(0.75)
    X["boundsMax"] += np.float32(0.75)
    g.update_nodes(X)
    assert r.refits() == [n + 1 for n in before], "the pending growth is flushed before the host's node records"
    shapes = _with(fs.shapes, ids, frames[1])
    r.verify(r.all(), shapes, X, "host nodes after two deferred frames", use_prev=False)
    g.animate(frames[2])
    g.animate(frames[3])
    j = r.dispatch()
    g.sync()
    base = _base_of(fs, shapes, X)
    r.verify(r.slot(j), _with(fs.shapes, ids, frames[3]), rr.grown_nodes(base, ids, frames[2:4]),
             "two frames after the host's nodes", use_prev=False)
    assert r.rebuilds() == r.rebuilds0


@pytest.mark.parametrize("mode", [1, 2])
def test_set_animated_with_growth_pending(grun, mode):
    """(b) rt_group_set_animated of another set with two frames pending: the old set's frames
    are not lost, and the new set's frame grows on top of them."""
    h, A, B, fb = case_ab("soup6")
    fs = scene("soup6")
    fa = frames_of(fs.shapes, A, np.random.default_rng(23), 2)
    r = grun(fs, 3, mode)
    g = r.g
    g.set_animated(A)
    g.animate(fa[0])
    g.animate(fa[1])
    before = r.refits()
    g.set_animated(B)
    assert r.refits() == [n + 1 for n in before], "the old set's pending frames are flushed with the old set"
    nodes = rr.grown_nodes(fs, A, fa)
    shapes = _with(fs.shapes, A, fa[1])
    r.verify(r.slot(1), shapes, nodes, "the old set's frames", use_prev=False, not_yet=B)
    rec = fb[0]  # built on B's base records: A and B are disjoint
    assert len(np.intersect1d(A, B)) == 0
    g.animate(rec)
    j = r.dispatch()
    g.sync()
    assert j == 0
    r.verify(r.all(), _with(shapes, B, rec), rr.grown_nodes(_base_of(fs, shapes, nodes), B, [rec]),
             "the new set's frame", use_prev=False)
    assert r.rebuilds() == r.rebuilds0


@pytest.mark.parametrize("mode", [1, 2])
def test_update_nodes_before_a_deferred_frame(grun, mode):
    """(c) rt_group_update_nodes, then rt_group_animate: the host's node records are flushed
    before the frame is deferred, so the frame grows them (the other order would leave them as
    the host wrote them); two more deferred frames grow them further."""
    fs, ids, frames = case("soup6", 64)
    r = grun(fs, 3, mode)
    g = r.g
    g.set_animated(ids)
    X = fs.nodes.copy()
    X["boundsMin"] -= np.float32(0.75)
    X["boundsMax"] += np.float32(0.75)
    before = r.refits()
    g.update_nodes(X)
    assert r.refits() == before
    g.animate(frames[0])
    assert r.refits() == [n + 1 for n in before], "the host's node records are flushed before the deferral"
    r.verify(r.all(), _with(fs.shapes, ids, frames[0]), rr.grown_nodes(_base_of(fs, fs.shapes, X), ids, frames[:1]),
             "a deferred frame after the host's nodes", use_prev=False)
    assert r.refits() == [n + 2 for n in before]
    g.animate(frames[1])
    g.animate(frames[2])
    r.verify(r.all(), _with(fs.shapes, ids, frames[2]), rr.grown_nodes(_base_of(fs, fs.shapes, X), ids, frames[:3]),
             "two more deferred frames", use_prev=False)
    assert r.refits() == [n + 3 for n in before]
    assert r.rebuilds() == r.rebuilds0


@pytest.mark.parametrize("mode", [1, 2])
def test_rt_animate_joins_pending_growth(grun, mode):
    """(d) rt_animate on one slot's own context with two deferred frames pending (sky rows off,
    or the group would refuse that member): the frame joins them and the slot flushes at once,
    to the state of the three frames in sequence. The other slots are untouched until their own
    flush, and a further group frame lands on both histories."""
    fs, ids, frames = case("soup6", 64)
    r = grun(fs, 3, mode)
    g = r.g
    g.set_sky_rows(False)
    g.set_animated(ids)
    g.animate(frames[0])
    g.animate(frames[1])
    before = r.refits()
    r.ctx(0, 1)._n_animated = len(ids)  # the group gave this context its animated set
    r.ctx(0, 1).animate(frames[2])
    assert r.refits() == [n + (i == 1) for i, n in enumerate(before)], "that slot flushes at once, no other does"
    r.verify([(0, 1)], _with(fs.shapes, ids, frames[2]), rr.grown_nodes(fs, ids, frames[:3]),
             "the slot given rt_animate", use_prev=False)
    assert r.refits() == [n + (i == 1) for i, n in enumerate(before)]
    others = [w for w in r.all() if w != (0, 1)]
    r.verify(others[:3], _with(fs.shapes, ids, frames[1]), rr.grown_nodes(fs, ids, frames[:2]),
             "the other slots", use_prev=False)
    g.animate(frames[3])
    j = r.dispatch()
    g.sync()
    assert j == 0
    r.verify([(0, 1)], _with(fs.shapes, ids, frames[3]), rr.grown_nodes(fs, ids, frames[:4]),
             "the slot given rt_animate, a group frame later", use_prev=False)
    r.verify(others, _with(fs.shapes, ids, frames[3]), rr.grown_nodes(fs, ids, frames[:2] + frames[3:4]),
             "the other slots, a group frame later", use_prev=False)
    assert r.rebuilds() == r.rebuilds0


@pytest.mark.parametrize("mode", [1, 2])
def test_kind_change_while_deferred(grun, mode):
    """test_gpu_refit_state.test_kind_change's collapsing triangle, given in a frame that slots
    0 and 1 do not render. At their next flush (the dump's) every slot box above the sliver is
    infinite and nothing is rebuilt; the flush after that rebuilds (debug_anim_rebuilds one
    higher) and the new accelerator passes as a fresh build, with the node boxes of all three
    frames. Slot 2 rendered the frame: its report is in by the second dump."""
    fs, ids, frames = case("soup6", 65)
    t_at = int(np.where(fs.shapes["type"][ids] == 3)[0][0])
    t = int(ids[t_at])
    frames = [f.copy() for f in frames[:3]]
    _sliver(frames[2], t_at)
    r = grun(fs, 3, mode)
    g = r.g
    g.set_animated(ids)
    for k in range(3):
        g.animate(frames[k])
        assert r.dispatch() == k
        g.sync()
    assert r.rebuilds() == r.rebuilds0
    shapes = _with(fs.shapes, ids, frames[2])
    nodes = rr.grown_nodes(fs, ids, frames)
    waiting = r.slot(0) + r.slot(1)
    out = r.verify(waiting, shapes, nodes, "sliver", use_prev=False)
    assert r.rebuilds() == r.rebuilds0
    for m, j in waiting:
        d = out[m, j, "own"]
        above = _slots_above(d, t)
        assert above, "the sliver's triangle is under no slot"
        sb = rr.slot_boxes(d)[above]
        assert np.all(sb[:, :3] == -np.inf) and np.all(sb[:, 3:] == np.inf), (m, j)
    out = r.verify(waiting, shapes, nodes, "rebuilt", use_prev=False, built=True)
    for m, j in r.slot(2):  # (its sub-contexts were not rendered with: their first flush is this dump's)
        for w in (r.subs if m == 0 else ("own",)):
            r.ctx(m, j).debug_accel_dump(w)
    r.verify(r.slot(2), shapes, nodes, "rebuilt, the slot that rendered the frame", use_prev=False, built=True)
    assert r.rebuilds() == [n + 1 for n in r.rebuilds0]
    d = out[0, 0, "own"]
    has = (d["slots"][:, 0] == 1) & ((d["slots"][:, 3] & 2) == 0)
    assert np.isfinite(rr.slot_boxes(d)[has]).all() and d["shape_cls"][t] != rr.BOUNDED


def _far_camera():
    """the soups' camera direction from twelve times as far: the root box, grown by 64 units a
    frame, stays well inside the 60 degrees of the 48 rows"""
    sc = rtamd.Scene().generate(3, 0, W / H)
    sc.set_camera((60, -300, 540), 60, W / H)
    sc.LookAt((0, 0, 0))
    return sc.serializeScene().camera


@pytest.mark.parametrize("mode", [1, 2])
def test_host_root_follows_the_device_root(grun, mode):
    """The host's copy of the grown root (the sky-row band and rtx::matches_view rest on it)
    against a root uploaded as it is: after every animate + dispatch of protocol A at F = 3 the
    group's band equals the band of a second two-member group with one frame slot, the same
    camera and parameters and a whole upload of the expected scene. The bands are proper
    sub-ranges of the rows, and they change as the root grows. A dispatch that is not refused
    shows that the slots' roots agree with the group's; the dumps' root node box equalling
    grown_nodes' is the device half."""
    fs, ids, frames = case("soup6", 64)
    cam = _far_camera()
    r = grun(fs, 3, mode, subs=("own",), camera=cam)
    other = rtamd.Group([0] * 2, rtamd.GATHER_COPY)
    try:
        other.set_timeout(60000)
        other.upload(rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, cam, fs.light))
        other.set_params(W, H, 3, True)
        _, bands = _protocol_a(r, fs, ids, frames, f"sky band mode {mode}", other=other)
    finally:
        other.close()
    assert all(a == b for a, b in bands), bands
    assert all(0 <= y0 < y1 <= H and y1 - y0 < H for (y0, y1), _ in bands), f"no proper band: {bands}"
    assert len({a for a, _ in bands}) > 1, f"the band never moved: {bands}"
