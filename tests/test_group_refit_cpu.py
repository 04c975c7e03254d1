"""The inputs of tests/test_gpu_group_refit_state.py shown able to fail, without a GPU.

A group's frame slot renders every F-th frame and must still hold the node growth of the frames it
skipped (rtx::animate_deferred). A test of that can fail only if a skipped frame changes a node
box, which the 0.8-unit moves of test_gpu_refit_state._moved mostly do not. So every frame here
is _moved(base, ids, rng, k) shifted by 64 units (the soups' root box spans about +-30) along
+x, -y, +z, -x, +y, -z in turn (refit_ref.shifted): each of six frames sets an extreme of the boxes
listing a moved shape that no other frame sets. From the seventh frame on the step doubles, so the
two further frames an F = 4 burst pair needs set new extremes again. This module asserts, for every
(scene, set) the GPU module uses, that dropping any single frame but the last changes a node box
and changes no shape's class, and that refit_ref.check reports exactly the nodes that lack a
dropped frame's growth.
"""
import numpy as np
import pytest

import refit_ref as rr
import rtamd
from test_gpu_refit_state import _moved, _set, _top_slot_shapes, scene

SCENES = ["soup6", "soup2"]
SIZES = [1, 64, 65, 300]
N_FRAMES = 8  # six, and two more at twice the step for the second burst at F = 4
_CASES = {}
_HOST_DUMPS = {}


def host_dump(name, mt=0):
    if (name, mt) not in _HOST_DUMPS:
        _HOST_DUMPS[name, mt] = rr.host_dump(scene(name), mt)
    return _HOST_DUMPS[name, mt]


def frames_of(shapes, ids, rng, n_frames=N_FRAMES):
    """n_frames frames of the shapes `ids` (their records, in the order of `ids`), each built
    from the base records `shapes`: _moved's noise and turn, then refit_ref.shifted's 64 units."""
    return [rr.shifted(_moved(shapes, ids, rng, k), ids, k)[ids].copy() for k in range(n_frames)]


def case(name, n):
    """(scene, ids, frames) of the set of n shapes; 300: triangles under one slot, as
    test_gpu_refit_state._top_slot_shapes picks them from the host-packed dump."""
    if (name, n) not in _CASES:
        fs = scene(name)
        rng = np.random.default_rng(300 + n)
        ids = _set(fs, n, rng, _top_slot_shapes(host_dump(name), 340) if n == 300 else None)
        _CASES[name, n] = (fs, ids, frames_of(fs.shapes, ids, rng))
    return _CASES[name, n]


def case_ab(name):
    """The entry-order case: (scene with set A moved and its nodes grown by A, A, B descending,
    B's frames). A enters the refit set first, in ascending order, so B's entries are neither at
    B's positions in the animated set nor in its order."""
    if (name, "ab") not in _CASES:
        fs = scene(name)
        rng = np.random.default_rng(17)
        A = _set(fs, 65, rng)
        B = np.setdiff1d(_set(fs, 130, rng), A)[:64][::-1].astype(np.int32).copy()
        h = rtamd.FlatScene(_moved(fs.shapes, A, rng, 0), fs.nodes.copy(), fs.indices, fs.camera, fs.light)
        rtamd.update_bvh(h, A)
        _CASES[name, "ab"] = (h, A, B, frames_of(h.shapes, B, rng))
    return _CASES[name, "ab"]


def _without(frames, i):
    return frames[:i] + frames[i + 1:]


@pytest.mark.parametrize("n", SIZES + ["ab"])
@pytest.mark.parametrize("name", SCENES)
def test_a_dropped_frame_changes_a_node_box(name, n):
    """Of the six frames, and of the eight of two F = 4 bursts (whose first burst is verified
    before the second hides its first two extremes), leaving out any frame but the last of the
    frames not yet verified changes at least one node box: a slot that forgot a frame it did not
    render cannot hold the expected nodes."""
    if n == "ab":
        fs, _, ids, frames = case_ab(name)
    else:
        fs, ids, frames = case(name, n)
    for total, first in ((6, 0), (4, 0), (N_FRAMES, 4)):
        full = rr.grown_nodes(fs, ids, frames[:total])
        for i in range(first, total - 1):
            changed = rr.boxes_differ(full, rr.grown_nodes(fs, ids, _without(frames[:total], i)))
            assert len(changed) >= 1, f"{name} n {n}: frame {i} of {total} leaves no trace in any node box"
            assert len(fs.nodes) - 1 in changed, f"{name} n {n}: frame {i} of {total} leaves no trace in the root"
    # the order of the frames is free (min and max are exact), only their set counts
    again = rr.grown_nodes(fs, ids, frames[:6][::-1])
    assert len(rr.boxes_differ(rr.grown_nodes(fs, ids, frames[:6]), again)) == 0


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_no_frame_changes_a_class(name, mt):
    """No frame moves a shape out of the class its boxes were built for (rta::classify with
    the accelerator's own origin_lim), so no GPU case but the kind change may rebuild."""
    d = host_dump(name, mt)
    fs = scene(name)
    base, _ = rr.classify(fs.shapes, d["origin_lim"], mt)
    sets = [case(name, n)[1:] for n in SIZES]
    h, _, B, fb = case_ab(name)
    for ids, frames in sets + [(B, fb)]:
        for k, f in enumerate(frames):
            cls, _ = rr.classify(f, d["origin_lim"], mt)
            assert np.array_equal(cls, base[ids]), f"{name} mt {mt}: frame {k} changes a class"


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("n", [1, 64])
@pytest.mark.parametrize("name", SCENES)
def test_check_reports_the_nodes_that_lack_a_frame(name, n, mt):
    """A host-packed dump whose node copies hold grown_nodes without one frame, checked against
    grown_nodes of all frames: reported at exactly the nodes whose box that frame changes, in
    every copy (the staging record, the packed node, anodes), and not at all with every frame."""
    fs, ids, frames = case(name, n)
    frames = frames[:6]
    shapes = fs.shapes.copy()
    shapes[ids] = frames[-1]
    full = rr.grown_nodes(fs, ids, frames)

    def dump(nodes):
        return rr.host_dump(rtamd.FlatScene(shapes, nodes, fs.indices, fs.camera, fs.light), mt)
    v = rr.check(dump(full), shapes, full, fs.indices, all_slots=True)
    assert v == [], v[:4]
    for i in (0, 2, 4):
        less = rr.grown_nodes(fs, ids, _without(frames, i))
        want = sorted(rr.boxes_differ(full, less).tolist())
        v = rr.check(dump(less), shapes, full, fs.indices, all_slots=True)
        for array in ("staging_nodes", "nodes", "anodes"):
            assert sorted(x[1] for x in v if x[0] == array) == want, (array, i, v[:4])
        assert all(x[0] in ("staging_nodes", "nodes", "anodes", "wnodes", "titems") for x in v), v[:4]
