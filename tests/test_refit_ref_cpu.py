"""The refit reference (tests/refit_ref.py) shown right without a GPU.

A "dump" of a freshly built accelerator is packed on the host (tests/native/refit_ref.cpp
rr_build: rta::build_accel, then the renderer's layouts). The reference must accept every
fresh build, barycentric and Moller-Trumbore, with no violation, and must report each single
corruption of the dump at the slot, node or item it was applied to.
"""
import copy

import numpy as np
import pytest

import refit_ref as rr
import rtamd
from test_gpu_updates import _soup  # the soup of the update tests (a scene generator: no GPU)

SCENES = ["soup6", "soup2", "config2", "config3"]


def _scene(name):
    if name == "soup6":
        return _soup(1, 1500, 6)
    if name == "soup2":
        return _soup(1, 1500, 2)
    return rtamd.generate(int(name[-1]), 0, 320, 180)


@pytest.fixture(scope="module")
def dumps():
    out = {}
    for name in SCENES:
        fs = _scene(name)
        for mt in (0, 1):
            out[name, mt] = (fs, rr.host_dump(fs, mt))
    return out


def _check(fs, d, **kw):
    return rr.check(d, fs.shapes, fs.nodes, fs.indices, all_slots=True, **kw)


def _where(v, array):
    return [x[1] for x in v if x[0] == array]


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_fresh_build_has_no_violation(dumps, name, mt):
    """Every rule that needs no previous dump, on every slot of a fresh build: the slot boxes are
    the exact float32 unions of classify's boxes, the node-box copies agree, the cones never
    cull a direction a normal below faces, the Moller-Trumbore constants bound their triangles."""
    fs, d = dumps[name, mt]
    assert d["built"] == 1 and d["P"] > 0 and (d["slots"][:, 0] == 1).sum() > 0
    v = _check(fs, d)
    assert v == [], v[:5]
    # the previous-dump rules on an unchanged dump
    v = _check(fs, d, prev=d)
    assert v == [], v[:5]


def _slots_with(d, pred):
    s = d["slots"]
    return [int(q) for q in np.where((s[:, 0] == 1) & ((s[:, 3] & 2) == 0))[0] if pred(q, int(s[q, 1]), int(s[q, 2]))]


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", ["soup6", "config3"])
@pytest.mark.parametrize("up", [False, True])
def test_slot_box_off_by_one_ulp_is_reported(dumps, name, mt, up):
    """hi.x of one slot lowered (too small: a ray could miss a prim) or raised (stale, too
    large) by one ulp: reported at that slot, and nowhere else."""
    fs, d0 = dumps[name, mt]
    for q in _slots_with(d0, lambda q, f, e: True)[3::97][:3]:
        d = copy.deepcopy(d0)
        x = rr.slot_boxes(d)[q, 3]
        rr.set_slot_box(d, q, 3, np.nextafter(x, np.float32(np.inf if up else -np.inf)))
        v = _check(fs, d)
        assert _where(v, "lnodes") == [q] and len(v) == 1, (q, v[:3])


def test_narrowed_cone_is_reported(dumps):
    """A cone's half angle narrowed by 0.2 degrees (less than the word's quantization slack
    hides from any sampled direction, more than kConeMargin): the threshold byte no longer is
    the byte of the reference cone. Slots of at most two prims, where the build's merged cone
    is the reference's cone; those whose byte the 0.2 degrees do not move are skipped."""
    fs, d0 = dumps["soup6", 0]
    shapes = rtamd.as_records(fs.shapes, rtamd.SHAPE_DTYPE)
    words = rr.cone_words(d0)
    done = 0
    for q in _slots_with(d0, lambda q, f, e: e - f <= 2 and words[q] != rr.CONE_NEVER):
        f, e = d0["slots"][q, 1:3]
        af, t = rr.ref_cone(shapes, d0["prim_shape"][f:e])
        aq = rr.cone_decode([words[q]])[0]
        t8 = rr.threshold_byte(t - np.radians(0.2))
        if t8 == aq[3]:
            continue
        d = copy.deepcopy(d0)
        rr.set_cone_word(d, q, int(words[q]) & 0x00FFFFFF | (t8 & 0xFF) << 24)
        v = _check(fs, d)
        assert _where(v, "lnodes") == [q] and "narrower" in v[0][3], (q, v[:3])
        done += 1
        if done == 5:
            break
    assert done == 5


def test_mt_constants_are_reported(dumps):
    """k[4] (the smallest |e1 x e2|) raised by 1e-3 relative, and the slab's half width k[9]
    halved: each reported at its slot. So is a cull given up or loosened: k[9] infinite or
    times 50 over triangles alone, and, where a build's cone is the tight one (up to two
    triangles), k[3] set to 2 or raised by a tenth."""
    fs, d0 = dumps["soup6", 1]
    K = rr.mt_consts(d0)
    qs = _slots_with(d0, lambda q, f, e: K[q, 4] > 0 and np.isfinite(K[q, 9]) and K[q, 9] > 1e-3)
    assert len(qs) >= 5
    for q in qs[::max(1, len(qs) // 5)][:5]:
        for k, val in ((4, K[q, 4] * np.float32(1.001)), (9, K[q, 9] * np.float32(0.5))):
            d = copy.deepcopy(d0)
            rr.set_mt_const(d, q, k, val)
            v = _check(fs, d)
            assert _where(v, "lnodes") == [q], (q, k, v[:3])
        for val in (np.float32(np.inf), K[q, 9] * np.float32(50)):
            d = copy.deepcopy(d0)
            rr.set_mt_const(d, q, 9, val)
            assert _where(_check(fs, d), "lnodes") == [q], (q, val)
    two = _slots_with(d0, lambda q, f, e: e - f <= 2 and 0 < K[q, 3] < 1.2 and np.isfinite(K[q, 9]))
    assert len(two) >= 5
    for q in two[::max(1, len(two) // 5)][:5]:
        for val in (np.float32(2.0), K[q, 3] + np.float32(0.1)):
            d = copy.deepcopy(d0)
            rr.set_mt_const(d, q, 3, val)
            assert _where(_check(fs, d, prev=d0), "lnodes") == [q], (q, val)
    # and a pad far too loose is reported too (tightness)
    d = copy.deepcopy(d0)
    rr.set_mt_const(d, qs[0], 6, K[qs[0], 6] * np.float32(1.01) + np.float32(1e-3))
    assert _where(_check(fs, d), "lnodes") == [qs[0]]


@pytest.mark.parametrize("name", ["soup6", "soup2"])
def test_node_box_copies_are_reported(dumps, name):
    """A titems box taken from the wrong leaf, a content box shrunk, a stale wnodes copy."""
    fs, d0 = dumps[name, 0]
    nodes = rtamd.as_records(fs.nodes, rtamd.NODE_DTYPE)
    N = len(nodes)
    ref = d0["titem_ref"]
    assert len(ref) >= 2, "no scene tree items"
    # titems: item 0 gets the box of another item's leaf
    other = int(np.where(ref != ref[0])[0][0])
    d = copy.deepcopy(d0)
    d["titems"][0:2, :3] = d0["titems"][2 * other:2 * other + 2, :3]
    v = _check(fs, d)
    assert _where(v, "titems") == [0] and len(v) == 1, v[:3]
    # a content box shrunk: against the previous dump at that node (and its parent's copy)
    an = d0["anodes"].reshape(N, 4, 4)
    k = int(np.where(np.isfinite(an[:, 3, 0]) & (nodes["leftChild"] == -1))[0][0])
    d = copy.deepcopy(d0)
    d["anodes"].reshape(N, 4, 4)[k, 3, 0] = np.nextafter(an[k, 3, 0], np.float32(-np.inf))
    v = _check(fs, d, prev=d0)
    assert k in _where(v, "anodes"), v[:3]
    parent = [(int(p), s) for p in range(N) for s, f in ((0, "leftChild"), (1, "rightChild"))
              if nodes["leftChild"][p] != -1 and nodes[f][p] == k]
    assert _where(v, "wnodes") == parent, v[:3]
    # a stale wnodes copy of a child's exact box
    p = int(np.where(nodes["leftChild"] != -1)[0][0])
    d = copy.deepcopy(d0)
    d["wnodes"].reshape(N, 2, 4, 4)[p, 1, 0, 2] -= np.float32(0.25)
    v = _check(fs, d)
    assert _where(v, "wnodes") == [(p, 1)] and len(v) == 1, v[:3]


def test_layouts_of_the_two_soups(dumps):
    """buildBVH(6) gives more than 8 reference leaves with scene-tree items (one titems record
    per item), buildBVH(2) at most 8 (the few-leaf layout: one record per leaf)."""
    assert dumps["soup6", 0][1]["nfew"] == 0 and dumps["soup6", 0][1]["n_titems"] > 8
    assert 0 < dumps["soup2", 0][1]["nfew"] == dumps["soup2", 0][1]["n_titems"] <= 8
