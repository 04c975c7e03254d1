"""The refit's maps (csrc/refit_plan.h plan_refit: what prepare_animation uploads) against a
brute-force restatement, on the CPU (tests/native/refit_plan_check.cpp).

Per entry its nodes (the leaves listing it and every ancestor, found by scanning all nodes for a
parent), its geo_leaf slots, prims and wide slots (every slot, local or scene tree and not kNoPrune,
whose prim range holds one of its prims); per dirty slot its range, the float32 min / max of pbox
over its prims outside the set and the list of those inside, big slots (more than kBigList refit
prims) first; direct_reads by its definition; refit_of -1 outside the set; every CSR offset pair
bracketing exactly its list, the sections following each other to the end of the buffer.

Scenes: test_gpu_refit_state.py's soups, soup6 (per-item titems) with 3 entries (a triangle, a
sphere and the plane, whose scene-tree slots are kNoPrune and must stay out), soup2 (few-leaf
titems) with 300 triangles under one slot (a big slot, asserted); soup6 with one index entry
rewritten so that a shape is listed by two leaves (the reference builder lists every shape once,
so the records are edited and the boxes grown by updateBVH); an empty set; a context without an
accelerator; a Moller-Trumbore build (no scene tree).
"""
import os
import subprocess

import numpy as np
import pytest

import refit_ref as rr
import rtamd
from test_gpu_refit_state import _set, _top_slot_shapes, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "build/refit_plan_check"], check=True)
    return os.path.join(ROOT, "tests", "native", "build", "refit_plan_check")


def _listed_twice(fs):
    """soup6 with the first index entry of its second leaf replaced by the first shape of its
    first leaf, the boxes grown to hold it: (scene, that shape)."""
    h = rtamd.FlatScene(fs.shapes.copy(), fs.nodes.copy(), fs.indices.copy(), fs.camera, fs.light)
    leaves = [k for k in range(len(h.nodes)) if h.nodes["leftChild"][k] == -1 and h.nodes["numShapes"][k] > 0]
    sh = int(h.indices[h.nodes["startShapeIdx"][leaves[0]]])
    h.indices[h.nodes["startShapeIdx"][leaves[1]]] = sh
    rtamd.update_bvh(h, np.array([sh], np.int32))
    return h, sh


def _case(name):
    rng = np.random.default_rng(41)
    if name == "twice":
        fs, sh = _listed_twice(scene("soup6"))
        assert int((fs.indices == sh).sum()) == 2
        return fs, np.array([sh, int(fs.indices[-1])], np.int32), 0
    fs = scene("soup2" if name == "few" else "soup6")
    if name == "few":
        return fs, _set(fs, 300, rng, _top_slot_shapes(rr.host_dump(fs, 0), 340)), 0
    if name == "empty":
        return fs, np.zeros(0, np.int32), 0
    if name == "item":  # a triangle, a sphere and the plane (unbounded: under the kNoPrune slots)
        t = fs.shapes["type"]
        ids = [rng.choice(np.where(t == rtamd.TRIANGLE)[0]), np.where(t == rtamd.SPHERE)[0][0], np.where(t == 1)[0][0]]
        return fs, np.sort(np.array(ids, np.int32)), 0
    return fs, _set(fs, 65, rng), int(name == "mt")


@pytest.mark.parametrize("name", ["item", "few", "twice", "empty", "noaccel", "mt"])
def test_refit_plan(exe, tmp_path, name):
    fs, ids, mt = _case(name)
    s = rtamd.as_records(fs.shapes, rtamd.SHAPE_DTYPE)
    n = rtamd.as_records(fs.nodes, rtamd.NODE_DTYPE)
    i = np.ascontiguousarray(fs.indices, np.int32)
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(s), len(n), len(i), len(ids), mt], np.int32).tobytes())
        for a in (s, n, i, np.ascontiguousarray(ids, np.int32)):
            f.write(a.tobytes())
    r = subprocess.run([exe, path, "any" if name == "empty" else name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refit_plan_check ok" in r.stdout and " 0 failed" in r.stdout, r.stdout
