"""A plain reference of the device state the refit maintains (k_refit, prepare_animation and
flush_updates in rt_kernels.hip), for dumps of rt_debug_accel_dump (ComputeShader.debug_accel_dump).

check(dump, shapes, nodes, indices, prev=, fresh=) recomputes what every array must hold from the
host's current records alone and returns the violations, each (array, where, prims, what):

* exact, bit for bit: the staging copies, the packed records against a context that uploaded
  the same arrays whole, every copy of a node box, the slot boxes (the float32 union of the
  conservative boxes of the prims below, entry_cbox's rule), pbox, the grow-only content boxes;
* conservative, inequalities in float64: the back-face cone words against sampled directions,
  the Moller-Trumbore constants and slabs against the triangles below;
* tight: a cone word is the word of the reference's own cone (the unit normals' sum, the
  largest angle to it plus kConeMargin); the Moller-Trumbore constants, the grazing cone's
  opening and the slab exceed their float64 bound, taken against the stored axis, by at most
  1e-4 relative + 1e-4 absolute, a refit's axis is the normalised sum of the normals flipped
  towards the previous dump's axis, and neither the opening nor the slab is given up
  (k[3] = 2, k[9] infinite) without its reason.

grown_nodes(fs, ids, frames) gives the node records a group's frame slot must hold after the
frames given to the group (updateBVH once per frame), and shifted() builds frames that each leave
a trace in them (tests/test_group_refit_cpu.py, tests/test_gpu_group_refit_state.py).

Only four product functions are used as they are by check() (tests/native/refit_ref.cpp):
classify, classify_mt_tight's constants, cone_culls_q with ray_consts, and the cone word's
fields. Everything else is numpy in float64 or exact float32 min / max. A fifth, the packer
(accel_pack.h pack_accel), is used only by host_dump(): the dump of a fresh build without a GPU
is what the renderer would upload, code words included; check() never calls it.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rtamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDED = 1
CONE_NEVER = np.int32(-0x7F000000)  # 0x81000000
CONE_MARGIN = 2e-3                  # accel_math.h kConeMargin
K_U = 2.0 ** -24
PHI = np.radians([0.0, 60.0, 85.0, 89.0, 89.9])
INF = np.float32(np.inf)
_lib = None


def lib():
    """tests/native/refit_ref.cpp with the product's accel.cpp, built once per process."""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="refit_ref"), "refit_ref.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out,
                        os.path.join(ROOT, "tests", "native", "refit_ref.cpp"),
                        os.path.join(ROOT, "opengl-ray-tracer_amd", "csrc", "accel.cpp")], check=True)
        _lib = C.CDLL(out)
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def classify(shapes, origin_lim, mt):
    """(class, box (n, 6) float32: lo xyz, hi xyz) of every record: rta::classify."""
    s = rtamd.as_records(shapes, rtamd.SHAPE_DTYPE)
    cls = np.zeros(len(s), np.int32)
    box = np.zeros((len(s), 6), np.float32)
    assert lib().rr_classify(_p(s), len(s), C.c_float(float(origin_lim)), int(mt), _p(cls), _p(box)) == 0
    return cls, box


def mt_tri(shapes):
    """(ok, q (n, 6) float64: cr, X, esum, p1 xyz): rta::classify_mt_tight's MtTri."""
    s = rtamd.as_records(shapes, rtamd.SHAPE_DTYPE)
    ok = np.zeros(len(s), np.int32)
    q = np.zeros((len(s), 6), np.float64)
    assert lib().rr_mt_tri(_p(s), len(s), _p(ok), _p(q)) == 0
    return ok.astype(bool), q


def cone_culls(words, dirs):
    words = np.ascontiguousarray(words, np.int32)
    dirs = np.ascontiguousarray(dirs, np.float32)
    out = np.zeros(len(words), np.uint8)
    assert lib().rr_cone_culls(_p(words), _p(dirs), len(words), _p(out)) == 0
    return out.astype(bool)


def cone_decode(words):
    words = np.ascontiguousarray(words, np.int32)
    out = np.zeros((len(words), 4), np.int32)
    assert lib().rr_cone_decode(_p(words), len(words), _p(out)) == 0
    return out


def host_dump(fs, mt):
    """The dump of a freshly built accelerator, packed on the host (rr_build)."""
    s = rtamd.as_records(fs.shapes, rtamd.SHAPE_DTYPE)
    n = rtamd.as_records(fs.nodes, rtamd.NODE_DTYPE)
    i = np.ascontiguousarray(fs.indices, np.int32)
    assert lib().rr_build(_p(s), len(s), _p(n), len(n), _p(i), len(i), int(mt)) == 0
    fn = lib().rr_section
    fn.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    out = {}
    for sec, (name, dt) in enumerate(rtamd.ComputeShader._DUMP):
        need = np.zeros(1, np.int64)
        assert fn(sec, None, 0, need.ctypes.data) == 0
        a = np.zeros(int(need[0]) // np.dtype(dt).itemsize, dt)
        if a.size:
            assert fn(sec, a.ctypes.data, a.nbytes, need.ctypes.data) == 0
        out[name] = a.reshape(-1, 4) if (dt == "<f4" and name != "finfo") or name == "slots" else a
    for k, v in zip(["rec", "mt", "cone_cull", "n_local_wide", "n_wide", "P", "S", "N", "I", "n_titems", "nfew",
                     "n_refit", "built"], out["info"].tolist()):
        out[k] = v
    out["origin_lim"] = np.float32(out["finfo"][0])
    out["mt_z"] = out["finfo"][1:4].copy()
    return out


# ---------------------------------------------------------------------------
# the frames of a group's deferred growth (tests/test_gpu_group_refit_state.py)

SHIFT_DIRS = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32)


def grown_nodes(fs, ids, frames):
    """The node records after updateBVH (rtamd.update_bvh) once per frame, in order, from the
    scene's own: what every node-box copy of every frame slot must hold once the slot has
    flushed, whichever of the frames it rendered. frames: the records of `ids`, in that order."""
    h = rtamd.FlatScene(fs.shapes.copy(), fs.nodes.copy(), fs.indices, fs.camera, fs.light)
    ids = np.ascontiguousarray(ids, np.int32)
    for f in frames:
        h.shapes[ids] = f
        rtamd.update_bvh(h, ids)
    return h.nodes


def shifted(shapes, ids, k, step=64.0):
    """`shapes` with the shapes `ids` shifted by `step` along direction k of +x, -y, +z, -x, +y,
    -z (from the seventh frame on by twice the step, and so on): a sphere's centre, a wall's
    start, a triangle's vertices with planeD through the new first vertex. With a step above
    the scene's extent every frame of six sets an extreme of the boxes no other frame sets."""
    s = shapes.copy()
    d = SHIFT_DIRS[k % 6] * np.float32(step * (1 + k // 6))
    for i in ids:
        t = s["type"][i]
        if t == rtamd.SPHERE:
            s["sphereCenter"][i] += d
        elif t == rtamd.WALL:
            s["wallStart"][i] += d
        elif t == rtamd.TRIANGLE:
            for f in ("triP1", "triP2", "triP3"):
                s[f][i] += d
            s["planeD"][i] = np.float32(-(s["planeNormal"][i].astype(np.float64) @ s["triP1"][i].astype(np.float64)))
    return s


def boxes_differ(a, b):
    """the nodes whose box differs between two node arrays, bit for bit"""
    return np.where((_u(a["boundsMin"]) != _u(b["boundsMin"])).any(1) | (_u(a["boundsMax"]) != _u(b["boundsMax"])).any(1))[0]


# ---------------------------------------------------------------------------
# views of the wide records (rt_kernels.hip wide_box_f)

def slot_boxes(d):
    """(wide slots, 6) float32 view-like copy: lo xyz, hi xyz of slot 4*w + s."""
    ln, rec = d["lnodes"], d["rec"]
    nw = d["n_wide"]
    f = ln.reshape(nw, rec * 4)
    if rec == 17:
        return f[:, :64].reshape(nw, 4, 16)[:, :, :6].reshape(4 * nw, 6).copy()
    return f[:, :24].reshape(nw, 6, 4).transpose(0, 2, 1).reshape(4 * nw, 6).copy()


def set_slot_box(d, slot, comp, value):
    w, s = divmod(slot, 4)
    f = d["lnodes"].reshape(d["n_wide"], d["rec"] * 4)
    f[w, 16 * s + comp if d["rec"] == 17 else 4 * comp + s] = value


def cone_words(d):
    """barycentric records: the cone word of every slot (int32)."""
    f = d["lnodes"].reshape(d["n_wide"], 32)
    return f[:, 24:28].reshape(-1).view(np.int32).copy()


def set_cone_word(d, slot, word):
    w, s = divmod(slot, 4)
    d["lnodes"].view(np.uint32).reshape(d["n_wide"], 32)[w, 24 + s] = int(word) & 0xFFFFFFFF


def mt_consts(d):
    """Moller-Trumbore records: (slots, 10) float32: axis xyz, s, cr, u X, M, 18 M + 10.5 Esum, w, h0."""
    f = d["lnodes"].reshape(d["n_wide"], 68)
    return f[:, :64].reshape(-1, 4, 16)[:, :, 6:16].reshape(-1, 10).copy()


def set_mt_const(d, slot, k, value):
    w, s = divmod(slot, 4)
    d["lnodes"].reshape(d["n_wide"], 68)[w, 16 * s + 6 + k] = value


def codes(d):
    """the .w words of the wide records (child codes), as uint32."""
    f = d["lnodes"].reshape(d["n_wide"], d["rec"] * 4)
    return f[:, -4:].reshape(-1).view(np.uint32).copy()


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fields_differ(a, b):
    """records that differ in any field (padding bytes are not the record's)."""
    bad = np.zeros(len(a), bool)
    for name in a.dtype.names:
        x, y = a[name], b[name]
        if x.dtype.names:
            bad |= _fields_differ(x, y)
        else:
            bad |= (np.ascontiguousarray(x).view(np.uint32).reshape(len(a), -1) !=
                    np.ascontiguousarray(y).view(np.uint32).reshape(len(a), -1)).any(axis=1)
    return bad


def node_lists(nodes, indices):
    """Per reference node, the sorted array of the shapes it lists (its own as a leaf, its
    children's as an inner node)."""
    N = len(nodes)
    memo = {}

    def rec(k):
        if k in memo:
            return memo[k]
        n = nodes[k]
        if n["leftChild"] == -1:
            r = np.unique(indices[n["startShapeIdx"]:n["startShapeIdx"] + n["numShapes"]])
        else:
            r = np.union1d(rec(int(n["leftChild"])), rec(int(n["rightChild"])))
        memo[k] = r
        return r
    return [rec(k) for k in range(N)]


def conservative_boxes(d, shapes):
    """entry_cbox's rule per shape: (lo, hi) (S, 3) float32 and the shapes whose bound changed
    kind. The box of classify on the current record if the shape was BOUNDED when the boxes
    above it were built and is BOUNDED now; empty if it was not; infinite if it no longer is."""
    cls, box = classify(shapes, d["origin_lim"], d["mt"])
    was = d["shape_cls"]
    lo = np.where((was == BOUNDED)[:, None], box[:, :3], INF).astype(np.float32)
    hi = np.where((was == BOUNDED)[:, None], box[:, 3:], -INF).astype(np.float32)
    gone = (was == BOUNDED) & (cls != BOUNDED)
    lo[gone] = -INF
    hi[gone] = INF
    return lo, hi, cls != was


def _union(lo, hi, first, end):
    if end <= first:
        return np.full(3, INF, np.float32), np.full(3, -INF, np.float32)
    return lo[first:end].min(axis=0), hi[first:end].max(axis=0)


def check(d, shapes, nodes, indices, prev=None, fresh=None, all_slots=False, rng=None):
    """Violations of the refit's rules in dump `d`, given the host's current shape records, the
    node records every copy must hold, and the indices. prev: the dump before this flush (same
    accelerator; None skips the rules that need it). fresh: the dump of a context that uploaded
    the same arrays whole. all_slots: apply the cone and Moller-Trumbore rules to every slot
    (a fresh build) instead of the slots above a refit prim."""
    rng = rng or np.random.default_rng(7)
    V = []
    shapes = rtamd.as_records(shapes, rtamd.SHAPE_DTYPE)
    nodes = rtamd.as_records(nodes, rtamd.NODE_DTYPE)
    S, N = len(shapes), len(nodes)

    def bad(array, where, prims, what):
        V.append((array, where, prims, what))

    # --- records
    for k in np.where(_fields_differ(d["staging_shapes"], shapes))[0]:
        bad("staging_shapes", int(k), None, "differs from the host's record")
    for k in np.where(_fields_differ(d["staging_nodes"], nodes))[0]:
        bad("staging_nodes", int(k), None, "differs from the expected node record")
    nlo, nhi = nodes["boundsMin"], nodes["boundsMax"]
    if len(d["nodes"]):
        pk = d["nodes"].reshape(N, 2, 4)
        for k in np.where((_u(pk[:, 0, :3]) != _u(nlo)).any(1) | (_u(pk[:, 1, :3]) != _u(nhi)).any(1))[0]:
            bad("nodes", int(k), None, "packed box differs from the node's")
    if fresh is not None:
        for name in ("geo_lin", "geo_leaf", "mat", "nodes"):
            a, b = _u(d[name]), _u(fresh[name])
            if a.shape != b.shape:
                bad(name, -1, None, f"shape {a.shape} against the fresh upload's {b.shape}")
                continue
            for k in np.where((a != b).any(axis=1))[0][:8]:
                bad(name, int(k), None, "differs from the fresh upload")
    if not d["built"]:
        return V
    P = d["P"]
    ps = d["prim_shape"]
    if fresh is not None and fresh["built"] and P:
        of = np.full(S, -1, np.int64)
        of[fresh["prim_shape"][::-1]] = np.arange(fresh["P"])[::-1]
        a = d["prims"].reshape(P, 16).view(np.uint32)
        b = fresh["prims"].reshape(fresh["P"], 16).view(np.uint32)[of[ps]]
        diff = (a[:, :15] != b[:, :15]).any(1) | ((a[:, 15] & 3) != (b[:, 15] & 3)) | (of[ps] < 0)
        for p in np.where(diff)[0][:8]:
            bad("prims", int(p), [int(p)], f"differs from the fresh record of shape {ps[p]}")
    # --- copies of node boxes
    an = d["anodes"].reshape(N, 4, 4)
    for k in np.where((_u(an[:, 0, :3]) != _u(nlo)).any(1) | (_u(an[:, 1, :3]) != _u(nhi)).any(1))[0]:
        bad("anodes", int(k), None, "exact box differs from the node's")
    wn = d["wnodes"].reshape(N, 2, 4, 4)
    inner = np.where(nodes["leftChild"] != -1)[0]
    for s, f in ((0, "leftChild"), (1, "rightChild")):
        ch = nodes[f][inner]
        e = (_u(wn[inner, s, 0, :3]) != _u(nlo[ch])).any(1) | (_u(wn[inner, s, 1, :3]) != _u(nhi[ch])).any(1)
        for k in inner[e]:
            bad("wnodes", (int(k), s), None, "child exact box differs from the child's")
        e = (_u(wn[inner, s, 2, :3]) != _u(an[ch, 2, :3])).any(1) | (_u(wn[inner, s, 3, :3]) != _u(an[ch, 3, :3])).any(1)
        for k in inner[e]:
            bad("wnodes", (int(k), s), None, "child content box differs from the child's anodes content box")
    ti = d["titems"].reshape(-1, 2, 4)
    ref = d["titem_ref"]
    if len(ref):
        e = (_u(ti[:, 0, :3]) != _u(nlo[ref])).any(1) | (_u(ti[:, 1, :3]) != _u(nhi[ref])).any(1)
        for i in np.where(e)[0]:
            bad("titems", int(i), None, f"box differs from its reference leaf {ref[i]}'s")
    if prev is not None:
        for name in ("anodes", "wnodes", "titems"):
            e = (_u(d[name])[:, 3] != _u(prev[name])[:, 3])
            for k in np.where(e)[0][:8]:
                bad(name, int(k), None, ".w word changed")
        for k in np.where(codes(d) != codes(prev))[0][:8]:
            bad("lnodes", int(k), None, "child code changed")
    # --- slot boxes
    clo, chi, _ = conservative_boxes(d, shapes)
    plo, phi = clo[ps], chi[ps]
    slots = d["slots"]
    sb = slot_boxes(d)
    refit_prim = d["refit_of"][ps] >= 0
    n_ref = np.concatenate([[0], np.cumsum(refit_prim)])
    has = slots[:, 0] == 1
    noprune = (slots[:, 3] & 2) != 0
    touched = np.zeros(len(slots), bool)
    for q in np.where(has)[0]:
        f, e = int(slots[q, 1]), int(slots[q, 2])
        touched[q] = n_ref[e] > n_ref[f]
        if noprune[q]:
            if d["n_refit"] > 0 and not (np.all(sb[q, :3] == -INF) and np.all(sb[q, 3:] == INF)):
                bad("lnodes", int(q), None, "a kNoPrune slot is not infinite while a refit set exists")
            continue
        lo, hi = _union(plo, phi, f, e)
        if (_u(sb[q, :3]) != _u(lo)).any() or (_u(sb[q, 3:]) != _u(hi)).any():
            bad("lnodes", int(q), list(range(f, min(e, f + 4))),
                f"slot box {sb[q].tolist()} is not the union {lo.tolist() + hi.tolist()} of prims [{f}, {e})")
    touched &= ~noprune
    if prev is not None:
        psb = slot_boxes(prev)
        for q in np.where(has & ~touched & ~noprune & (_u(sb) != _u(psb)).any(1))[0]:
            bad("lnodes", int(q), None, "a slot with no refit prim below changed")
    # --- pbox
    if len(d["pbox"]):
        pb = d["pbox"].reshape(P, 2, 4)
        sel = refit_prim & (d["shape_cls"][ps] == BOUNDED)
        e = sel & ((_u(pb[:, 0, :3]) != _u(plo)).any(1) | (_u(pb[:, 1, :3]) != _u(phi)).any(1))
        for p in np.where(e)[0]:
            bad("pbox", int(p), [int(p)], "differs from the prim's conservative box")
    # --- content boxes (grow-only)
    if prev is not None:
        pan = prev["anodes"].reshape(N, 4, 4)
        entries = np.where(d["refit_of"] >= 0)[0]
        lists = node_lists(nodes, np.asarray(indices))
        for k in range(N):
            m = np.intersect1d(lists[k], entries)
            lo, hi = pan[k, 2, :3].copy(), pan[k, 3, :3].copy()
            if len(m):
                lo = np.minimum(lo, clo[m].min(axis=0))
                hi = np.maximum(hi, chi[m].max(axis=0))
            if (_u(an[k, 2, :3]) != _u(lo)).any() or (_u(an[k, 3, :3]) != _u(hi)).any():
                bad("anodes", int(k), None, "content box is not the previous one grown by the entries it lists"
                    if len(m) else "content box of a node listing no entry changed")
    # --- cones and Moller-Trumbore constants
    which = np.where(has & ~noprune & (touched | all_slots))[0]
    if d["mt"]:
        _check_mt(d, prev, shapes, ps, slots, which, all_slots, bad)
    else:
        _check_cones(d, prev, shapes, ps, slots, which, all_slots, rng, bad)
    return V


def _unit_normals(shapes, ids):
    """(ok, n (len, 3) float64 unit, raw float32 normals) of the walls and triangles `ids`."""
    t = shapes["type"][ids]
    raw = shapes["planeNormal"][ids]
    n = raw.astype(np.float64)
    l = np.sqrt((n * n).sum(axis=1))
    ok = ((t == rtamd.WALL) | (t == rtamd.TRIANGLE)) & (l > 1e-20) & np.isfinite(l)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / l[:, None]
    return ok, n, raw


def ref_cone(shapes, ids):
    """The reference cone over the shapes `ids`: (axis as stored (float32 values), half angle
    plus kConeMargin), or None where a shape has no normal or the normals cancel."""
    ok, n, _ = _unit_normals(shapes, ids)
    sn = n.sum(axis=0)
    l = np.sqrt((sn * sn).sum())
    if not ok.all() or not len(ids) or not l > 1e-6:
        return None
    af = (sn / l).astype(np.float32).astype(np.float64)
    cmin = np.clip((n @ af) / np.sqrt((af * af).sum()), -1.0, 1.0).min()
    return af, np.arccos(cmin) + CONE_MARGIN


def threshold_byte(t):
    """accel_math.h cone_word: t8 = floor((127^2 thr - 222) / 128) of thr = -sin(t)."""
    return int(np.floor((16129.0 * -np.sin(t) - 222.0) / 128.0))


def _check_cones(d, prev, shapes, ps, slots, which, all_slots, rng, bad):
    words = cone_words(d)
    pwords = cone_words(prev) if prev is not None else None
    W, D, NR, Q = [], [], [], []  # the sampled (word, direction, raw normal, slot) rows
    for q in which:
        f, e = int(slots[q, 1]), int(slots[q, 2])
        ids = ps[f:e]
        ok, n, raw = _unit_normals(shapes, ids)
        w = words[q]
        if not d["cone_cull"]:
            if w != CONE_NEVER:
                bad("lnodes", int(q), None, "a cone culls with culling off")
            continue
        if not ok.all() or e <= f:
            if w != CONE_NEVER:
                bad("lnodes", int(q), [int(f + np.argmin(ok))] if e > f else None,
                    "a cone over a shape without a normal (or a sphere / plane) is not kConeNever")
            continue
        if pwords is not None and pwords[q] == CONE_NEVER:
            if w != CONE_NEVER:
                bad("lnodes", int(q), None, "a cone that was kConeNever culls again")
            continue
        # the reference cone: axis = the unit normals' sum, half angle = the largest angle to
        # the axis as stored (float32), plus kConeMargin
        sn = n.sum(axis=0)
        l = np.sqrt((sn * sn).sum())
        expect_never, either = not l > 1e-6, False
        if not expect_never:
            af = (sn / l).astype(np.float32).astype(np.float64)
            cmin = np.clip((n @ af) / np.sqrt((af * af).sum()), -1.0, 1.0).min()
            t = np.arccos(cmin) + CONE_MARGIN
            # full at 1.5707 rad, and where the threshold byte would be -128 (cone_word)
            v = (16129.0 * -np.sin(min(t, np.pi / 2)) - 222.0) / 128.0
            expect_never = t >= 1.5707 + 1e-6 or np.floor(v + 1e-3) <= -128
            either = abs(t - 1.5707) <= 1e-6 or (np.floor(v - 1e-3) <= -128) != (np.floor(v + 1e-3) <= -128)
        if w != CONE_NEVER:
            # conservative: whenever the word culls a direction, the shader's float32 N.d of
            # every stored normal below is <= 0
            m = len(ids)
            pp = np.cross(n[:, None, :], rng.normal(size=(m, 2, 3)))
            pp /= np.sqrt((pp * pp).sum(axis=2))[:, :, None]
            dd = (np.cos(PHI)[None, None, :, None] * n[:, None, None, :] +
                  np.sin(PHI)[None, None, :, None] * pp[:, :, None, :])  # (m, 2, 5, 3)
            W.append(np.full(10 * m, w, np.int32))
            D.append(dd.reshape(-1, 3))
            NR.append(np.repeat(raw, 10, axis=0))
            Q.append(np.stack([np.full(10 * m, q), np.repeat(np.arange(f, e), 10)], axis=1))
        touched_now = not all_slots or len(ids) <= 2  # (a build's merged cone is this cone up to two prims)
        if not touched_now:
            continue
        if expect_never and not either:
            if w != CONE_NEVER:
                bad("lnodes", int(q), None, "the normals below cancel or span a half space: kConeNever expected")
            continue
        if w == CONE_NEVER:
            if not either and (pwords is not None or all_slots):
                bad("lnodes", int(q), None, f"a cone of half angle {t:.4f} rad went full for no reason")
            continue
        aq = cone_decode([w])[0]
        # accel_math.h cone_word: t8 = floor((127^2 thr - 222) / 128), thr = -sin(t); 1e-3 of a
        # step covers the last bits of the normals' sum, which the device adds in another order
        if np.abs(127.0 * af - aq[:3]).max() > 0.5 + 1e-3:
            bad("lnodes", int(q), None, f"cone axis bytes {aq[:3].tolist()} are not rint(127 a), a = {af.tolist()}")
        elif aq[3] > np.floor(v + 1e-3):
            bad("lnodes", int(q), None, f"cone threshold byte {aq[3]} is narrower than the half angle {t:.5f} rad "
                f"(with kConeMargin) allows: {np.floor(v + 1e-3):.0f}")
        elif aq[3] < np.floor(v - 1e-3):
            bad("lnodes", int(q), None, f"cone threshold byte {aq[3]} is wider than the half angle {t:.5f} rad "
                f"needs: {np.floor(v - 1e-3):.0f}")
        # (the byte's floor leaves -axis unculled from about 1.44 rad on: 128 t8 <= -127^2 + 221)
        if t < 1.5 and np.floor(v - 1e-3) >= -124 and not cone_culls([w], [-af])[0]:
            bad("lnodes", int(q), None, "the cone does not cull the direction opposite its axis")
    if W:
        D = np.concatenate(D).astype(np.float32)
        NR = np.concatenate(NR).astype(np.float32)
        Q = np.concatenate(Q)
        nd = (NR[:, 0] * D[:, 0] + NR[:, 1] * D[:, 1]) + NR[:, 2] * D[:, 2]  # float32, no contraction
        wrong = cone_culls(np.concatenate(W), D) & (nd > 0)
        seen = set()
        for i in np.where(wrong)[0]:
            if tuple(Q[i]) not in seen:
                seen.add(tuple(Q[i]))
                bad("lnodes", int(Q[i][0]), [int(Q[i][1])], f"the cone culls a direction with N.d = {nd[i]:.3g} > 0")




def _check_mt(d, prev, shapes, ps, slots, which, all_slots, bad):
    """The Moller-Trumbore record of each slot in `which` (refit_slot_mt; on a fresh build,
    all_slots, build_cones_mt's). Conservative for any stored axis. Tight against the stored
    axis: the opening k[3] and the slab k[8] +- k[9] exceed what the triangles below need by
    at most 1e-4 relative + 1e-4 absolute (the kernel's own margins are 1e-6 + 2e-5 and
    1e-5), and neither is given up (k[3] = 2, k[9] infinite) without its reason. A refit's
    axis is the float32 of the normalised sum of the normals, each flipped towards the
    previous dump's axis. A build's merged cone is that tight only up to two triangles, so
    on a fresh build the opening's tightness is asked of those slots alone."""
    K = mt_consts(d).astype(np.float64)
    PK = mt_consts(prev).astype(np.float64) if prev is not None else None
    ok_all, q_all = mt_tri(shapes)
    z = d["mt_z"].astype(np.float64)
    for q in which:
        f, e = int(slots[q, 1]), int(slots[q, 2])
        ids = ps[f:e]
        ok = ok_all[ids]
        k = K[q]
        if not ok.any():
            if not (np.all(k[4:9] == 0) and k[9] == np.inf):
                bad("lnodes", int(q), None, "no bounded triangle below: k[4..8] = 0 and k[9] infinite expected")
            if k[3] != 2.0:
                bad("lnodes", int(q), None, "no bounded triangle below: k[3] = 2 expected")
            continue
        tri = ids[ok]
        s = shapes[tri]
        e1 = (s["triP2"] - s["triP1"]).astype(np.float64)  # float32 edges, as the device forms them
        e2 = (s["triP3"] - s["triP1"]).astype(np.float64)
        n = np.cross(e1, e2)
        n /= np.sqrt((n * n).sum(axis=1))[:, None]
        a = k[:3]
        sm = np.sqrt(np.minimum(((n - a) ** 2).sum(1), ((n + a) ** 2).sum(1))).max()
        tq = q_all[tri]
        cr, X, es = tq[:, 0].min(), tq[:, 1].max(), tq[:, 2].max()
        M = np.sqrt(((tq[:, 3:6] - z) ** 2).sum(axis=1)).max()
        pr = [int(f + np.where(ok)[0][0])]
        # a refit's axis, and whether the flipped normals cancel (then a full cone and no slab)
        cancels = False
        if PK is not None and not all_slots:
            a0 = PK[q, :3]
            sg = np.where((n[:, 0] * a0[0] + n[:, 1] * a0[1]) + n[:, 2] * a0[2] < 0, -1.0, 1.0)
            sn = (n * sg[:, None]).sum(axis=0)
            l = np.sqrt((sn * sn).sum())
            cancels = not l > 1e-6
            want = a0 if cancels else sn / l
            if np.abs(a - want).max() > (0.0 if cancels else 1e-6):
                bad("lnodes", int(q), pr, f"axis {a.tolist()} is not the normalised sum of the normals flipped towards "
                    f"the previous axis, {want.tolist()}")
        tight3 = not all_slots or (ok.all() and len(ids) <= 2)
        sv = sm * (1.0 + 1e-6) + 2e-5
        if k[3] == 2.0:
            if tight3 and d["cone_cull"] and not cancels and sv < 1.3633 - 1e-5:
                bad("lnodes", int(q), pr, f"k[3] = 2 (any direction grazes) where the largest |n -+ a| is {sm:.9g}")
        elif k[3] < sm:
            bad("lnodes", int(q), pr, f"k[3] = {k[3]:.9g} is below the largest |n -+ a| = {sm:.9g}")
        elif tight3 and k[3] > sm * (1.0 + 1e-4) + 1e-4:
            bad("lnodes", int(q), pr, f"k[3] = {k[3]:.9g} is looser than the largest |n -+ a| = {sm:.9g} by more than 1e-4")
        for i, (lo_ok, bound, name) in enumerate([
                (k[4] <= cr, cr, "k[4] above the smallest cr"), (k[5] >= K_U * X, K_U * X, "k[5] below kU max X"),
                (k[6] >= M, M, "k[6] below the largest |p1 - mt_z|"),
                (k[7] >= 18.0 * M + 10.5 * es, 18.0 * M + 10.5 * es, "k[7] below 18 M + 10.5 max esum")]):
            if not lo_ok:
                bad("lnodes", int(q), pr, f"{name}: {k[4 + i]:.9g} against {bound:.9g}")
            elif abs(k[4 + i] - bound) > 1e-4 * abs(bound) + 1e-4:
                bad("lnodes", int(q), pr, f"k[{4 + i}] = {k[4 + i]:.9g} is looser than {bound:.9g} by more than 1e-4")
        if np.isinf(k[9]):
            if ok.all() and not cancels:
                bad("lnodes", int(q), pr, "no slab (k[9] infinite) over bounded triangles alone whose normals do not cancel")
            continue
        if not ok.all():
            bad("lnodes", int(q), [int(f + np.argmin(ok))], "a finite slab over a shape that is no bounded triangle")
            continue
        v = np.concatenate([s["triP1"], s["triP2"], s["triP3"]]).astype(np.float64) @ a
        if v.min() < k[8] - k[9] or v.max() > k[8] + k[9]:
            bad("lnodes", int(q), pr, f"the slab {k[8]:.9g} +- {k[9]:.9g} misses a vertex: a.v in [{v.min():.9g}, {v.max():.9g}]")
            continue
        wc, h0 = 0.5 * (v.min() + v.max()), 0.5 * (v.max() - v.min())
        tol = 1e-4 * (abs(wc) + 1.0)
        if k[9] > h0 * (1.0 + 1e-4) + tol or abs(k[8] - wc) > tol:
            bad("lnodes", int(q), pr, f"the slab {k[8]:.9g} +- {k[9]:.9g} is looser than {wc:.9g} +- {h0:.9g} by more than 1e-4")
