"""A plain restatement of the device LBVH (csrc/lbvh.hip), in numpy and Python.

For a given shape array the LBVH is fully determined: primitive centres, their
bounds, 30-bit Morton codes, the unique keys `code << 32 | shape`, and the binary
radix tree over the sorted keys (Karras, HPG 2012, section 3: a node covers a
range of sorted keys and splits it where the first bit that differs between its
first and last key changes). The build keeps IEEE float32 arithmetic with no
contraction and correctly rounded division and square root, so every step is
restated here in np.float32, in the kernels' operation order, and the tree can be
compared node for node.

The tree is built top-down from that definition; nothing here searches for a
node's range the way k_lbvh_inner does.
"""
import functools

import numpy as np

import oracle
import rtamd

F = np.float32
KEY_BITS = 64


def _normalize(x, y, z):
    s = F(1.0) / np.sqrt(x * x + y * y + z * z)
    return x * s, y * s, z * s


def centres(shapes):
    """[n, 3] float32: the centre each shape is sorted by (the reference's split())."""
    shapes = rtamd.as_records(shapes, rtamd.SHAPE_DTYPE)
    n = len(shapes)
    out = np.zeros((n, 3), F)  # planes keep (0, 0, 0)
    typ = shapes["type"]
    with np.errstate(all="ignore"):
        sph = typ == rtamd.SPHERE
        out[sph] = shapes["sphereCenter"][sph]

        w = np.where(typ == rtamd.WALL)[0]
        if w.size:
            nx, ny, nz = (shapes["planeNormal"][w, a].astype(F) for a in range(3))
            zero = np.zeros(w.size, F)
            steep = np.abs(nx) > np.abs(ny)
            ax, ay, az = _normalize(-nz, zero, nx)
            bx, by, bz = _normalize(zero, -nz, ny)
            t1 = (np.where(steep, ax, bx), np.where(steep, ay, by), np.where(steep, az, bz))
            # cross(n, t1)
            t2 = _normalize(ny * t1[2] - t1[1] * nz, nz * t1[0] - t1[2] * nx, nx * t1[1] - t1[0] * ny)
            width, height = shapes["wallWidth"][w].astype(F), shapes["wallHeight"][w].astype(F)
            for a in range(3):
                start = shapes["wallStart"][w, a].astype(F)
                end = (start + width * t1[a]) + height * t2[a]
                out[w, a] = (start + end) * F(0.5)

        t = np.where(typ == rtamd.TRIANGLE)[0]
        if t.size:
            p1, p2, p3 = shapes["triP1"][t].astype(F), shapes["triP2"][t].astype(F), shapes["triP3"][t].astype(F)
            out[t] = ((p1 + p2) + p3) / F(3.0)
    return out


def morton_codes(c):
    """30-bit Morton codes of the centres c inside the bounds of the finite ones."""
    n = len(c)
    ok = np.isfinite(c).all(axis=1)
    q = np.zeros((n, 3), np.uint64)
    with np.errstate(all="ignore"):
        for a in range(3):
            if not ok.any():
                break
            v = c[ok, a]
            lo, hi = v.min(), v.max()
            ext = F(hi - lo)
            u = (v - lo) / ext if ext > 0 else np.full(v.shape, F(0.5))
            u = np.fmin(np.fmax(u, F(0.0)), F(1.0))  # fmaxf / fminf: a NaN gives the other operand
            q[ok, a] = np.fmin(u * F(1024.0), F(1023.0)).astype(np.int64).astype(np.uint64)
    code = np.zeros(n, np.uint64)
    for bit in range(10):  # x, y, z interleaved, x highest
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - a)
    return code


def keys_of(shapes):
    """uint64 keys in shape order: code << 32 | shape index (all distinct)."""
    code = morton_codes(centres(shapes))
    return (code << np.uint64(32)) | np.arange(len(code), dtype=np.uint64)


def common_bits(a, b):
    """Leading bits two 64-bit keys share (64 for equal keys)."""
    return KEY_BITS - (int(a) ^ int(b)).bit_length()


def split_after(keys, first, last):
    """The largest index in [first, last] whose key shares more leading bits with
    keys[first] than keys[first] shares with keys[last]."""
    top = (int(keys[first]) ^ int(keys[last])).bit_length() - 1  # the first bit that differs
    same = ((keys[first:last + 1] ^ keys[first]) >> np.uint64(top)) == 0
    return first + int(np.nonzero(same)[0].max())


def leaf_boxes(shapes, indices):
    """The reference's growToInclude box of each sorted shape (oracle.update_bvh from
    empty boxes, on a forest of one-shape leaves)."""
    n = len(indices)
    leaves = np.zeros(n, rtamd.NODE_DTYPE)
    leaves["boundsMin"] = F(np.inf)
    leaves["boundsMax"] = F(-np.inf)
    leaves["leftChild"] = leaves["rightChild"] = -1
    leaves["startShapeIdx"] = np.arange(n)
    leaves["numShapes"] = 1
    cam, light = np.zeros(1, rtamd.CAMERA_DTYPE), np.zeros(1, rtamd.LIGHT_DTYPE)
    forest = rtamd.FlatScene(shapes, leaves, indices, cam, light)
    oracle.update_bvh(forest, np.arange(n, dtype=np.int32))
    return forest.nodes["boundsMin"].copy(), forest.nodes["boundsMax"].copy()


def build(shapes):
    """(nodes, indices, sorted keys) of the LBVH over `shapes`, in the FlatNode layout:
    leaf j is node j, the inner node with Karras index i is node 2n-2-i."""
    shapes = rtamd.as_records(shapes, rtamd.SHAPE_DTYPE)
    n = len(shapes)
    keys = keys_of(shapes)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    indices = order.astype(np.int32)
    nodes = np.zeros(max(2 * n - 1, 0), rtamd.NODE_DTYPE)
    if n == 0:
        return nodes, indices, skeys
    lo, hi = leaf_boxes(shapes, indices)
    nodes["boundsMin"][:n], nodes["boundsMax"][:n] = lo, hi
    nodes["leftChild"][:n] = nodes["rightChild"][:n] = -1
    nodes["startShapeIdx"][:n] = np.arange(n)
    nodes["numShapes"][:n] = 1

    def node_of(first, last, karras):
        return first if first == last else 2 * n - 2 - karras

    made = []  # inner nodes, parents before children
    todo = [(0, n - 1, 0)] if n > 1 else []
    while todo:
        first, last, karras = todo.pop()
        me = node_of(first, last, karras)
        g = split_after(skeys, first, last)
        nodes["leftChild"][me] = node_of(first, g, g)
        nodes["rightChild"][me] = node_of(g + 1, last, g + 1)
        nodes["startShapeIdx"][me] = first
        nodes["numShapes"][me] = last - first + 1
        made.append(me)
        if first < g:
            todo.append((first, g, g))
        if g + 1 < last:
            todo.append((g + 1, last, g + 1))
    bmin, bmax = nodes["boundsMin"], nodes["boundsMax"]
    for me in reversed(made):  # children before parents; glm::min / glm::max
        a, b = nodes["leftChild"][me], nodes["rightChild"][me]
        bmin[me] = np.where(bmin[b] < bmin[a], bmin[b], bmin[a])
        bmax[me] = np.where(bmax[a] < bmax[b], bmax[b], bmax[a])
    return nodes, indices, skeys


# ---------------------------------------------------------------------------
# The scenes the CPU tests of this restatement and the device comparison share.

COUNTS = [2, 3, 63, 64, 65, 255, 256, 257, 1000]  # wave and block edges of n and of n - 1


def _finish(sc):
    sc.set_camera((0, 0, 30), 60, 4 / 3)
    sc.LookAt((0, 0, 0))
    sc.set_light((10, -30, 20), (1, 1, 1), 40)
    sc.buildBVH(1)
    return sc.serializeScene()


def _with_shapes(fs, shapes):
    """fs with another shape array, under a reference tree of it (what an upload needs)."""
    nodes, idx = oracle.build_bvh(shapes, 5)
    return rtamd.FlatScene(shapes, nodes, idx, fs.camera, fs.light)


def _counted(soup, n):
    """The soup's first n shapes, reordered so that the shapes whose centres set the
    bounds sit at the end of the array: in the last, partial wave of the bounds
    reduction as far as it has room (for n = 65 and 257 that is one shape)."""
    shapes = soup.shapes[:n].copy()
    c = centres(shapes)
    extreme = []
    for a in range(3):
        for k in (int(np.argmax(c[:, a])), int(np.argmin(c[:, a]))):
            if k not in extreme:
                extreme.append(k)
    rest = [k for k in range(n) if k not in extreme]
    return _with_shapes(soup, shapes[rest + extreme[::-1]])


def _duplicates():
    sc = rtamd.Scene()
    for i in range(200):
        sc.add_sphere((1.5, -2.25, 3.0), 0.01 * (i + 1))
    return _finish(sc)


def _flat():
    rng = np.random.default_rng(11)
    sc = rtamd.Scene()
    for _ in range(300):
        x, y = rng.uniform(-10, 10, 2)
        sc.add_sphere((x, y, 2.5), rng.uniform(0.05, 0.5))
    return _finish(sc)


def _lattice():
    sc = rtamd.Scene()
    for _ in range(2):
        for x in range(10):
            for y in range(10):
                for z in range(10):
                    sc.add_sphere((x - 4.5, y - 4.5, z - 4.5), 0.1)
    return _finish(sc)


def _outlier():
    rng = np.random.default_rng(12)
    sc = rtamd.Scene()
    for _ in range(500):
        v = np.array([1.0, 2.0, 3.0]) + rng.uniform(-5e-4, 5e-4, (3, 3))
        sc.add_triangle(v[0], v[1], v[2])
    sc.add_sphere((1e4, 2.0, 3.0), 1.0)
    return _finish(sc)


def _non_finite(soup):
    shapes = soup.shapes[900:].copy()  # 100 triangles, then the spheres, walls and the plane
    shapes["sphereRadius"][np.where(shapes["type"] == rtamd.SPHERE)[0][3]] = F(np.inf)
    shapes["triP2"][np.where(shapes["type"] == rtamd.TRIANGLE)[0][17], 0] = F(np.inf)
    return _with_shapes(soup, shapes)


@functools.lru_cache(maxsize=None)
def _soup(seed, n_tri):
    from test_gpu_parity import _soup as soup_of  # the adversarial soup of the accelerator's tests
    return soup_of(seed, n_tri)


SCENES = {
    **{"n%d" % n: (lambda n=n: _counted(_soup(7, 1000), n)) for n in COUNTS},
    "duplicates": _duplicates,  # ext = 0 on every axis: equal codes, the index bits decide
    "flat": _flat,              # one degenerate axis
    "lattice": _lattice,        # equal codes in pairs
    "outlier": _outlier,        # all but one shape in one cell
    "mixed": lambda: _soup(3, 2500),  # planes, ±Y and slanted walls, slivers
    "non_finite": lambda: _non_finite(_soup(7, 1000)),
    "config2": lambda: rtamd.generate(2, 0, 320, 240),
    "config3": lambda: rtamd.generate(3, 0, 320, 240),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The FlatScene of one of SCENES (shared: do not modify)."""
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """build() of that scene's shapes (shared: do not modify)."""
    return build(scene(name).shapes)


def first_difference(fs, nodes, indices, ref):
    """Where a device tree (nodes, indices) first departs from build()'s (ref): None, or
    a message with the first differing sorted position and both keys."""
    rnodes, rindices, rkeys = ref
    keys = keys_of(fs.shapes)
    if len(indices) != len(rindices) or len(nodes) != len(rnodes):
        return "sizes: %d nodes, %d indices against %d, %d" % (len(nodes), len(indices), len(rnodes), len(rindices))
    bad = np.nonzero(indices != rindices)[0]
    if bad.size:
        j = int(bad[0])
        dev = int(keys[indices[j]]) if 0 <= indices[j] < len(keys) else -1
        return "indices differ at %d sorted positions, first %d: device shape %d (key %#018x), reference shape %d " \
               "(key %#018x)" % (bad.size, j, indices[j], dev, rindices[j], int(rkeys[j]))
    for f in ("leftChild", "rightChild", "startShapeIdx", "numShapes", "boundsMin", "boundsMax"):
        a, b = nodes[f], rnodes[f]
        if not np.array_equal(a, b):
            k = int(np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0][0])
            j = int(rnodes["startShapeIdx"][k])
            last = j + int(rnodes["numShapes"][k]) - 1
            return "%s differs at node %d (reference range [%d, %d], keys %#018x .. %#018x): device %s, reference %s" \
                   % (f, k, j, last, int(rkeys[j]), int(rkeys[last]), a[k].tolist(), b[k].tolist())
    return None
