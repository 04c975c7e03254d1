"""Degenerate and non-finite shape records, shared by tests/test_degenerate_cpu.py and
tests/test_gpu_degenerate.py.

One small base scene, and nine families of record mutations aimed at the edge rules of
accel_bound.h::classify (non-finite coordinates, |radius|, zero-area and thin triangles, the
stored normal's length and its cosine to the vertices' plane, the wall basis, unknown types) and
at the overflow of the scene magnitude. Everything is a pure function of (family, seed, depth):
numpy's default_rng, the host scene library for the base records and oracle.build_bvh for the
tree. tests/test_degenerate_cpu.py shows on the CPU that the scalar emulation of the accelerated
walk agrees with the oracle on every one of them, that the mutations change what the rays see,
and that the oracle's frames are not mostly NaN.
"""
import functools

import numpy as np

import oracle
import rtamd
import test_accel_cpu as ta
import trace_rays as tr

W, H = 60, 44  # neither a multiple of the 8x8 tile: partial tiles in x and y, geometry behind them
N_RANDOM = 4000
SEEDS = (1, 2)
DEPTHS = (1, 6)
N_TRI, N_SPH, N_WALL = 60, 20, 6
f32 = np.float32
NAN, INF = float("nan"), float("inf")
VALUES = (0.0, NAN, INF, -INF, 3e38, -3e38, 1e-30, -1.0, 1e-7, 1e7)

FAMILIES = ("radius", "centre", "vertex", "zero_area", "stored_plane", "wall", "type", "thresholds", "huge")
# the Moller-Trumbore test never reads a triangle's stored plane: this family changes nothing under it
MT_BLIND = ("stored_plane",)
# Every family gives at least one of its shapes another accel_bound.h class than the base record
# has, under the barycentric test (tests/test_degenerate_cpu.py::test_every_family_changes_a_class
# classifies both records of every mutated shape): a refit from either set of records to the
# other changes a class, and the host has to rebuild the accelerator.


def _base_records(seed):
    rng = np.random.default_rng(1000 + seed)
    sc = rtamd.Scene()
    for i in range(N_TRI):
        c = rng.uniform(-6.5, 6.5, 3)
        v = c + rng.normal(size=(3, 3)) * 1.5
        sc.add_triangle(v[0], v[1], v[2], invert=bool(i % 2),
                        mat=rtamd.material(color=rng.uniform(0.1, 1, 3), specular=0.6 if i % 3 == 0 else 0.0))
    for i in range(N_SPH):
        sc.add_sphere(rng.uniform(-7, 7, 3), rng.uniform(0.4, 1.4),
                      mat=rtamd.material(color=rng.uniform(0.1, 1, 3), specular=0.5 if i % 2 else 0.0))
    for i in range(N_WALL):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        sc.add_wall(rng.uniform(-7, 3, 3), rng.uniform(2.5, 5), rng.uniform(2.5, 5), n,
                    mat=rtamd.material(color=rng.uniform(0.1, 1, 3), specular=0.3))
    sc.add_plane((0, 0, 1), (0, 0, -8), mat=rtamd.material(color=(0.3, 0.5, 0.3), specular=0.0))
    sc.add_plane((0, 1, 0), (0, 8, 0), mat=rtamd.material(color=(0.5, 0.4, 0.3), specular=0.2))
    sc.set_camera((3, -6, 22), 60, 4 / 3)
    sc.LookAt((0, 0, 0))
    sc.set_light((5, -15, 10), (1, 1, 1), 40)
    sc.buildBVH(1)
    return sc.serializeScene()


def _clean(a, dtype=rtamd.SHAPE_DTYPE):
    """A copy of records `a` with zeros in the layout's padding (numpy leaves it unset in copies)."""
    out = np.zeros(len(a), dtype)
    for name in dtype.names:
        out[name] = a[name]
    return out


def _ids(shapes, kind):
    return np.where(shapes["type"] == kind)[0]


def _unit(v):
    return v / np.linalg.norm(v)


def _set_triangle(s, i, p1, p2, p3, normal=None, d=None):
    """Vertices in float32; the stored plane is the vertices' own (from the rounded vertices, in
    double) unless given."""
    s["triP1"][i], s["triP2"][i], s["triP3"][i] = f32(p1), f32(p2), f32(p3)
    q1, q2, q3 = (s[k][i].astype(np.float64) for k in ("triP1", "triP2", "triP3"))
    if normal is None:
        normal = _unit(np.cross(q2 - q1, q3 - q1))
    s["planeNormal"][i] = f32(normal)
    s["planeD"][i] = f32(-np.dot(s["planeNormal"][i].astype(np.float64), q1)) if d is None else f32(d)


def _facing_triangle(rng, size):
    """A triangle of about `size` between the camera and the origin, roughly facing the camera."""
    c = np.array([rng.uniform(-7, 7), rng.uniform(-6, 4), rng.uniform(0, 9)])
    a, b = rng.normal(size=3), rng.normal(size=3)
    a[2] *= 0.2
    b[2] *= 0.2
    a = _unit(a)
    b = _unit(b - a * np.dot(a, b))
    return c, a, b, size


def _tilted_normal(s, i, cos):
    """Unit stored normal at cosine `cos` to the normal of triangle i's vertices, the stored plane
    through the triangle's centroid."""
    q = [s[k][i].astype(np.float64) for k in ("triP1", "triP2", "triP3")]
    nt = _unit(np.cross(q[1] - q[0], q[2] - q[0]))
    t = _unit(q[1] - q[0])
    n = cos * nt + np.sqrt(1.0 - cos * cos) * t
    n32 = f32(n)
    return n32, f32(-np.dot(n32.astype(np.float64), (q[0] + q[1] + q[2]) / 3))


# ---------------------------------------------------------------------------
# The families: each changes records of `s` in place and returns the changed shape ids.

def _radius(s, rng):
    sph = _ids(s, rtamd.SPHERE)[:len(VALUES)]
    s["sphereRadius"][sph] = f32(VALUES)
    return sph


def _centre(s, rng):
    sph = _ids(s, rtamd.SPHERE)[:len(VALUES)]
    for k, i in enumerate(sph):
        s["sphereCenter"][i, k % 3] = f32(VALUES[k])
    return sph


def _vertex(s, rng):
    tri = _ids(s, rtamd.TRIANGLE)[:3 * len(VALUES)]
    for k, i in enumerate(tri):  # each value in a coordinate of P1, of P2 and of P3; the stored plane stays
        s[("triP1", "triP2", "triP3")[k // len(VALUES)]][i, k % 3] = f32(VALUES[k % len(VALUES)])
    return tri


def _zero_area(s, rng):
    tri = _ids(s, rtamd.TRIANGLE)[:45]
    for k, i in enumerate(tri):
        if k % 3 == 0:
            s["triP3"][i] = s["triP1"][i]
        elif k % 3 == 1:  # P3 on the edge P1 P2, as float32 puts it
            s["triP3"][i] = s["triP1"][i] + (s["triP2"][i] - s["triP1"][i]) * f32(rng.uniform(0.1, 0.9))
        else:
            s["triP2"][i] = s["triP1"][i]
            s["triP3"][i] = s["triP1"][i]
    return tri


TILT_COS = (0.0, 0.03, 0.049, 0.051, 0.1)


def _stored_plane(s, rng):
    tri = _ids(s, rtamd.TRIANGLE)
    n = len(VALUES)
    for k, i in enumerate(tri[:n]):
        s["planeNormal"][i] = s["planeNormal"][i] * f32(VALUES[k])
    for k, i in enumerate(tri[n:2 * n]):
        s["planeD"][i] = f32(VALUES[k])
    tilt = tri[2 * n:2 * n + 3 * len(TILT_COS)]
    for k, i in enumerate(tilt):
        s["planeNormal"][i], s["planeD"][i] = _tilted_normal(s, i, TILT_COS[k % len(TILT_COS)])
    return tri[:2 * n + len(tilt)]


def _wall(s, rng):
    wal = _ids(s, rtamd.WALL)
    assert len(wal) == N_WALL
    s["wallWidth"][wal[0]] = f32(0.0)
    s["wallWidth"][wal[1]] = f32(-2.0)
    s["wallHeight"][wal[1]] = f32(-2.0)
    s["wallWidth"][wal[2]] = f32(INF)
    s["wallHeight"][wal[3]] = f32(NAN)
    s["planeNormal"][wal[4]] = (0.0, 1.0, 0.0)  # the intersection basis of a +-Y wall is NaN
    s["planeD"][wal[4]] = f32(-s["wallStart"][wal[4], 1])
    s["planeNormal"][wal[5]] = (0.0, 0.0, 0.0)
    return wal


def _type(s, rng):
    ids = np.concatenate([_ids(s, rtamd.TRIANGLE)[:16], _ids(s, rtamd.SPHERE)[:8], _ids(s, rtamd.WALL)[:2],
                          _ids(s, rtamd.PLANE)[:1]])
    s["type"][ids] = np.where(np.arange(len(ids)) % 2 == 0, 7, -1).astype(np.int32)
    return ids


SIN2 = tuple(1e-3 * k for k in (0.5, 0.999, 1.001, 2.0))
NORMAL_LEN = tuple(b * k for b in (1e-6, 1e6) for k in (0.999, 1.001))
COS = tuple(0.05 * k for k in (0.999, 1.001))


def _thresholds(s, rng):
    """Finite records on both sides of each classify rule: the thin ones long, the others large,
    all between the camera and the scene."""
    tri = _ids(s, rtamd.TRIANGLE)
    out = []
    k = 0
    for rep in range(2):
        for sin2 in SIN2:
            i = tri[k]
            c, a, b, L = _facing_triangle(rng, 14.0)
            th = np.arcsin(np.sqrt(sin2))
            p1 = c - a * (L / 2)
            _set_triangle(s, i, p1, p1 + a * L, p1 + (a * np.cos(th) + b * np.sin(th)) * L)
            out.append(i)
            k += 1
    for length in NORMAL_LEN:
        i = tri[k]
        c, a, b, L = _facing_triangle(rng, 5.0)
        _set_triangle(s, i, c - a * L / 2 - b * L / 3, c + a * L / 2 - b * L / 3, c + b * L * 2 / 3)
        n = s["planeNormal"][i].astype(np.float64) * length
        s["planeNormal"][i] = f32(n)
        s["planeD"][i] = f32(-np.dot(s["planeNormal"][i].astype(np.float64), s["triP1"][i].astype(np.float64)))
        out.append(i)
        k += 1
    for rep in range(2):
        for cos in COS:
            i = tri[k]
            c, a, b, L = _facing_triangle(rng, 5.0)
            _set_triangle(s, i, c - a * L / 2 - b * L / 3, c + a * L / 2 - b * L / 3, c + b * L * 2 / 3)
            s["planeNormal"][i], s["planeD"][i] = _tilted_normal(s, i, cos)
            out.append(i)
            k += 1
    return np.array(out)


def _huge(s, rng):
    """Finite records whose magnitude overflows float32 sums and squares."""
    tri, sph, wal = _ids(s, rtamd.TRIANGLE), _ids(s, rtamd.SPHERE), _ids(s, rtamd.WALL)
    s["triP2"][tri[0], 0] = f32(3e38)
    s["triP3"][tri[1], 1] = f32(-3e38)
    s["triP1"][tri[2]] = (3e38, -3e38, 3e38)
    s["sphereCenter"][sph[0], 2] = f32(-3e38)
    s["sphereCenter"][sph[1]] = (3e38, 3e38, 3e38)
    s["sphereRadius"][sph[2]] = f32(1e30)
    s["sphereRadius"][sph[3]] = f32(1e30)
    s["sphereCenter"][sph[3]] = (1e30, 0.0, 0.0)
    s["wallStart"][wal[0], 0] = f32(-3e38)
    return np.concatenate([tri[:3], sph[:4], wal[:1]])


_MUTATE = {"radius": _radius, "centre": _centre, "vertex": _vertex, "zero_area": _zero_area,
           "stored_plane": _stored_plane, "wall": _wall, "type": _type, "thresholds": _thresholds, "huge": _huge}
assert tuple(_MUTATE) == FAMILIES


@functools.lru_cache(maxsize=None)
def _records(family, seed):
    fs = _base_records(seed)
    s = _clean(fs.shapes)
    ids = np.zeros(0, np.int32)
    if family is not None:
        ids = np.sort(np.asarray(_MUTATE[family](s, np.random.default_rng(2000 + seed)))).astype(np.int32)
        assert len(np.unique(ids)) == len(ids)
    s.setflags(write=False)
    ids.setflags(write=False)
    return s, ids, fs.camera, fs.light


def _flat(family, seed, depth):
    s, _, cam, light = _records(family, seed)
    nodes, idx = oracle.build_bvh(s, depth)
    return rtamd.FlatScene(_clean(s), nodes, idx, _clean(cam, rtamd.CAMERA_DTYPE), _clean(light, rtamd.LIGHT_DTYPE))


def scene(family, seed, depth):
    """The base scene with the family's mutations, under the reference builder's tree of `depth`."""
    assert family in FAMILIES
    return _flat(family, seed, depth)


def base(seed, depth):
    """The unmutated scene."""
    return _flat(None, seed, depth)


def mutated_ids(family, seed):
    """The shapes the family changed (sorted int32)."""
    return _records(family, seed)[1].copy()


@functools.lru_cache(maxsize=None)
def _rays(seed):
    fs = _base_records(seed)  # every family keeps the base camera
    o, d = tr.pixel_rays(fs, W, H, [(x, y) for y in range(H) for x in range(W)])
    rng = np.random.default_rng(3000 + seed)
    o2, d2 = ta.random_rays(rng, N_RANDOM)
    o = np.ascontiguousarray(np.concatenate([o, o2]), f32)
    d = np.ascontiguousarray(np.concatenate([d, d2]), f32)
    lim = rng.uniform(1, 80, len(o)).astype(f32)
    for a in (o, d, lim):
        a.setflags(write=False)
    return o, d, lim


def rays(family, seed):
    """(origins, dirs, limits): the W x H camera rays, then N_RANDOM random rays; limits in [1, 80).
    The same for every family of a seed, so that mutated and base answers compare ray by ray."""
    assert family is None or family in FAMILIES
    return _rays(seed)


# Scenes by name, for the helpers keyed by a scene name (tests/trace_rays.py scene, and through
# it tests/gbuffer_ref.py and tests/ao_ref.py)
def key(family, seed, depth):
    return f"degenerate/{family}/{seed}/{depth}"


def scene_of_key(name):
    _, family, seed, depth = name.split("/")
    return scene(family, int(seed), int(depth))
