"""The reference geometry buffer of tests/test_gbuffer_cpu.py and tests/test_gpu_gbuffer.py,
from the oracle alone.

Camera rays from trace_rays.pixel_rays (oracle.get_ray, NDC in float32), shape and depth from
trace_rays.oracle_trace (the reference walk), position from oracle.intersect of the winning
shape, and the normal from the float32 restatement of include/rt_api.h: for a sphere
v * (1 / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z)) with v = p - centre, else the record's
planeNormal. tests/test_gbuffer_cpu.py shows that restatement is the oracle's own normal.
"""
import ctypes as C
import functools

import numpy as np

import oracle
import rtamd
import trace_rays as tr

PLANES = ("shape", "depth", "normal", "position")
W0, H0 = tr.CAM_W, tr.CAM_H     # 96 x 54: 54 is no multiple of the 8-row tile
W1, H1 = 41, 27                 # neither side a multiple of the tile
WA, HA = 160, 90                # the animated frame: the moved wheels cover more pixels
EDGE_SIZES =((1, 1), (8, 8), (9, 1), (1, 9), (W1, H1))
FAR_BACK, FAR_FOV = 2000.0, 1.0
ANIM_FRAMES = 30                # half a radian of wheel turn, as tests/test_gpu_trace.py


def image_row(r, y0, stripe, period):
    """Image row of compact row r (rt_dispatch_rows_ex)."""
    return y0 + (r // stripe) * period + r % stripe


def dispatch_rows(height, y0, stripe, period, out_rows):
    """[(r, y)] of the compact rows a dispatch writes: those whose image row is inside the frame."""
    rows = [(r, image_row(r, y0, stripe, period)) for r in range(out_rows)]
    return [(r, y) for r, y in rows if y < height]


def wheel_move():
    """(ids, records) of the car's wheels after ANIM_FRAMES frames of bench.wheel_frames."""
    import bench
    ids, frames = bench.wheel_frames(tr.scene("cfg3"), ANIM_FRAMES)
    return ids, frames[-1]


@functools.lru_cache(maxsize=None)
def scene(key):
    """"cfg3": trace_rays.scene; "cfg3:far": its camera FAR_BACK units back along -Front with
    fov FAR_FOV; "cfg3:anim": the car with its wheels moved and oracle.update_bvh's nodes;
    "cfg3:ties": every shape twice (tests/test_accel_cpu.py::test_accel_ties)."""
    name, _, variant = key.partition(":")
    fs = tr.scene(name)
    if variant == "":
        return fs
    if variant == "far":
        cam = np.array(fs.camera, rtamd.CAMERA_DTYPE).reshape(-1)[:1].copy()
        cam["Position"][0] = cam["Position"][0] - np.float32(FAR_BACK) * cam["Front"][0]
        cam["fov"][0] = FAR_FOV
        return rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, cam, fs.light)
    if variant == "anim":
        ids, rec = wheel_move()
        host = rtamd.FlatScene(fs.shapes.copy(), fs.nodes.copy(), fs.indices, fs.camera, fs.light)
        host.shapes[ids] = rec
        oracle.update_bvh(host, ids)
        return host
    if variant == "ties":
        shapes = np.concatenate([fs.shapes, fs.shapes.copy()])
        nodes, idx = oracle.build_bvh(shapes, 25)
        return rtamd.FlatScene(shapes, nodes, idx, fs.camera, fs.light)
    raise KeyError(key)


def restated_normals(shapes, shape, position):
    """include/rt_api.h's normal of hit pixels i (shape[i] >= 0, position[i, :3] the hit
    point), float32 throughout; zeros elsewhere. [n, 4], w = 0."""
    f = np.float32
    n = np.zeros((len(shape), 4), f)
    hit = shape >= 0
    rec = shapes[np.where(hit, shape, 0)]
    n[:, :3] = rec["planeNormal"]
    sph = hit & (rec["type"] == rtamd.SPHERE)
    v = (position[:, :3] - rec["sphereCenter"]).astype(f)
    with np.errstate(all="ignore"):
        s = f(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=f)
        n[sph, :3] = (v * s[:, None])[sph]
    n[~hit] = 0
    return n


@functools.lru_cache(maxsize=None)
def rays(key, W, H):
    """(origins, dirs) of the W x H frame's camera rays, row-major."""
    o, d = tr.pixel_rays(scene(key), W, H, [(x, y) for y in range(H) for x in range(W)])
    for a in (o, d):
        a.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def reference(key, W, H, mt):
    """{plane: array} of the whole W x H frame: shape [H, W] int32, depth [H, W] float32,
    normal and position [H, W, 4] float32. Computed once per (scene, size, mt), read-only."""
    fs = scene(key)
    o, d = rays(key, W, H)
    shape, depth, _ = tr.oracle_trace(fs, o, d, np.full(len(o), np.inf, np.float32), mt)
    position = np.zeros((len(o), 4), np.float32)
    for i in np.where(shape >= 0)[0]:
        kind, p = oracle.intersect(fs.shapes[shape[i]:shape[i] + 1], o[i], d[i], mt)
        assert kind == 1  # INNER: the shape the walk chose is hit by this test
        position[i, :3] = p
        position[i, 3] = 1.0
    normal = restated_normals(fs.shapes, shape, position)
    out = {"shape": shape.reshape(H, W), "depth": depth.reshape(H, W), "normal": normal.reshape(H, W, 4),
           "position": position.reshape(H, W, 4)}
    for a in out.values():
        a.setflags(write=False)
    return out


def shadow_origins(key, W, H, mt):
    """Per pixel the origin of the shadow ray the oracle's main() casts from the camera ray's
    hit (orc_pixel_rays with maxBounces = 1, cap = 2): hit + normal * 1e-3 with the oracle's
    own normal. ([H * W, 3] float32, [H * W] bool: the pixel has one.)"""
    fs = scene(key)
    fs = rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, fs.camera, fs.light)
    fn = oracle.lib().orc_pixel_rays
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    p = oracle.params(W, H, 1, True, False, mt)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    cam = rtamd.as_records(fs.camera, rtamd.CAMERA_DTYPE)
    light = rtamd.as_records(fs.light, rtamd.LIGHT_DTYPE)
    o, d = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)
    lim, kind = np.zeros(2, np.float32), np.zeros(2, np.int32)
    out, have = np.zeros((H * W, 3), np.float32), np.zeros(H * W, bool)
    for y in range(H):
        for x in range(W):
            n = fn(P(fs.shapes), len(fs.shapes), P(fs.nodes), len(fs.nodes), P(fs.indices), len(fs.indices),
                   P(cam), P(light), C.byref(p), x, y, P(o), P(d), P(lim), P(kind), 2)
            if n == 2:
                assert kind[1] == 1
                out[y * W + x] = o[1]
                have[y * W + x] = True
    return out, have
