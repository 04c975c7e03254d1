"""Ray sets and oracle bindings shared by tests/test_trace_cpu.py and tests/test_gpu_trace.py.

The GPU tests send exactly these rays through rt_trace_rays; the CPU test first shows, with
the scalar emulation of the accelerated walk (tests/native/accel_check.cpp), that for every
one of them the accelerated walk and the reference walk agree, with no ray left out.
"""
import ctypes as C
import functools

import numpy as np

import oracle
import rtamd
import test_accel_cpu as ta

CAM_W, CAM_H = 96, 54
N_RANDOM, N_AXIS, N_FAR, N_SCALED, N_GRAZING = 4000, 2000, 1000, 1000, 2000
SCENES = ("cfg2", "cfg3", "cfg5", "soup1")


@functools.lru_cache(maxsize=None)
def scene(name):
    """cfg2 / cfg3 / cfg5: the generator's scenes at 96x54; soup1: the adversarial soup;
    degenerate/<family>/<seed>/<depth>: a scene of tests/degenerate_scenes.py."""
    if name.startswith("degenerate/"):
        import degenerate_scenes as dg
        fs = dg.scene_of_key(name)
    elif name.startswith("soup"):
        import test_gpu_parity as tg
        fs = tg._soup(int(name[4:]))
    else:
        fs = rtamd.generate(int(name[3:]), 0, CAM_W, CAM_H)
    return rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, fs.camera, fs.light)  # enforce record layout


def camera_ndc(x, y, W, H):
    """The shader's pixel NDC (gpu_shader.comp main: 2x/resX - 1, 1 - 2y/resY) in float32."""
    f = np.float32
    return f(2.0) * f(x) / f(W) - f(1.0), f(1.0) - f(2.0) * f(y) / f(H)


def pixel_rays(fs, W, H, xy):
    """The reference's camera ray of each pixel (x, y) of a W x H frame."""
    o, d = [], []
    for x, y in xy:
        ro, rd = oracle.get_ray(fs.camera, *camera_ndc(x, y, W, H))
        o.append(ro)
        d.append(rd)
    return np.array(o, np.float32), np.array(d, np.float32)


@functools.lru_cache(maxsize=None)
def ray_sets(name):
    """{set name: (origins, dirs)} as float32 arrays, in a fixed order."""
    fs = scene(name)
    rng = np.random.default_rng(100 + SCENES.index(name))
    sets = {}
    sets["camera"] = pixel_rays(fs, CAM_W, CAM_H, [(x, y) for y in range(CAM_H) for x in range(CAM_W)])
    sets["random"] = ta.random_rays(rng, N_RANDOM)
    # axis-aligned directions, and the same with tiny components in place of the zeros
    R = N_AXIS // 2
    o = rng.uniform(-20, 20, (R, 3))
    d = np.zeros((R, 3))
    d[np.arange(R), rng.integers(0, 3, R)] = rng.choice([-1.0, 1.0], R)
    tiny = rng.choice([0.0, 1e-30, -1e-25, 1e-20, -1e-19, 1e-12, 3e-8], (R, 3))
    sets["axis"] = (np.concatenate([o, o]), np.concatenate([d, np.where(d == 0, tiny, d)]))
    # far origins aimed back at the scene (the always-enter mode of accel_math.h ray_consts)
    t = rng.uniform(-5, 5, (N_FAR, 3))
    far = rng.normal(size=(N_FAR, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.choice([1e4, 1e6, 1e8], (N_FAR, 1))
    sets["far"] = (far, (t - far) / np.linalg.norm(t - far, axis=1, keepdims=True))
    # non-unit directions: below 0.5 and above 2 (always-enter too)
    o, d = ta.random_rays(rng, N_SCALED)
    sets["scaled"] = (o, d * rng.choice([0.3, 3.0], (N_SCALED, 1)))
    if (fs.shapes["type"] == 3).any():
        sets["grazing"] = ta.grazing_rays(fs, rng, N_GRAZING)
    return {k: (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)) for k, (o, d) in sets.items()}


@functools.lru_cache(maxsize=None)
def all_rays(name):
    """Every set of the scene as one (origins, dirs, limits): limits uniform in [1, 80)."""
    sets = ray_sets(name)
    o = np.concatenate([v[0] for v in sets.values()])
    d = np.concatenate([v[1] for v in sets.values()])
    lim = np.random.default_rng(7).uniform(1, 80, len(o)).astype(np.float32)
    return o, d, lim


def _p(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def oracle_trace(fs, o, d, lim, mt):
    """orc_trace_rays_mt: (shape, distance, shadow) of the reference walk for each ray."""
    lib = oracle.lib()
    lib.orc_trace_rays_mt.restype = C.c_int
    lib.orc_trace_rays_mt.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + \
        [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int]
    fs = rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, fs.camera, fs.light)
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    lim = np.ascontiguousarray(lim, np.float32)
    R = len(o)
    shape, dist, shadow = np.zeros(R, np.int32), np.zeros(R, np.float32), np.zeros(R, np.int32)
    rc = lib.orc_trace_rays_mt(_p(fs.shapes), len(fs.shapes), _p(fs.nodes), len(fs.nodes), _p(fs.indices),
                               len(fs.indices), _p(o), _p(d), _p(lim), R, _p(shape), _p(dist), _p(shadow), int(mt))
    assert rc == 0
    return shape, dist, shadow


@functools.lru_cache(maxsize=None)
def oracle_all(name, mt):
    """The oracle's answers for all_rays(name); computed once per (scene, mt), never modified."""
    out = oracle_trace(scene(name), *all_rays(name), mt)
    for a in out:
        a.setflags(write=False)
    return out
