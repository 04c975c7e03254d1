"""The reference ambient occlusion of tests/test_ao_cpu.py and tests/test_gpu_ao.py: the numpy
restatement of include/rt_api.h's "Definition of a pixel" (rt_dispatch_ao), steps 1-6, over the
geometry buffer of tests/gbuffer_ref.py, every operation in float32 in the order written.

The tables are regenerated here in double from their formulas (not read from the header or the
generator); the counts come from trace_rays.oracle_trace, the oracle's own walk, with the ray's
limit as the ANY limit.
"""
import functools
from fractions import Fraction

import numpy as np

import gbuffer_ref as gr
import trace_rays as tr

PLANES = ("count", "visibility")
BIAS = 1e-3
RADII = (2.0, float("inf"))
K0 = 16
W0, H0, W1, H1, WA, HA = gr.W0, gr.H0, gr.W1, gr.H1, gr.WA, gr.HA
f32 = np.float32


def radical_inverse(n, base):
    v, f = Fraction(0), Fraction(1, base)
    while n:
        v += (n % base) * f
        n //= base
        f /= base
    return float(v)


@functools.lru_cache(maxsize=None)
def tables():
    """(D [64, 3], ROT [16, 2]) float32: step 3, evaluated in double."""
    u1 = np.array([radical_inverse(k + 1, 2) for k in range(64)])
    u2 = np.array([radical_inverse(k + 1, 3) for k in range(64)])
    d = np.stack([np.sqrt(u1) * np.cos(2 * np.pi * u2), np.sqrt(u1) * np.sin(2 * np.pi * u2), np.sqrt(1 - u1)], 1)
    a = 2 * np.pi * np.array([(7 * j) % 16 for j in range(16)], np.float64) / 16
    d, rot = d.astype(f32), np.stack([np.cos(a), np.sin(a)], 1).astype(f32)
    d.setflags(write=False)
    rot.setflags(write=False)
    return d, rot


def frames(n, d):
    """Steps 1 and 2 for normals n [h, 3] and camera directions d [h, 3]: (nf, t, u), float32."""
    n, d = np.ascontiguousarray(n, f32), np.ascontiguousarray(d, f32)
    with np.errstate(all="ignore"):
        s = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        nf = np.where((s > 0)[:, None], -n, n)
        x, y, z = nf[:, 0], nf[:, 1], nf[:, 2]
        sg = np.copysign(f32(1), z)
        a = f32(-1.0) / (sg + z)
        b = (x * y) * a
        t = np.stack([f32(1.0) + sg * ((x * x) * a), sg * b, -(sg * x)], 1)
        u = np.stack([b, sg + (y * y) * a, -y], 1)
    assert nf.dtype == t.dtype == u.dtype == f32
    return nf, t, u


def build_rays(p, n, d, x, y, K, bias=BIAS):
    """Steps 1-5 for hit pixels (x, y) with position p, normal n and camera direction d:
    origins [h, 3] and directions [h, K, 3], float32."""
    D, ROT = tables()
    nf, t, u = frames(n, d)
    o = (np.ascontiguousarray(p, f32) + nf * f32(bias)).astype(f32)
    j = (np.asarray(x) & 3) + 4 * (np.asarray(y) & 3)
    c, sn = ROT[j, 0][:, None], ROT[j, 1][:, None]
    dx, dy, dz = D[None, :K, 0], D[None, :K, 1], D[None, :K, 2]
    lx = c * dx - sn * dy
    ly = sn * dx + c * dy
    lz = np.broadcast_to(dz, lx.shape)
    dirs = np.stack([(t[:, None, i] * lx + u[:, None, i] * ly) + nf[:, None, i] * lz for i in range(3)], 2)
    assert o.dtype == dirs.dtype == f32 and dirs.shape == (len(o), K, 3)
    return o, dirs


@functools.lru_cache(maxsize=None)
def ray_set(key, W, H, mt, K=K0, bias=BIAS):
    """(hit pixel indices [h] row-major, origins [h, 3], directions [h, K, 3]) of a whole frame."""
    g = gr.reference(key, W, H, mt)
    _, d = gr.rays(key, W, H)
    idx = np.where(g["shape"].reshape(-1) >= 0)[0]
    o, dirs = build_rays(g["position"].reshape(-1, 4)[idx, :3], g["normal"].reshape(-1, 4)[idx, :3], d[idx],
                         idx % W, idx // W, K, bias)
    for a in (idx, o, dirs):
        a.setflags(write=False)
    return idx, o, dirs


def flat_rays(o, dirs):
    """One (origins, directions) row per ray, pixel-major."""
    K = dirs.shape[1]
    return np.repeat(o, K, axis=0), dirs.reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def occluded(key, W, H, mt, radius, K=K0, bias=BIAS):
    """[h, K] bool: the oracle's RT_TRACE_ANY answer of every ray of ray_set."""
    _, o, dirs = ray_set(key, W, H, mt, K, bias)
    ro, rd = flat_rays(o, dirs)
    _, _, shadow = tr.oracle_trace(gr.scene(key), ro, rd, np.full(len(ro), radius, f32), mt)
    occ = (shadow != 0).reshape(len(o), K)
    occ.setflags(write=False)
    return occ


def reference(key, W, H, mt, K=K0, radius=2.0, bias=BIAS):
    """{"count": [H, W] uint8, "visibility": [H, W] float32} of the whole frame (step 6). Ray
    count K is the sum over the first K rays of the set walked (16, or 64 for K > 16)."""
    kmax = K0 if K <= K0 else 64
    idx, _, _ = ray_set(key, W, H, mt, kmax, bias)
    occ = occluded(key, W, H, mt, radius, kmax, bias)
    count = np.zeros(W * H, np.uint8)
    count[idx] = occ[:, :K].sum(axis=1)
    vis = (K - count.astype(np.int32)).astype(f32) / f32(K)
    assert vis.dtype == f32
    return {"count": count.reshape(H, W), "visibility": vis.reshape(H, W)}


# every (scene key, W, H, triangle tests, ray count) whose rays tests/test_gpu_ao.py walks on the
# device; tests/test_ao_cpu.py sends the same rays through the emulated accelerated walk
def gpu_ray_sets():
    sets = [(name, W0, H0, (0, 1), K0) for name in tr.SCENES]
    sets += [("cfg3", W0, H0, (0,), 64)]
    sets += [("cfg3", W, H, (0,), K0) for W, H in gr.EDGE_SIZES]
    sets += [("cfg3:far", W0, H0, (0, 1), K0), ("cfg3:anim", WA, HA, (0, 1), K0), ("cfg3:ties", W0, H0, (0,), K0)]
    return sets
