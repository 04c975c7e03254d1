"""The reference of rt_set_lights for tests/test_lights_cpu.py and tests/test_gpu_lights.py:
tests/shade_ref.py's bounce loop with the light loop of include/rt_api.h's definition, float32
in the shader's order.

Per bounce that hit something, for light i = 0 .. L-1 in order: the shadow ray from the one
origin hit + normal * 1e-3 towards pos_i, blocked by an INNER hit nearer than
min(dist(pos_i, hit), 1e20) (trace_rays.oracle_trace, the reference walk); term_i =
shade_ref.phong with light i, times 0.3 where blocked. pc = term_0, then pc = pc + term_i left
to right; the rest of the bounce is shade_ref's. tests/test_lights_cpu.py anchors it: one light
is shade_ref.shade bit for bit (and through it the oracle's frame), and a second light of
colour zero changes no value.

The fixed test lights (fixed_lights): L0 the scene's own light at half its colour, L1 off the
camera (Position + 3 Right + 4 Up), L2 the scene light mirrored in x and z, L3..L7 the scene
light's position moved by fixed vectors, every colour distinct.
"""
import numpy as np

import gbuffer_ref as gr
import oracle
import rtamd
import trace_rays as tr
from shade_ref import background, dot, gmax, gmin, normalize, phong, reflect

F = np.float32
MAX_LIGHTS = 8
# L3..L7: offsets from the scene light's position, and the colours
OFFSETS = ((6.0, 0.0, 0.0), (-6.0, 1.0, 0.0), (0.0, 2.0, 6.0), (0.0, -1.0, -6.0), (4.0, 5.0, 4.0))
COLOURS = ((3.0, 0.5, 0.5), (0.5, 3.0, 0.5), (0.5, 0.5, 3.0), (2.0, 2.0, 0.25), (0.25, 2.0, 2.0))


def fixed_lights(fs, count):
    """The first `count` of the eight fixed test lights of scene fs, as LIGHT_DTYPE records."""
    assert 1 <= count <= MAX_LIGHTS
    own = rtamd.as_records(fs.light, rtamd.LIGHT_DTYPE).reshape(-1)[0]
    cam = rtamd.as_records(fs.camera, rtamd.CAMERA_DTYPE).reshape(-1)[0]
    pos, col = own["position"].astype(F), own["color"].astype(F)
    out = np.zeros(MAX_LIGHTS, rtamd.LIGHT_DTYPE)
    out["position"][0], out["color"][0] = pos, col * F(0.5)
    out["position"][1] = cam["Position"].astype(F) + F(3.0) * cam["Right"].astype(F) + F(4.0) * cam["Up"].astype(F)
    out["color"][1] = (4.0, 2.0, 1.0)
    out["position"][2], out["color"][2] = pos * np.array([-1.0, 1.0, -1.0], F), (1.0, 2.0, 4.0)
    for k, (off, c) in enumerate(zip(OFFSETS, COLOURS)):
        out["position"][3 + k], out["color"][3 + k] = pos + np.array(off, F), c
    return out[:count].copy()


def shade(fs, o, d, sky, lights, bounces=3, fresnel=False, mt=False, info=None):
    """[n, 4] float32: the pixel of every ray under `lights` (LIGHT_DTYPE records), alpha 1. BVH
    branch only. info: a dict that receives "shadow0", [n, L] int8 -- each light's shadow answer
    at the camera ray's hit, -1 for rays that hit nothing."""
    fs = rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, fs.camera, fs.light)
    lights = rtamd.as_records(lights, rtamd.LIGHT_DTYPE).reshape(-1)
    L = len(lights)
    assert 1 <= L <= MAX_LIGHTS
    o = np.array(o, F).reshape(-1, 3)
    d = np.array(d, F).reshape(-1, 3)
    n = len(o)
    bg = background(sky)
    acc, att = np.zeros((n, 3), F), np.ones((n, 3), F)
    alive = np.ones(n, bool)
    inf = F(np.inf)
    if info is not None:
        info["shadow0"] = np.full((n, L), -1, np.int8)
    with np.errstate(all="ignore"):
        for bounce in range(bounces):
            idx = np.where(alive)[0]
            if idx.size == 0:
                break
            shape, _, _ = tr.oracle_trace(fs, o[idx], d[idx], np.full(idx.size, inf, F), mt)
            miss = shape < 0
            acc[idx[miss]] = acc[idx[miss]] + att[idx[miss]] * bg[idx[miss]]
            alive[idx[miss]] = False
            idx, shape = idx[~miss], shape[~miss]
            if idx.size == 0:
                break
            hp = np.zeros((idx.size, 4), F)
            for j, i in enumerate(idx):
                kind, p = oracle.intersect(fs.shapes[shape[j]:shape[j] + 1], o[i], d[i], mt)
                assert kind == 1  # INNER: the shape the walk chose is hit by this test
                hp[j, :3] = p
            hn = gr.restated_normals(fs.shapes, shape, hp)[:, :3]
            hp = hp[:, :3]
            m = fs.shapes[shape]["material"]
            hc = m["color"].astype(F)
            so = hp + hn * F(1e-3)  # one shadow origin for every light
            pc = None
            for k in range(L):
                lpos, lcol = lights["position"][k].astype(F)[None, :], lights["color"][k].astype(F)
                sd = normalize(lpos - hp)
                ld = np.sqrt(dot(hp - lpos, hp - lpos))
                _, _, shadow = tr.oracle_trace(fs, so, sd, gmin(ld, F(1e20)), mt)
                if info is not None and bounce == 0:
                    info["shadow0"][idx, k] = shadow != 0
                term = phong(hp, hn, d[idx], lpos, lcol, m)
                term = np.where((shadow != 0)[:, None], term * F(0.3), term).astype(F)
                pc = term if k == 0 else (pc + term).astype(F)
            acc[idx] = acc[idx] + att[idx] * pc
            mirror = m["specularStrength"] > 0
            rd = reflect(d[idx], hn)
            o[idx[mirror]] = so[mirror]
            d[idx[mirror]] = rd[mirror]
            if fresnel:
                fr = np.power(F(1.0) - gmax(dot(-rd, hn), F(0.0)), F(5.0), dtype=F)
                fr = gmin(gmax(fr, F(0.0)), F(0.8))
                rw = m["fresnelStrength"] * fr
                mw = F(1.0) - rw
                mixed = hc + rw[:, None] * (F(1.0) - hc)
                k = idx[mirror]
                att[k] = att[k] * mixed[mirror]
                acc[k] = acc[k] + (mw[:, None] * hc)[mirror] * pc[mirror]
            else:
                att[idx[mirror]] = att[idx[mirror]] * m["specularStrength"][mirror][:, None]
            alive[idx[~mirror]] = False
    out = np.ones((n, 4), F)
    out[:, :3] = acc
    return out
