"""The reference of rt_shade_rays for tests/test_shade_cpu.py and tests/test_gpu_shade.py: the
bounce loop of the shader's main() (oracle/rt_oracle.c shade_pixel, BVH branch) restated in
numpy, float32 in the shader's order, for rays the caller gives.

Per bounce: the closest hit of every live ray from trace_rays.oracle_trace (the reference
walk), the hit point from oracle.intersect of the winning shape, the normal from
gbuffer_ref.restated_normals, the shadow answer from oracle_trace with the limit
min(dist(light, hit), 1e20); then phong_gpu, shadow x0.3, reflect, Fresnel and the background
mix, each operation one float32 operation in the order rt_oracle.c writes it (glm: dot =
(x*x + y*y) + z*z, normalize = v * (1 / sqrt(v.v)), reflect = I - (N * dot(N, I)) * 2,
mix = x + a * (y - x)). tests/test_shade_cpu.py shows it is the oracle's frame for a frame's
own camera rays.
"""
import numpy as np

import gbuffer_ref as gr
import oracle
import rtamd
import trace_rays as tr

F = np.float32
BG_LO = np.array([0.05, 0.07, 0.1], F)
BG_HI = np.array([0.5, 0.7, 1.0], F)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize(a):
    return a * (F(1.0) / np.sqrt(dot(a, a)))[:, None]


def reflect(i, n):
    return i - (n * dot(n, i)[:, None]) * F(2.0)


def gmax(a, b):
    """GLSL / glm max: (a < b) ? b : a."""
    return np.where(a < b, b, a).astype(F)


def gmin(a, b):
    """GLSL / glm min: (b < a) ? b : a."""
    return np.where(b < a, b, a).astype(F)


def background(sky):
    """mix((0.05, 0.07, 0.1), (0.5, 0.7, 1.0), sky) per ray."""
    sky = np.asarray(sky, F).reshape(-1)
    return BG_LO[None, :] + sky[:, None] * (BG_HI - BG_LO)[None, :]


def frame_sky(W, H, y0=0, rows=None):
    """The background parameter a frame uses: f32(y) / f32(H) for every pixel, row-major."""
    rows = H - y0 if rows is None else rows
    y = np.repeat(np.arange(y0, y0 + rows), W).astype(F)
    return y / F(H)


def phong(p, n, view, lpos, lcol, m):
    """phong_gpu for hit points p, normals n, view vectors (the rays' directions)."""
    dl = np.sqrt(dot(p - lpos, p - lpos))
    lc = lcol[None, :] / dl[:, None]
    amb = m["ambientStrength"][:, None] * lc
    ldir = normalize(lpos - p)
    diff = gmax(dot(n, ldir), F(0.0))
    dif = (m["diffuseStrength"] * diff)[:, None] * lc
    rd = reflect(-ldir, n)
    sp = np.power(gmax(dot(view, rd), F(0.0)), m["shininess"].astype(F), dtype=F)
    spc = np.where((diff > 0)[:, None], (m["specularStrength"] * sp)[:, None] * lc, F(0.0)).astype(F)
    return ((amb + dif) + spc) * m["color"]


def shade(fs, o, d, sky, bounces=3, fresnel=False, mt=False):
    """[n, 4] float32: the pixel of every ray (origin o, direction d as given, background
    parameter sky), alpha 1. BVH branch only."""
    fs = rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, fs.camera, fs.light)
    o = np.array(o, F).reshape(-1, 3)
    d = np.array(d, F).reshape(-1, 3)
    n = len(o)
    bg = background(sky)
    light = rtamd.as_records(fs.light, rtamd.LIGHT_DTYPE).reshape(-1)[0]
    lpos, lcol = light["position"].astype(F)[None, :], light["color"].astype(F)
    acc, att = np.zeros((n, 3), F), np.ones((n, 3), F)
    alive = np.ones(n, bool)
    inf = F(np.inf)
    with np.errstate(all="ignore"):
        for _ in range(bounces):
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
            # the shadow ray: origin hit + normal * 1e-3, towards the light, blocked by an INNER
            # hit nearer than the light
            so = hp + hn * F(1e-3)
            sd = normalize(lpos - hp)
            ld = np.sqrt(dot(hp - lpos, hp - lpos))
            _, _, shadow = tr.oracle_trace(fs, so, sd, gmin(ld, F(1e20)), mt)
            pc = phong(hp, hn, d[idx], lpos, lcol, m)
            pc = np.where((shadow != 0)[:, None], pc * F(0.3), pc).astype(F)
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
