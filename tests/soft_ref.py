"""The reference of rt_set_soft_shadows for tests/test_soft_cpu.py and tests/test_gpu_soft.py:
tests/lights_ref.py's bounce loop with the sample loop of include/rt_api.h's definition,
float32 in the order written.

Per bounce that hit something, for light i = 0 .. L-1 in order: a light of radius 0 sends
lights_ref's one shadow ray (K_i = 1); a light of radius R > 0 sends K rays from the one shadow
origin towards the points pos_i + t * (R lx) + u * (R ly) of a disc that faces the hit -- (t, u)
ao_ref.frames' tangent frame about w = normalize(pos_i - hp) (no facing flip), (lx, ly) the x, y
of ao_ref.tables()' D[k] turned by ROT[j], j a hash of the hit point's bits -- each blocked by an
INNER hit nearer than min(dist(s, hp), 1e20) (trace_rays.oracle_trace). b_i counts the blocked
rays; term_i = shade_ref.phong with the light's centre, times 1 - 0.7 * (b_i / K_i) where
b_i > 0. tests/test_soft_cpu.py anchors it to lights_ref.
"""
import numpy as np

import ao_ref
import gbuffer_ref as gr
import oracle
import rtamd
import trace_rays as tr
from lights_ref import MAX_LIGHTS
from shade_ref import background, dot, gmax, gmin, normalize, phong, reflect

F = np.float32
MAX_SHADOW_SAMPLES = 64


def rotation_index(hp):
    """Step 3: j [h] of hit points hp [h, 3] float32."""
    b = np.ascontiguousarray(hp, F).view(np.uint32)
    x = (b[:, 0] ^ b[:, 1] ^ b[:, 2]).astype(np.uint64)
    return (((x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)).astype(np.int64)


def frame(w):
    """Step 2 for unit vectors w [h, 3]: (t, u), ao_ref.frames' arithmetic with nf := w."""
    w = np.ascontiguousarray(w, F)
    # a camera direction of -w never flips w: dot(w, -w) < 0
    nf, t, u = ao_ref.frames(w, -w)
    assert np.array_equal(nf.view(np.uint32), w.view(np.uint32))
    return t, u


def sample_points(hp, lpos, R, K):
    """Steps 1-5: [h, K, 3] float32, the K sample points of a light at lpos [1, 3] with radius R
    for hit points hp [h, 3]."""
    D, ROT = ao_ref.tables()
    R = F(R)
    w = normalize(lpos - hp)
    t, u = frame(w)
    j = rotation_index(hp)
    c, sn = ROT[j, 0][:, None], ROT[j, 1][:, None]
    dx, dy = D[None, :K, 0], D[None, :K, 1]
    lx = c * dx - sn * dy
    ly = sn * dx + c * dy
    rx = R * lx
    ry = R * ly
    s = np.stack([lpos[0, i] + ((t[:, None, i] * rx) + (u[:, None, i] * ry)) for i in range(3)], 2)
    assert s.dtype == F and s.shape == (len(hp), K, 3)
    return s


def shade(fs, o, d, sky, lights, radii=(), samples=1, bounces=3, fresnel=False, mt=False, info=None,
          all_blocked=False):
    """[n, 4] float32: the pixel of every ray under `lights` (LIGHT_DTYPE records) with the radii
    `radii` (lights past the list have radius 0) and K = `samples`, alpha 1. BVH branch only.
    info: a dict that receives "blocked0", [n, L] int16 -- each light's b_i at the camera ray's
    hit, -1 for rays that hit nothing -- and "rays0", [L], each light's K_i.
    all_blocked: every b_i is K_i whatever the walks say (the darkest frame the definition allows)."""
    fs = rtamd.FlatScene(fs.shapes, fs.nodes, fs.indices, fs.camera, fs.light)
    lights = rtamd.as_records(lights, rtamd.LIGHT_DTYPE).reshape(-1)
    L = len(lights)
    assert 1 <= L <= MAX_LIGHTS and len(radii) <= MAX_LIGHTS and 1 <= samples <= MAX_SHADOW_SAMPLES
    rad = np.zeros(MAX_LIGHTS, F)
    rad[:len(radii)] = np.asarray(radii, F)
    assert np.isfinite(rad).all() and (rad >= 0).all()
    o = np.array(o, F).reshape(-1, 3)
    d = np.array(d, F).reshape(-1, 3)
    n = len(o)
    bg = background(sky)
    acc, att = np.zeros((n, 3), F), np.ones((n, 3), F)
    alive = np.ones(n, bool)
    inf = F(np.inf)
    if info is not None:
        info["blocked0"] = np.full((n, L), -1, np.int16)
        info["rays0"] = np.array([samples if rad[k] > 0 else 1 for k in range(L)])
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
            so = hp + hn * F(1e-3)  # one shadow origin for every light and sample
            pc = None
            for k in range(L):
                lpos, lcol = lights["position"][k].astype(F)[None, :], lights["color"][k].astype(F)
                if rad[k] > 0:
                    K = samples
                    s = sample_points(hp, lpos, rad[k], K).reshape(-1, 3)
                    h3 = np.repeat(hp, K, axis=0)
                    ro = np.repeat(so, K, axis=0)
                else:
                    K, s, h3, ro = 1, np.broadcast_to(lpos, hp.shape), hp, so
                sd = normalize(s - h3)
                ld = np.sqrt(dot(h3 - s, h3 - s))
                _, _, shadow = tr.oracle_trace(fs, ro, sd, gmin(ld, F(1e20)), mt)
                b = (shadow != 0).reshape(idx.size, K).sum(axis=1)
                if all_blocked:
                    b[:] = K
                if info is not None and bounce == 0:
                    info["blocked0"][idx, k] = b
                term = phong(hp, hn, d[idx], lpos, lcol, m)
                factor = F(1.0) - F(0.7) * (b.astype(F) / F(K))
                assert factor.dtype == F
                term = np.where((b > 0)[:, None], term * factor[:, None], term).astype(F)
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
