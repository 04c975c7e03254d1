"""Ambient occlusion (rt_dispatch_ao) against the route a host composes without it.

    python tools/bench_ao.py [--workloads 3:1920x1080,5:1920x1080,2:800x600] [--rays 4,16,64]
                             [--radii 2.0,inf] [--rounds 5] [--reps 3] [--out FILE]

For each workload (config:WxH) one process, the context's stream set to a torch stream, HIP
events around whole routes, a warm-up of every shape, then interleaved rounds. Per ray count K
and radius:
  pack      rt_dispatch_ao, count plane, the repacked form (rt_debug_ao form 1)
  lane      the same, each hit lane walking its own K rays (form 2)
  composed  the route without this call, all on the device and on the same stream:
            rt_dispatch_gbuffer (normal + position), a torch op that builds the K rays of every
            pixel as rt_ray records (include/rt_api.h's steps 1-5; a miss pixel sends its
            camera ray, which hits nothing), rt_trace_rays RT_TRACE_ANY, and a sum per pixel
  trace     the rt_trace_rays call of `composed` alone, over the rays already built: the cost
            of incoherent hemisphere rays per ray, beside the camera rays of tools/bench_trace.py
and once per workload (K = 16, radius 2.0) default (rt_debug_ao(0, 0): the form that ships),
pack_w2 / pack_w4 (two and four tiles to a block) and g (rt_dispatch_gbuffer normal + position
alone, for scale).
Checks at the timed size that `lane`, pack_w2 and pack_w4 write `pack`'s bytes (fails otherwise)
and reports whether the composed sums equal the count plane. Appends one JSON line per workload
to --out (default profiles/ao_bench.jsonl): median, minimum and per-round medians in ms of every
shape, each shape's spread (the range of its per-round medians), whether pack and lane beat
composed by more than the two spreads, which form is faster per K and radius, and rays per second
(hit pixels x K / time; for trace all pixels x K, the miss pixels' rays included).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", default="3:1920x1080,5:1920x1080,2:800x600")
ap.add_argument("--rays", default="4,16,64")
ap.add_argument("--radii", default="2.0,inf")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3, help="timed routes per round")
ap.add_argument("--bias", type=float, default=1e-3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ao_bench.jsonl"))
a = ap.parse_args()
KS = [int(v) for v in a.rays.split(",")]
RADII = [float(v) for v in a.radii.split(",")]


def camera_rays(cam, W, H):
    """getRay (gpu_shader.comp:155-168) for every pixel, float32, row order."""
    f = np.float32
    cam = np.asarray(cam).reshape(-1)[0]
    pos, front, right, up = (cam[k].astype(np.float32) for k in ("Position", "Front", "Right", "Up"))
    ph = f(2.0) * np.tan(f(cam["fov"]) / f(2.0) * f(0.017453292519943295)).astype(np.float32)
    pw = ph * f(cam["aspectRatio"])
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    nx = (f(2.0) * x / f(W) - f(1.0)).reshape(-1, 1)
    ny = (f(1.0) - f(2.0) * y / f(H)).reshape(-1, 1)
    p = ((pos + front) + (nx * pw / f(2.0)) * right) + (ny * ph / f(2.0)) * up
    d = p - pos
    d = d * (f(1.0) / np.sqrt((d * d).sum(1, keepdims=True), dtype=np.float32))
    return np.broadcast_to(pos, d.shape).astype(np.float32), d.astype(np.float32)


def build_rays(pos4, nrm4, cam_o, cam_d, rot, D, K, bias, radius, out):
    """The host's device op: rt_ray records [n, K, 8] float32 from the geometry buffer's planes,
    include/rt_api.h's steps 1-5 in float32 (one torch op per operation: nothing contracted)."""
    hit = pos4[:, 3] > 0
    n, p = nrm4[:, :3], pos4[:, :3]
    s = (n[:, 0] * cam_d[:, 0] + n[:, 1] * cam_d[:, 1]) + n[:, 2] * cam_d[:, 2]
    nf = torch.where((s > 0)[:, None], -n, n)
    x, y, z = nf[:, 0], nf[:, 1], nf[:, 2]
    sg = torch.copysign(torch.ones_like(z), z)
    av = torch.full_like(z, -1.0) / (sg + z)
    b = (x * y) * av
    t = torch.stack([1.0 + sg * ((x * x) * av), sg * b, -(sg * x)], 1)
    u = torch.stack([b, sg + (y * y) * av, -y], 1)
    o = torch.where(hit[:, None], p + nf * bias, cam_o)
    c, sn = rot[:, 0:1], rot[:, 1:2]
    dx, dy, dz = D[None, :K, 0], D[None, :K, 1], D[None, :K, 2]
    lx = c * dx - sn * dy
    ly = sn * dx + c * dy
    out[:, :, 0:3] = o[:, None, :]
    out[:, :, 3] = radius
    for i in range(3):
        di = (t[:, i:i + 1] * lx + u[:, i:i + 1] * ly) + nf[:, i:i + 1] * dz
        out[:, :, 4 + i] = torch.where(hit[:, None], di, cam_d[:, i:i + 1])
    out[:, :, 7] = 0.0


stream = torch.cuda.Stream()
D_np, ROT_np = rtamd.ao_table()
for wl in a.workloads.split(","):
    config, size = wl.split(":")
    config, (W, H) = int(config), (int(v) for v in size.split("x"))
    fs = rtamd.generate(config, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, 3, True)
    ctx.set_stream(stream.cuda_stream)
    n = W * H
    o_np, d_np = camera_rays(fs.camera, W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rot_np = ROT_np[((xs & 3) + 4 * (ys & 3)).reshape(-1)]
    with torch.cuda.stream(stream):
        cam_o, cam_d = torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()
        rot, D = torch.from_numpy(np.ascontiguousarray(rot_np)).cuda(), torch.from_numpy(D_np).cuda()
        nrm4 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        pos4 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        kmax = max(KS)
        rays_buf = torch.zeros(n * kmax * 8, dtype=torch.float32, device="cuda")
        hits_buf = torch.zeros(n * kmax * 4, dtype=torch.int32, device="cuda")
        counts = {k: torch.zeros(n, dtype=torch.uint8, device="cuda")
                  for k in ("pack", "lane", "default", "pack_w2", "pack_w4")}
        sums = torch.zeros(n, dtype=torch.int64, device="cuda")
    stream.synchronize()
    torch.cuda.synchronize()

    def gbuffer():
        ctx.gbuffer_device(W, H, 0, 1, 1, H, normal=(nrm4.data_ptr(), 16 * W), position=(pos4.data_ptr(), 16 * W))

    def ao(kind, K, radius):
        form, waves = {"pack": (1, 0), "lane": (2, 0), "default": (0, 0), "pack_w2": (1, 2), "pack_w4": (1, 4)}[kind]
        ctx.debug_ao(form, waves)
        ctx.ao_device(W, H, 0, 1, 1, H, K, radius, a.bias, count=(counts[kind].data_ptr(), W))
        ctx.debug_ao(0, 0)

    def trace(K):
        ctx.trace_rays_device(rays_buf.data_ptr(), n * K, hits_buf.data_ptr(), rtamd.TRACE_ANY)

    def composed(K, radius):
        gbuffer()
        with torch.cuda.stream(stream):
            build_rays(pos4, nrm4, cam_o, cam_d, rot, D, K, a.bias, radius, rays_buf[:n * K * 8].view(n, K, 8))
        trace(K)
        with torch.cuda.stream(stream):
            torch.sum(hits_buf[:n * K * 4].view(n, K, 4)[:, :, 2], dim=1, out=sums)

    def launch(kind, K, radius):
        if kind == "g":
            gbuffer()
        elif kind == "composed":
            composed(K, radius)
        elif kind == "trace":
            trace(K)
        else:
            ao(kind, K, radius)

    shapes = [(kind, K, r) for K in KS for r in RADII for kind in ("pack", "lane", "composed", "trace")]
    shapes += [(kind, 16, 2.0) for kind in ("default", "pack_w2", "pack_w4", "g")]
    name = lambda s: s[0] if s[0] in ("default", "pack_w2", "pack_w4", "g") else f"{s[0]}_k{s[1]}_r{s[2]:g}"  # noqa: E731
    rounds = {name(s): [] for s in shapes}
    checks = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every shape up and carries the identity checks
        for s in shapes:
            ms = []
            for _ in range(1 if rnd == 0 else a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(*s)
                e1.record(stream)
                stream.synchronize()
                ms.append(e0.elapsed_time(e1))
            if rnd > 0:
                rounds[name(s)].append(ms)
                continue
            kind, K, r = s
            if kind == "lane":
                checks[f"lane_equals_pack_k{K}_r{r:g}"] = bool(torch.equal(counts["lane"], counts["pack"]))
            elif kind == "composed":
                checks[f"composed_equals_pack_k{K}_r{r:g}"] = bool(torch.equal(sums, counts["pack"].to(torch.int64)))
                checks[f"occluded_rays_k{K}_r{r:g}"] = int(counts["pack"].sum(dtype=torch.int64).item())
            elif kind in ("default", "pack_w2", "pack_w4"):
                ao("pack", K, r)
                stream.synchronize()
                checks[f"{kind}_equals_pack"] = bool(torch.equal(counts[kind], counts["pack"]))

    hit_px = int((pos4[:, 3] > 0).sum().item())
    med = {k: float(np.median(np.concatenate(v))) for k, v in rounds.items()}
    per_round = {k: [float(np.median(r)) for r in v] for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in per_round.items()}
    verdict, rays_per_s, faster = {}, {}, {}
    for K in KS:
        for r in RADII:
            tag = f"k{K}_r{r:g}"
            for form in ("pack", "lane"):
                gain = med[f"composed_{tag}"] - med[f"{form}_{tag}"]
                verdict[f"{form}_beats_composed_{tag}"] = bool(gain > spread[f"composed_{tag}"] + spread[f"{form}_{tag}"])
                rays_per_s[f"{form}_{tag}"] = hit_px * K / (med[f"{form}_{tag}"] * 1e-3)
            rays_per_s[f"trace_{tag}"] = n * K / (med[f"trace_{tag}"] * 1e-3)
            faster[tag] = "pack" if med[f"pack_{tag}"] < med[f"lane_{tag}"] else "lane"
    line = {"config": config, "width": W, "height": H, "pixels": n, "hit_pixels": hit_px, "rounds": a.rounds,
            "reps": a.reps, "bias": a.bias, "median_ms": med,
            "min_ms": {k: float(np.min(np.concatenate(v))) for k, v in rounds.items()},
            "round_medians_ms": per_round, "spread_ms": spread, "verdict": verdict, "faster_form": faster, "rays_per_s": rays_per_s,
            "checks": checks}
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    ctx.close()
    del rays_buf, hits_buf
    bad = [k for k, v in checks.items() if v is False and not k.startswith("composed_")]
    assert not bad, f"config {config}: forms differ: {bad}"
