"""Ray queries (rt_trace_rays): the accelerated walk against the literal reference walk.

    python tools/bench_trace.py [--configs 3,5] [--rounds 3] [--reps 10] [--literal-reps 3] [--out FILE]

For each config at 1920x1080 and three ray sets of W*H rays each
  rows   : the frame's camera rays in row order (64 consecutive pixels of a row to a wave)
  tiles  : the same rays in 8x8-tile order (one tile to a wave, as the render kernels)
  random : origins uniform in the scene's root box grown by half, aimed at uniform points in it
times the query kernel alone (HIP events on the context's stream around one rt_trace_rays
launch on device buffers) for RT_TRACE_CLOSEST and RT_TRACE_ANY, with the accelerated walk
(k_trace, RT_KERNEL_AUTO) and with the literal walk (k_trace_ref, RT_KERNEL_LANE), in
interleaved rounds in one process after a warm-up launch of each. Limits are infinite: ANY
asks whether anything lies along the ray. Checks that both walks return identical hit
buffers, and appends one JSON line per (config, set, mode) to --out (default
profiles/trace_bench.jsonl): median and minimum ms of each walk, Mrays/s, their ratio.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-ray-tracer_amd"))
import rtamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,5")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=10, help="timed launches of the accelerated walk per round")
ap.add_argument("--literal-reps", type=int, default=3, help="timed launches of the literal walk per round")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.jsonl"))
a = ap.parse_args()
W, H = a.width, a.height


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


def tile_order(W, H):
    """Row-order pixel indices listed 8x8 tile by tile (row-major tiles, row-major inside)."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    key = ((ys // 8) * ((W + 7) // 8) + xs // 8) * 64 + (ys % 8) * 8 + xs % 8
    return np.argsort(key.reshape(-1), kind="stable")


def random_rays(fs, n, rng):
    lo = fs.nodes["boundsMin"][-1].astype(np.float64)
    hi = fs.nodes["boundsMax"][-1].astype(np.float64)
    lo, hi = np.maximum(lo, -1e3), np.minimum(hi, 1e3)  # a plane's box is unbounded
    c, e = (lo + hi) / 2, (hi - lo) / 2
    o = rng.uniform(c - 1.5 * e, c + 1.5 * e, (n, 3))
    t = rng.uniform(lo, hi, (n, 3))
    d = t - o
    return o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


stream = torch.cuda.Stream()
lines = []
for config in [int(c) for c in a.configs.split(",")]:
    fs = rtamd.generate(config, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, 3, True)
    ctx.set_stream(stream.cuda_stream)
    o, d = camera_rays(fs.camera, W, H)
    order = tile_order(W, H)
    sets = {"rows": (o, d), "tiles": (o[order], d[order]), "random": random_rays(fs, W * H, np.random.default_rng(1))}
    for name, (ro, rd) in sets.items():
        rays = rtamd.ComputeShader.make_rays(ro, rd)
        n = len(rays)
        dev = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
        hits = {k: torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for k in ("accel", "literal")}
        torch.cuda.synchronize()
        for mode, mname in ((rtamd.TRACE_CLOSEST, "closest"), (rtamd.TRACE_ANY, "any")):
            ms = {"accel": [], "literal": []}
            for rnd in range(a.rounds + 1):  # round 0 warms both up
                for walk, kernel, reps in (("accel", rtamd.KERNEL_AUTO, a.reps), ("literal", rtamd.KERNEL_LANE, a.literal_reps)):
                    ctx.set_kernel(kernel)
                    for _ in range(1 if rnd == 0 else reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        ctx.trace_rays_device(dev.data_ptr(), n, hits[walk].data_ptr(), mode)
                        e1.record(stream)
                        stream.synchronize()
                        if rnd > 0:
                            ms[walk].append(e0.elapsed_time(e1))
            same = bool(torch.equal(hits["accel"], hits["literal"]))
            h = hits["accel"].cpu().numpy().view(rtamd.HIT_DTYPE)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            line = {"config": config, "width": W, "height": H, "rays": n, "set": name, "mode": mname,
                    "rounds": a.rounds, "reps": {"accel": a.reps, "literal": a.literal_reps},
                    "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
                    "mrays_per_s": {k: n / v / 1e3 for k, v in med.items()},
                    "literal_over_accel": med["literal"] / med["accel"],
                    "hit_fraction": float((h["occluded"] != 0).mean()),
                    "accel_equals_literal": same}
            print(json.dumps(line), flush=True)
            lines.append(line)
            assert same, f"config {config} {name} {mname}: the two walks' hit buffers differ"
    ctx.set_kernel(rtamd.KERNEL_AUTO)
    ctx.close()
with open(a.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
