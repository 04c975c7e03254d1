"""Geometry buffers (rt_dispatch_gbuffer) against the ray-query route to the same data.

    python tools/bench_gbuffer.py [--workloads 3:1920x1080,5:1920x1080,2:800x600] [--rounds 5]
                                  [--reps 10] [--literal-reps 2] [--out FILE]

For each workload (config:WxH) one process, the context's stream set to a torch stream, HIP
events around single launches, a warm-up launch of every shape, then interleaved rounds:
  a        rt_dispatch_gbuffer, planes shape + depth (the packet kernel, default block shape)
  b        rt_dispatch_gbuffer, all four planes
  c        the route without this call: rt_trace_rays RT_TRACE_CLOSEST over the frame's camera
           rays in 8x8-tile order on device buffers (tools/bench_trace.py's "tiles" set)
  d        one ordinary one-sample rt_dispatch of the same frame, for scale
  e        (a) with rt_set_kernel(RT_KERNEL_LANE): the literal walk
  a_lane   (a) walked per lane over the accelerator (rt_debug_gbuffer): packet against lane
  a_w2, a_w4   (a) with two and four tiles (waves) to a block instead of one
Checks at the timed size that plane `shape` equals (c)'s rt_hit::shape and plane `depth` equals
(c)'s rt_hit::distance bit for bit, and that (e), a_lane, a_w2 and a_w4 write (a)'s bytes; fails
otherwise. Appends one JSON line per workload to --out (default profiles/gbuffer_bench.jsonl):
median, minimum and per-round medians in ms of every shape, the spread of (c) (the range of its
per-round medians), whether (a) is within it, and the achieved GB/s of (b) from 40 B per pixel
plus rt_accel_info::record_bytes.
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
ap.add_argument("--workloads", default="3:1920x1080,5:1920x1080,2:800x600")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10, help="timed launches per round")
ap.add_argument("--literal-reps", type=int, default=2, help="timed launches of the literal walk per round")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbuffer_bench.jsonl"))
a = ap.parse_args()


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


stream = torch.cuda.Stream()
for wl in a.workloads.split(","):
    config, size = wl.split(":")
    config, (W, H) = int(config), (int(v) for v in size.split("x"))
    fs = rtamd.generate(config, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, 3, True)
    ctx.set_stream(stream.cuda_stream)
    o, d = camera_rays(fs.camera, W, H)
    order = tile_order(W, H)
    rays = rtamd.ComputeShader.make_rays(o[order], d[order])
    n = W * H
    dev_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    px = {"shape": 4, "depth": 4, "normal": 16, "position": 16}
    small, full = ("shape", "depth"), ("shape", "depth", "normal", "position")
    gshapes = {"a": (small, rtamd.KERNEL_AUTO, 0, 0), "b": (full, rtamd.KERNEL_AUTO, 0, 0),
               "e": (small, rtamd.KERNEL_LANE, 0, 0), "a_lane": (small, rtamd.KERNEL_AUTO, 1, 0),
               "a_w2": (small, rtamd.KERNEL_AUTO, 0, 2), "a_w4": (small, rtamd.KERNEL_AUTO, 0, 4)}
    planes = {k: {p: torch.zeros(n * px[p], dtype=torch.uint8, device="cuda") for p in g[0]}
              for k, g in gshapes.items()}
    torch.cuda.synchronize()

    def launch(kind):
        if kind == "c":
            ctx.trace_rays_device(dev_rays.data_ptr(), n, hits.data_ptr(), rtamd.TRACE_CLOSEST)
        elif kind == "d":
            ctx.dispatch(W, H)
        else:
            names, kernel, walk, waves = gshapes[kind]
            ctx.set_kernel(kernel)
            ctx.debug_gbuffer(walk, waves)
            ctx.gbuffer_device(W, H, 0, 1, 1, H, **{p: (planes[kind][p].data_ptr(), W * px[p]) for p in names})
            ctx.debug_gbuffer(0, 0)
            ctx.set_kernel(rtamd.KERNEL_AUTO)

    kinds = ["a", "b", "c", "d", "e", "a_lane", "a_w2", "a_w4"]
    rounds = {k: [] for k in kinds}
    for rnd in range(a.rounds + 1):  # round 0 warms every shape up
        for kind in kinds:
            reps = 1 if rnd == 0 else (a.literal_reps if kind == "e" else a.reps)
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(kind)
                e1.record(stream)
                stream.synchronize()
                ms.append(e0.elapsed_time(e1))
            if rnd > 0:
                rounds[kind].append(ms)

    # identity at the timed size: the planes against the query route, and every variant against (a)
    h = hits.cpu().numpy().view(rtamd.HIT_DTYPE)
    shape = planes["a"]["shape"].cpu().numpy().view(np.int32)
    depth = planes["a"]["depth"].cpu().numpy().view(np.uint32)
    same_shape = bool(np.array_equal(shape[order], h["shape"]))
    same_depth = bool(np.array_equal(depth[order], h["distance"].view(np.uint32)))
    variants = {k: all(bool(torch.equal(planes[k][p], planes["a"][p])) for p in small)
                for k in ("b", "e", "a_lane", "a_w2", "a_w4")}
    info = ctx.accel_info()
    med = {k: float(np.median(np.concatenate(v))) for k, v in rounds.items()}
    per_round = {k: [float(np.median(r)) for r in v] for k, v in rounds.items()}
    spread_c = max(per_round["c"]) - min(per_round["c"])
    line = {"config": config, "width": W, "height": H, "pixels": n, "rounds": a.rounds,
            "reps": {"default": a.reps, "e": a.literal_reps},
            "median_ms": med, "min_ms": {k: float(np.min(np.concatenate(v))) for k, v in rounds.items()},
            "round_medians_ms": per_round, "spread_c_ms": spread_c,
            "a_minus_c_ms": med["a"] - med["c"], "a_within_spread_of_c": bool(med["a"] - med["c"] <= spread_c),
            "record_bytes": info["record_bytes"],
            "b_gb_per_s": (40.0 * n + info["record_bytes"]) / (med["b"] * 1e-3) / 1e9,
            "hit_fraction": float((shape >= 0).mean()),
            "shape_equals_trace": same_shape, "depth_equals_trace": same_depth, "variants_equal_a": variants}
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    ctx.close()
    assert same_shape and same_depth, f"config {config}: planes differ from rt_trace_rays' hits"
    assert all(variants.values()), f"config {config}: kernel variants differ: {variants}"
