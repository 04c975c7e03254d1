"""Shaded rays (rt_shade_rays) against the frame that shades the same rays itself.

    python tools/bench_shade.py [--configs 3,5,2] [--rounds 3] [--reps 10] [--out FILE]

For the car (config 3, 1920x1080, 3 bounces), the 100k-triangle scene (config 5, 1920x1080, 3
bounces) and the monkey scene (config 2, 800x600, 1 bounce), device time per call (HIP events on
the context's stream around one launch on device buffers, interleaved rounds in one process
after warm-up launches of each, median and minimum):
  a_rows / a_tiles : rt_shade_rays over the frame's rt_camera_rays list in raster order and in
                     8x8-tile order (one tile to a wave, as the render kernels)
  a_rows_plain / a_rows_split : the same raster list with k_shade's plain and split-walk
                     instances (rt_debug_shade 1 and 2; barycentric frames), the A/B behind
                     the default choice
  b_lane_frame     : the same frame through rt_dispatch_rows with rt_set_walk(0): the same lane
                     walks without a ray list, so a - b is the cost of reading 32 B per ray and
                     of 64x1 waves instead of 8x8 tiles in cost order
  c_frame          : the default frame
  rays             : rt_camera_rays alone
Checks that both lists shade to the frame's bytes, and appends one JSON line per config to
--out (default profiles/shade_bench.jsonl) with the ratios a/b and a/c.
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
ap.add_argument("--configs", default="3,5,2")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=10, help="timed launches of each variant per round")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_bench.jsonl"))
a = ap.parse_args()
SCENES = {3: (1920, 1080, 3), 5: (1920, 1080, 3), 2: (800, 600, 1)}  # bench.py's workloads


def tile_order(W, H):
    """Row-order pixel indices listed 8x8 tile by tile (row-major tiles, row-major inside)."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    key = ((ys // 8) * ((W + 7) // 8) + xs // 8) * 64 + (ys % 8) * 8 + xs % 8
    return np.argsort(key.reshape(-1), kind="stable")


stream = torch.cuda.Stream()
lines = []
for config in [int(c) for c in a.configs.split(",")]:
    W, H, bounces = SCENES[config]
    n = W * H
    fs = rtamd.generate(config, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, bounces, True)
    ctx.set_stream(stream.cuda_stream)
    rows = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.camera_rays_device(W, H, 0, H, rows.data_ptr())
    ctx.sync()
    order = torch.from_numpy(tile_order(W, H)).cuda()
    tiles = rows.view(n, 32)[order].contiguous().view(-1)
    px = {k: torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
          for k in ("a_rows", "a_tiles", "a_rows_plain", "a_rows_split", "b_lane_frame", "c_frame")}
    torch.cuda.synchronize()

    def shade(key, rays, split):
        ctx.debug_shade(split)
        ctx.shade_rays_device(rays.data_ptr(), n, px[key].data_ptr(), rtamd.FORMAT_RGBA32F)

    def frame(key, walk):
        ctx.set_walk(walk)
        ctx.dispatch_rows(W, H, 0, 1, 1, H, px[key].data_ptr(), W * 16)

    variants = {
        "a_rows": lambda: shade("a_rows", rows, 0),
        "a_tiles": lambda: shade("a_tiles", tiles, 0),
        "a_rows_plain": lambda: shade("a_rows_plain", rows, 1),
        "a_rows_split": lambda: shade("a_rows_split", rows, 2),
        "b_lane_frame": lambda: frame("b_lane_frame", 0),
        "c_frame": lambda: frame("c_frame", -1),
        "rays": lambda: ctx.camera_rays_device(W, H, 0, H, rows.data_ptr()),
    }
    ms = {k: [] for k in variants}
    for rnd in range(a.rounds + 1):  # round 0 warms every variant up (frames: their cost order too)
        for key, run in variants.items():
            for _ in range(3 if rnd == 0 else a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                stream.synchronize()
                if rnd > 0:
                    ms[key].append(e0.elapsed_time(e1))
    ctx.set_walk(-1)
    ctx.debug_shade(0)
    want = px["c_frame"]
    same = {k: bool(torch.equal(px[k], want)) for k in ("a_rows", "a_rows_plain", "a_rows_split", "b_lane_frame")}
    same["a_tiles"] = bool(torch.equal(px["a_tiles"].view(n, 16), want.view(n, 16)[order]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"config": config, "width": W, "height": H, "bounces": bounces, "rays": n, "rounds": a.rounds,
            "reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
            "mrays_per_s": {k: n / med[k] / 1e3 for k in ("a_rows", "a_tiles")},
            "a_rows_over_b": med["a_rows"] / med["b_lane_frame"], "a_rows_over_c": med["a_rows"] / med["c_frame"],
            "a_tiles_over_b": med["a_tiles"] / med["b_lane_frame"], "a_tiles_over_c": med["a_tiles"] / med["c_frame"],
            "split_over_plain": med["a_rows_split"] / med["a_rows_plain"],
            "equals_frame": same}
    print(json.dumps(line), flush=True)
    lines.append(line)
    assert all(same.values()), f"config {config}: shaded lists and frames differ: {same}"
    ctx.close()
with open(a.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
