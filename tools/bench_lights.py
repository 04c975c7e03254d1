"""Frames of several point lights (rt_set_lights) against L one-light frames and against the
same rays as a list.

    python tools/bench_lights.py [--configs 3,2,5] [--lights 2,4,8] [--rounds 3] [--reps 10] [--out FILE]

For the car (config 3, 1920x1080, 3 bounces), the monkey scene (config 2, 800x600, 1 bounce) and
the 100k-triangle scene (config 5, 1920x1080, 3 bounces), device time per call (HIP events on
the context's stream around one launch on device buffers, interleaved rounds in one process
after warm-up launches of each, median and minimum):
  frame_1  : the one-light frame, today's path (k_accel)
  list_1   : rt_shade_rays over the frame's rt_camera_rays list in raster order, one light
  frame_L  : the L-light frame (k_lights, frame mode: camera rays and their L shadow rays as
             packets), L = 2, 4, 8
  list_L   : the same rays through rt_shade_rays (k_lights, list mode: every walk per lane)
Each L-light frame is reported against L x frame_1 (the camera walk and the bounces' closest
walks are shared, so it should come in under that product) and against list_L (the frame
mode's packets must earn their kernel). Checks that frame_L and list_L write the same bytes,
and appends one JSON line per config to --out (default profiles/lights_bench.jsonl).
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
ap.add_argument("--configs", default="3,2,5")
ap.add_argument("--lights", default="2,4,8")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=10, help="timed launches of each variant per round")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights_bench.jsonl"))
a = ap.parse_args()
SCENES = {3: (1920, 1080, 3), 5: (1920, 1080, 3), 2: (800, 600, 1)}  # bench.py's workloads
COUNTS = [int(c) for c in a.lights.split(",")]
# lights 1..7: the scene light's position moved by these vectors, in these colours (a key
# light and fills around it); light 0 is the scene's own
OFFSETS = ((-8.0, 0.0, 3.0), (6.0, 2.0, -4.0), (0.0, 4.0, 6.0), (-5.0, -1.0, -6.0), (4.0, 5.0, 4.0),
           (9.0, 1.0, 0.0), (-3.0, 6.0, -2.0))
COLOURS = ((1.0, 2.0, 4.0), (4.0, 2.0, 1.0), (3.0, 0.5, 0.5), (0.5, 3.0, 0.5), (0.5, 0.5, 3.0), (2.0, 2.0, 0.25),
           (0.25, 2.0, 2.0))


def light_set(fs, count):
    own = rtamd.as_records(fs.light, rtamd.LIGHT_DTYPE).reshape(-1)[0]
    out = np.zeros(count, rtamd.LIGHT_DTYPE)
    out[0] = own
    for k in range(1, count):
        out["position"][k] = own["position"] + np.array(OFFSETS[k - 1], np.float32)
        out["color"][k] = COLOURS[k - 1]
    return out


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
    rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.camera_rays_device(W, H, 0, H, rays.data_ptr())
    ctx.sync()
    keys = [f"{form}_{c}" for c in [1] + COUNTS for form in ("frame", "list")]
    px = {k: torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for k in keys}
    torch.cuda.synchronize()

    def run(key):
        form, count = key.split("_")
        ctx.set_lights(light_set(fs, int(count)))
        if form == "frame":
            ctx.dispatch_rows(W, H, 0, 1, 1, H, px[key].data_ptr(), W * 16)
        else:
            ctx.shade_rays_device(rays.data_ptr(), n, px[key].data_ptr(), rtamd.FORMAT_RGBA32F)

    ms = {k: [] for k in keys}
    kinds = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every variant up (the one-light frame: its cost order too)
        for key in keys:
            for _ in range(3 if rnd == 0 else a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run(key)
                e1.record(stream)
                stream.synchronize()
                if rnd > 0:
                    ms[key].append(e0.elapsed_time(e1))
            if key.startswith("frame"):
                kinds[key] = ctx.accel_info()["last_kernel"]
    same = {c: bool(torch.equal(px[f"frame_{c}"], px[f"list_{c}"])) for c in [1] + COUNTS}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"config": config, "width": W, "height": H, "bounces": bounces, "rays": n, "rounds": a.rounds,
            "reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
            "last_kernel": kinds,
            "frame_over_L_one_light_frames": {c: med[f"frame_{c}"] / (c * med["frame_1"]) for c in COUNTS},
            "frame_over_list": {c: med[f"frame_{c}"] / med[f"list_{c}"] for c in COUNTS},
            "frame_equals_list": same}
    print(json.dumps(line), flush=True)
    lines.append(line)
    assert all(same.values()), f"config {config}: frames and lists differ: {same}"
    ctx.close()
with open(a.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
