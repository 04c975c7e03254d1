"""Frames of area lights (rt_set_soft_shadows) against the hard frame of the same lights and
against k_lights' frame of eight point lights.

    python tools/bench_soft.py [--configs 3,2,5] [--lights 1,3] [--samples 4,8,16,64] [--radius 1.0]
                               [--rounds 3] [--reps 5] [--out FILE]

For the car (config 3, 1920x1080, 3 bounces), the monkey scene (config 2, 800x600, 1 bounce) and
the 100k-triangle scene (config 5, 1920x1080, 3 bounces), device time per dispatch (HIP events on
the context's stream around one launch on a device buffer, the lights and radii set before the
first event; interleaved rounds in one process after warm-up launches of each; median, minimum
and maximum over rounds x reps):
  hard_L    : the hard frame of the first L lights (L = 1: k_accel, today's path; else k_lights)
  soft_L_K  : the same lights at --radius with K shadow rays each (k_soft, frame mode), later
              bounces' sample rays per live lane (rt_debug_soft form 2)
  pack_L_K  : the same frame with those rays repacked over the wave (form 1); checked to write
              the same bytes as soft_L_K
  lights_8  : k_lights' frame of eight point lights
soft_1_8 walks as many shadow packets from the same hits as lights_8 and evaluates Phong once
instead of eight times, so it is expected to be no slower: "no slower" is within the larger of
the two min-max spreads. Each soft frame also reports its cost per added sample ray,
(soft - hard) / (L K), and pack / soft. Appends one JSON line per config to --out (default
profiles/soft_bench.jsonl).
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
ap.add_argument("--lights", default="1,3")
ap.add_argument("--samples", default="4,8,16,64")
ap.add_argument("--radius", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5, help="timed launches of each variant per round")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_bench.jsonl"))
a = ap.parse_args()
SCENES = {3: (1920, 1080, 3), 5: (1920, 1080, 3), 2: (800, 600, 1)}  # bench.py's workloads
COUNTS = [int(c) for c in a.lights.split(",")]
SAMPLES = [int(k) for k in a.samples.split(",")]
# lights 1..7 (tools/bench_lights.py's): the scene light's position moved by these vectors, in
# these colours; light 0 is the scene's own
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
    fs = rtamd.generate(config, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, bounces, True)
    ctx.set_stream(stream.cuda_stream)
    # key -> (lights, K or 0 for the hard frame)
    variants = {"lights_8": (8, 0, 0)}
    for c in COUNTS:
        variants[f"hard_{c}"] = (c, 0, 0)
        for k in SAMPLES:
            variants[f"soft_{c}_{k}"] = (c, k, 2)
            variants[f"pack_{c}_{k}"] = (c, k, 1)
    px = torch.zeros(W * H * 16, dtype=torch.uint8, device="cuda")
    kept = {}
    torch.cuda.synchronize()

    def setup(key):
        count, k, form = variants[key]
        ctx.set_lights(light_set(fs, count))
        ctx.set_soft_shadows([a.radius] * count if k else None, k or 1)
        ctx.debug_soft(form)

    def run(key):
        ctx.dispatch_rows(W, H, 0, 1, 1, H, px.data_ptr(), W * 16)

    ms = {k: [] for k in variants}
    kinds = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every variant up (the one-light frame: its cost order too)
        for key in variants:
            setup(key)
            for _ in range(2 if rnd == 0 else a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run(key)
                e1.record(stream)
                stream.synchronize()
                if rnd > 0:
                    ms[key].append(e0.elapsed_time(e1))
            kinds[key] = ctx.accel_info()["last_kernel"]
            if rnd == 0 and key.startswith(("soft", "pack")):
                kept[key] = px.clone()
    same = {k[5:]: bool(torch.equal(kept[k], kept["soft" + k[4:]])) for k in kept if k.startswith("pack")}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lo = {k: float(np.min(v)) for k, v in ms.items()}
    hi = {k: float(np.max(v)) for k, v in ms.items()}
    line = {"config": config, "width": W, "height": H, "bounces": bounces, "radius": a.radius, "rounds": a.rounds,
            "reps": a.reps, "median_ms": med, "min_ms": lo, "max_ms": hi, "last_kernel": kinds,
            "pack_equals_soft": same,
            "pack_over_soft": {f"{c}_{k}": med[f"pack_{c}_{k}"] / med[f"soft_{c}_{k}"] for c in COUNTS for k in SAMPLES},
            "us_per_added_sample_ray": {f"{c}_{k}": 1e3 * (med[f"soft_{c}_{k}"] - med[f"hard_{c}"]) / (c * k)
                                        for c in COUNTS for k in SAMPLES}}
    if "soft_1_8" in med:
        spread = max(hi["soft_1_8"] - lo["soft_1_8"], hi["lights_8"] - lo["lights_8"])
        line["soft_1_8_over_lights_8"] = med["soft_1_8"] / med["lights_8"]
        line["soft_1_8_minus_lights_8_ms"] = med["soft_1_8"] - med["lights_8"]
        line["larger_spread_ms"] = spread
        line["soft_1_8_no_slower"] = bool(med["soft_1_8"] - med["lights_8"] <= spread)
    print(json.dumps(line), flush=True)
    lines.append(line)
    assert all(same.values()), f"config {config}: the repacked form writes other bytes: {same}"
    ctx.close()
with open(a.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
