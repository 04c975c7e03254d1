"""Adaptive supersampling (rt_set_adaptive) against full supersampling and the one-sample frame.

    python tools/bench_adaptive.py [--configs 3,2] [--samples 2,4] [--thresholds 0.0625,0.015625]
                                   [--rounds 5] [--frames 20] [--out FILE]

For each config at its tools/ab.py size, each n and each threshold, interleaved rounds in one
process of
  one      : the plain one-sample W x H frame
  full     : rt_set_samples(n), adaptive off (k_accel averages each n x n block in its store)
  adaptive : rt_set_adaptive(threshold): the one-sample frame, the classify kernel and the
             refine kernel over the listed pixels (fast path)
  general  : the same with rt_debug_ss_general(1): the whole sample frame, then the adaptive
             filter kernel (what every frame k_accel does not render takes)
Prints one JSON line per (config, n, threshold) with the median, minimum and maximum device ms
of each arm (HIP events around the whole dispatch, every pass included), the refined share
from rt_adaptive_stats, and checks that the two adaptive arms render identical images.
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

WL = {2: (2, 800, 600, 1), 3: (3, 1920, 1080, 3), 5: (5, 1920, 1080, 3)}  # tools/ab.py

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,2")
ap.add_argument("--samples", default="2,4")
ap.add_argument("--thresholds", default="0.0625,0.015625")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--walk", type=int, default=-1, help="rt_set_walk for every arm (-1: the automatic policy)")
ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
a = ap.parse_args()

lines = []
for config in [int(c) for c in a.configs.split(",")]:
    cfg, W, H, mb = WL[config]
    fs = rtamd.generate(cfg, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, mb, True)
    ctx.set_walk(a.walk)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for n in [int(s) for s in a.samples.split(",")]:
        for thr in [float(t) for t in a.thresholds.split(",")]:
            # arm: (samples, threshold, forced general path)
            variants = {"one": (1, -1.0, 0), "full": (n, -1.0, 0), "adaptive": (n, thr, 0), "general": (n, thr, 1)}
            res = {v: [] for v in variants}
            img, share = {}, {}
            for rnd in range(a.rounds):
                for v, (samples, t, general) in variants.items():
                    ctx.set_samples(samples)
                    ctx.set_adaptive(t)
                    ctx.debug_ss_general(general)
                    ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)  # also rebuilds the cost order
                    ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
                    ctx.sync()
                    assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
                    if rnd == 0:
                        img[v] = out.cpu().numpy()
                        if t >= 0:
                            refined, pixels = ctx.adaptive_stats()
                            assert pixels == W * H
                            share[v] = refined / pixels
                    ctx.kernel_times()
                    for _ in range(a.frames):
                        ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
                    res[v].extend(ctx.kernel_times().tolist())
            same = bool(np.array_equal(img["adaptive"], img["general"])) and share["adaptive"] == share["general"]
            med = {v: float(np.median(t)) for v, t in res.items()}
            line = {"config": config, "width": W, "height": H, "maxBounces": mb, "samples": n, "threshold": thr,
                    "walk": a.walk,
                    "rounds": a.rounds, "frames": a.frames, "refined_share": share["adaptive"],
                    "median_ms": med, "min_ms": {v: float(np.min(t)) for v, t in res.items()},
                    "max_ms": {v: float(np.max(t)) for v, t in res.items()},
                    "adaptive_over_full": med["adaptive"] / med["full"],
                    "adaptive_over_one": med["adaptive"] / med["one"],
                    "general_over_full": med["general"] / med["full"],
                    "adaptive_equals_general": same,
                    "max_diff_from_full": float(np.abs(img["adaptive"] - img["full"]).max()),
                    "mean_diff_from_full": float(np.abs(img["adaptive"] - img["full"])[..., :3].mean()),
                    "mean_diff_one_from_full": float(np.abs(img["one"] - img["full"])[..., :3].mean())}
            print(json.dumps(line), flush=True)
            lines.append(line)
            assert same, f"config {config} n={n} threshold {thr}: the adaptive arms differ"
    ctx.set_samples(1)
    ctx.set_adaptive(-1.0)
    ctx.debug_ss_general(0)
    ctx.close()
    del out
if a.out:
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
