"""Supersampled frames (rt_set_samples): the fused store against the general path.

    python tools/bench_ss.py [--configs 3,2] [--samples 2,4] [--rounds 5] [--frames 20] [--out FILE]

For each config at its tools/ab.py size and each n, interleaved rounds in one process of
  fused   : rt_set_samples(n), k_accel averages each n x n block in its store
  general : the same with rt_debug_ss_general(1): the n*W x n*H one-sample frame into
            the context's scratch surface, then k_box_filter (what a host could do
            before rt_set_samples, minus its own second surface)
  one     : the plain one-sample W x H frame
Prints one JSON line per (config, n) with the median device ms of each (HIP events
around the whole dispatch, filter kernel included) and checks that fused and general
render identical images.
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

WL = {2: (2, 800, 600, 1), 3: (3, 1920, 1080, 3), 4: (3, 3840, 2160, 3), 5: (5, 1920, 1080, 3)}  # tools/ab.py

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,2")
ap.add_argument("--samples", default="2,4")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
a = ap.parse_args()

lines = []
for config in [int(c) for c in a.configs.split(",")]:
    cfg, W, H, mb = WL[config]
    fs = rtamd.generate(cfg, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, mb, True)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for n in [int(s) for s in a.samples.split(",")]:
        variants = {"fused": (n, 0), "general": (n, 1), "one": (1, 0)}
        res = {v: [] for v in variants}
        img = {}
        for rnd in range(a.rounds):
            for v, (samples, general) in variants.items():
                ctx.set_samples(samples)
                ctx.debug_ss_general(general)
                ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)  # also rebuilds the cost order
                ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
                ctx.sync()
                assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
                if rnd == 0:
                    img[v] = out.cpu().numpy()
                ctx.kernel_times()
                for _ in range(a.frames):
                    ctx.dispatch_rows(W, H, 0, 1, 1, H, out.data_ptr(), W * 16)
                res[v].extend(ctx.kernel_times().tolist())
        same = bool(np.array_equal(img["fused"], img["general"]))
        med = {v: float(np.median(t)) for v, t in res.items()}
        line = {"config": config, "width": W, "height": H, "maxBounces": mb, "samples": n,
                "rounds": a.rounds, "frames": a.frames,
                "median_ms": med, "min_ms": {v: float(np.min(t)) for v, t in res.items()},
                "fused_over_general": med["fused"] / med["general"],
                "fused_over_one": med["fused"] / med["one"],
                "fused_equals_general": same,
                "max_diff_from_one_sample": float(np.abs(img["fused"] - img["one"]).max())}
        print(json.dumps(line), flush=True)
        lines.append(line)
        assert same, f"config {config} n={n}: fused and general images differ"
    ctx.set_samples(1)
    ctx.debug_ss_general(0)
    ctx.close()
    del out
if a.out:
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
