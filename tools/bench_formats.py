"""Display formats (rt_set_surface_format): device time of the frame and the cost of reading it back.

    python tools/bench_formats.py [--configs 3,2] [--rounds 5] [--frames 20] [--out FILE]

For each config at its tools/ab.py size and each surface format (RGBA32F, RGBA8, SRGBA8, RGBA16F),
interleaved rounds in one process of
  device   : rt_dispatch into the context surface, frames back to back; the device ms of each
             dispatch from rt_kernel_times (HIP events around the render kernel)
  readback : rt_dispatch + rt_read_surface into pinned host memory, one frame at a time; host
             wall ms per frame (what a host that looks at every frame waits for)
  two_pass : (8-bit and half formats) the same device time with rt_debug_convert_pass(1): the
             float frame into a scratch surface, then a conversion kernel -- what a host could do
             before the kernels converted in their stores
Appends one JSON line per (config, format) to profiles/format_bench.jsonl (or --out) with the
median and the spread (min, max) of each, and checks every frame against tests/fmt_ref.py
applied to the float frame.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fmt_ref  # noqa: E402
import rtamd  # noqa: E402

WL = {2: (2, 800, 600, 1), 3: (3, 1920, 1080, 3)}  # tools/ab.py
FORMATS = {"rgba32f": rtamd.FORMAT_RGBA32F, "rgba8": rtamd.FORMAT_RGBA8, "srgba8": rtamd.FORMAT_SRGBA8,
           "rgba16f": rtamd.FORMAT_RGBA16F}

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,2")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "format_bench.jsonl"))
a = ap.parse_args()


def stat(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


T = rtamd.srgb_thresholds()
lines = []
for config in [int(c) for c in a.configs.split(",")]:
    cfg, W, H, mb = WL[config]
    fs = rtamd.generate(cfg, 0, W, H)
    ctx = rtamd.ComputeShader(0)
    ctx.upload(fs)
    ctx.set_params(W, H, mb, True)
    pinned = {n: torch.empty((H, W, 4), dtype={np.float32: torch.float32, np.uint8: torch.uint8,
                                               np.float16: torch.float16}[rtamd.SURFACE_DTYPE[f]],
                             pin_memory=True).numpy() for n, f in FORMATS.items()}
    res = {n: {"device": [], "readback": [], "two_pass": []} for n in FORMATS}
    img = {}
    for rnd in range(a.rounds):
        for name, f in FORMATS.items():
            for two_pass in ([0, 1] if f != rtamd.FORMAT_RGBA32F else [0]):
                ctx.debug_convert_pass(two_pass)
                ctx.set_surface_format(f)
                ctx.dispatch(W, H)  # also reallocates the surface and rebuilds the cost order
                ctx.dispatch(W, H)
                ctx.sync()
                assert ctx.accel_info()["last_kernel"] == rtamd.KERNEL_ACCEL
                if rnd == 0:
                    img[name, two_pass] = ctx.read_surface(W, H)
                ctx.kernel_times()
                for _ in range(a.frames):
                    ctx.dispatch(W, H)
                res[name]["two_pass" if two_pass else "device"].extend(ctx.kernel_times().tolist())
            ctx.debug_convert_pass(0)
            ctx.dispatch(W, H)
            ctx.read_surface(W, H, out=pinned[name])
            for _ in range(a.frames):
                t0 = time.perf_counter()
                ctx.dispatch(W, H)
                ctx.read_surface(W, H, out=pinned[name])
                res[name]["readback"].append((time.perf_counter() - t0) * 1e3)
            ctx.kernel_times()
    ref32 = img["rgba32f", 0]
    for name, f in FORMATS.items():
        ok = True
        if f != rtamd.FORMAT_RGBA32F:
            want = fmt_ref.convert(ref32, f, T)
            for two_pass in (0, 1):
                ok = ok and bool(np.array_equal(img[name, two_pass], want, equal_nan=True))
        line = {"tool": "bench_formats", "config": config, "width": W, "height": H, "maxBounces": mb, "format": name,
                "bytes_per_frame": int(pinned[name].nbytes), "rounds": a.rounds, "frames": a.frames,
                "device_ms": stat(res[name]["device"]), "readback_wall_ms": stat(res[name]["readback"]),
                "two_pass_device_ms": stat(res[name]["two_pass"]) if res[name]["two_pass"] else None,
                "equals_fmt_ref": ok, "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
        print(json.dumps(line), flush=True)
        lines.append(line)
        assert ok, f"config {config} {name}: the frame differs from fmt_ref of the float frame"
    ctx.set_surface_format(rtamd.FORMAT_RGBA32F)
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
