"""The reference of tests/test_gpu_shade.py checked against the oracle on the CPU: for a frame's
own camera rays, tests/shade_ref.py's restated bounce loop gives oracle.render's frame within
the project's 1e-4 per channel (the restatement's powf is numpy's, the oracle's glibc's; every
other operation is the same float32 operation), with no ray left out. And the binding's record
layout is the header's.
"""
import os
import re

import numpy as np
import pytest

import gbuffer_ref as gr
import oracle
import rtamd
import shade_ref as sr
import trace_rays as tr

TOL = 1e-4
W, H = tr.CAM_W, tr.CAM_H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (scene, maxBounces, useFresnel, useMollerTrumbore): Fresnel off and on, MT off and on,
# bounces 1 and 3, over the three scenes
CASES = [("cfg2", 1, 0, 0), ("cfg2", 3, 1, 1), ("cfg3", 3, 0, 0), ("cfg3", 3, 1, 0), ("cfg3", 1, 0, 1),
         ("cfg3", 3, 1, 1), ("soup1", 3, 0, 1), ("soup1", 3, 1, 0), ("soup1", 1, 1, 1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_b%d_f%d_mt%d" % c)
def test_restatement_is_the_oracle_frame(case):
    name, bounces, fresnel, mt = case
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    got = sr.shade(fs, o, d, sr.frame_sky(W, H), bounces, bool(fresnel), bool(mt)).reshape(H, W, 4)
    ref, _ = oracle.render(fs, W, H, oracle.params(W, H, bounces, True, fresnel, mt))
    assert got.shape == ref.shape  # every ray of the frame
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bad = int((diff > TOL).any(axis=-1).sum())
    assert bad == 0, f"{case}: {bad} pixels over {TOL}, max {np.nanmax(diff):.3g}"
    assert (got[..., 3] == 1).all()
    # the frame is not trivial: some rays hit something
    bg = sr.background(sr.frame_sky(W, H)).reshape(H, W, 3)
    assert (got[..., :3] == bg).all(axis=-1).sum() < W * H


def test_zero_bounces_and_empty_list():
    fs = tr.scene("cfg3")
    o, d = gr.rays("cfg3", W, H)
    out = sr.shade(fs, o[:100], d[:100], np.full(100, 0.5, np.float32), bounces=0)
    assert (out[:, :3] == 0).all() and (out[:, 3] == 1).all()
    assert sr.shade(fs, o[:0], d[:0], np.zeros(0, np.float32)).shape == (0, 4)


def test_background_is_the_frames():
    """sky = f32(y) / f32(H) reproduces the oracle's background rows bit for bit (an empty scene)."""
    import test_gpu_parity as tg
    fs = tg._empty_scene(W, H)
    ref, _ = oracle.render(fs, W, H, oracle.params(W, H, 3))
    bg = sr.background(sr.frame_sky(W, H)).reshape(H, W, 3)
    assert np.array_equal(bg.view(np.uint32), np.ascontiguousarray(ref[..., :3]).view(np.uint32))


def test_view_ray_dtype_is_the_headers():
    with open(os.path.join(ROOT, "include", "rt_api.h")) as f:
        text = f.read()
    m = re.search(r"typedef struct rt_view_ray \{(.*?)\} rt_view_ray;", text, re.S)
    assert m, "rt_view_ray is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(float|int)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [f[1] for f in fields] == list(rtamd.VIEW_RAY_DTYPE.names) == ["origin", "sky", "dir", "reserved"]
    off = 0
    for ctype, name, count in fields:
        sub, field_off = rtamd.VIEW_RAY_DTYPE.fields[name][:2]
        assert field_off == off, name
        assert sub.base == np.dtype("<f4" if ctype == "float" else "<i4"), name
        off += 4 * int(count or 1)
    assert off == rtamd.VIEW_RAY_DTYPE.itemsize == 32
    asserted = re.search(r"RT_STATIC_ASSERT\(sizeof\(rt_view_ray\) == 32 && offsetof\(rt_view_ray, sky\) == 12 && "
                         r"offsetof\(rt_view_ray, dir\) == 16", text)
    assert asserted, "the header does not pin rt_view_ray's layout"
    rays = rtamd.ComputeShader.make_view_rays([[1, 2, 3]], [[4, 5, 6]], [0.25])
    assert rays.tobytes() == np.array([1, 2, 3, 0.25, 4, 5, 6, 0], np.float32).tobytes()
    assert rtamd.ComputeShader.make_view_rays([[1, 2, 3]], [[4, 5, 6]])["sky"][0] == 0
