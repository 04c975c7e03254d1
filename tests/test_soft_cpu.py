"""rt_set_soft_shadows without a device: the numpy reference of tests/test_gpu_soft.py
(tests/soft_ref.py) anchored to tests/lights_ref.py -- radii so small that every sample point is
the light, and radii of 0 -- the fixed lights really cast penumbrae; the soft frame is nowhere
darker than the fully blocked one; the routing rule of csrc/dispatch_plan.h and the SoftSet
kernel argument's layout (tests/native/soft_check.cpp); the header's and the binding's
declarations.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import gbuffer_ref as gr
import lights_ref as lr
import rtamd
import shade_ref as sr
import soft_ref as sf
import trace_rays as tr

W, H = tr.CAM_W, tr.CAM_H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("cfg2", "cfg3", "soup1")
K0 = 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def hard(name, fresnel, mt):
    """lights_ref's frame of the first three fixed lights; computed once, read-only."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    out = lr.shade(fs, o, d, sr.frame_sky(W, H), lr.fixed_lights(fs, 3), 3, bool(fresnel), bool(mt))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def soft(name, all_blocked=False):
    """(soft_ref's frame of the first three fixed lights at radius 2.0, K = 16; its info)."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    info = {}
    out = sf.shade(fs, o, d, sr.frame_sky(W, H), lr.fixed_lights(fs, 3), (2.0, 2.0, 2.0), K0, info=info,
                   all_blocked=all_blocked)
    out.setflags(write=False)
    return out, info


@pytest.mark.parametrize("name", SCENES)
def test_tiny_radii_are_the_hard_frame(name):
    """Anchor 1: radii of 1e-30 for every light, K = 16 -- every sample ray is the hard ray, bit
    for bit (the light at (0, -14, 0) included, whose x and z are zero), so every b_i is 0 or K
    and the frame is lights_ref.shade's bit for bit."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    lights = lr.fixed_lights(fs, 3)
    info = {}
    got = sf.shade(fs, o, d, sr.frame_sky(W, H), lights, (1e-30,) * 3, K0, info=info)
    assert np.array_equal(bits(got), bits(hard(name, 0, 0))), name
    b = info["blocked0"]
    assert (info["rays0"] == K0).all() and np.isin(b, (-1, 0, K0)).all()
    hinfo = {}
    lr.shade(fs, o, d, sr.frame_sky(W, H), lights, info=hinfo)
    assert np.array_equal(np.where(b < 0, -1, b // K0), hinfo["shadow0"])


@pytest.mark.parametrize("name", SCENES)
def test_radii_of_zero_are_lights_ref(name):
    """Anchor 2: radii all 0 (and K = 1) through soft_ref: lights_ref bit for bit, Fresnel and
    the triangle test off and on; so is K = 16 with radii 0, which sends one ray per light."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    lights = lr.fixed_lights(fs, 3)
    for fresnel, mt in ((0, 0), (1, 1)):
        got = sf.shade(fs, o, d, sr.frame_sky(W, H), lights, (0.0, 0.0, 0.0), 1, 3, bool(fresnel), bool(mt))
        assert np.array_equal(bits(got), bits(hard(name, fresnel, mt))), (name, fresnel, mt)
    info = {}
    got = sf.shade(fs, o, d, sr.frame_sky(W, H), lights, (), K0, info=info)
    assert np.array_equal(bits(got), bits(hard(name, 0, 0)))
    assert (info["rays0"] == 1).all() and info["blocked0"].max() == 1


@pytest.mark.parametrize("name", SCENES)
def test_the_penumbra_is_real(name):
    """The first three fixed lights at radius 2.0, K = 16: some light gives 0 < b < K at 5 % or
    more of the camera-hit pixels (a kernel that reused one sample's answer would not pass the
    GPU test), and the frame differs from the hard one."""
    got, info = soft(name)
    b = info["blocked0"]
    hit = b[:, 0] >= 0
    partial = (b > 0) & (b < K0)
    share = partial[hit].mean(axis=0)
    print(f"{name}: share of camera hits with 0 < b < K per light: {share}")
    assert hit.sum() > 0 and share.max() >= 0.05, (name, share)
    assert not np.array_equal(bits(got), bits(hard(name, 0, 0)))


@pytest.mark.parametrize("name", SCENES)
def test_soft_is_between_lit_and_fully_blocked(name):
    """No NaN, and the soft frame is nowhere darker than the frame with every light fully blocked
    (every factor is at least 1 - 0.7 = 0.3, every term non-negative)."""
    got, _ = soft(name)
    dark, _ = soft(name, True)
    assert not np.isnan(got).any() and not np.isnan(dark).any()
    assert (got[:, :3] >= dark[:, :3]).all()
    assert (got[:, :3] > dark[:, :3]).any()


def test_the_full_factor_is_the_hard_factor():
    """1.0f - 0.7f * (K / K) is 0.3f's bits for every K the tests use, in float32."""
    F = np.float32
    for K in (1, 2, 3, 4, 8, 16, 64):
        assert bits(F(1.0) - F(0.7) * (F(K) / F(K))) == bits(F(0.3)), K


def test_the_rotation_index_spreads():
    """Step 3's j takes all 16 values over the camera hits of a frame, each between half and
    twice its even share."""
    g = gr.reference("cfg3", W, H, 0)
    hitp = g["position"].reshape(-1, 4)[g["shape"].reshape(-1) >= 0, :3]
    n = np.bincount(sf.rotation_index(hitp), minlength=16)
    assert n.min() >= len(hitp) / 32 and n.max() <= len(hitp) / 8, n


def test_routing_rule_and_soft_set_layout(tmp_path):
    """tests/native/soft_check.cpp: soft_route for every count, radius pattern, stats and
    accelerator case; lights_route as it was; the SoftSet argument as make_soft_set fills it."""
    exe = str(tmp_path / "soft_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "soft_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "soft_check ok" in r.stdout and " 0 failed" in r.stdout


def test_declarations():
    """The header declares the two calls, RT_MAX_SHADOW_SAMPLES = 64 and RT_KERNEL_SOFT = 5; the
    binding has both symbols and the constants; no device is needed for the argument checks."""
    with open(os.path.join(ROOT, "include", "rt_api.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"enum\s*\{\s*RT_MAX_SHADOW_SAMPLES\s*=\s*64\s*\}", text)
    assert re.search(r"RT_KERNEL_SOFT\s*=\s*5\b", text)
    assert re.search(r"int\s+rt_set_soft_shadows\(struct rt_ctx\* ctx, const float\* radii, int count, int samples\);",
                     text)
    assert re.search(r"int\s+rt_get_soft_shadows\(struct rt_ctx\* ctx, float\* radii, int cap, int\* count, "
                     r"int\* samples\);", text)
    assert rtamd.MAX_SHADOW_SAMPLES == sf.MAX_SHADOW_SAMPLES == 64 and rtamd.KERNEL_SOFT == 5
    assert "rt_set_soft_shadows" in rtamd.RT_SYMBOLS and "rt_get_soft_shadows" in rtamd.RT_SYMBOLS
    assert hasattr(rtamd.ComputeShader, "set_soft_shadows") and hasattr(rtamd.ComputeShader, "get_soft_shadows")
    lib = rtamd.rt_lib()
    radii = np.array([1.0, 0.5], np.float32)
    assert lib.rt_set_soft_shadows(None, radii.ctypes.data, 2, 16) == -1
    assert lib.rt_set_soft_shadows(None, None, 0, 0) == -1
    assert lib.rt_get_soft_shadows(None, None, 0, None, None) == -1
