"""rt_set_lights without a device: the numpy reference of tests/test_gpu_lights.py
(tests/lights_ref.py) anchored to tests/shade_ref.py and through it to the oracle's frame; the
fixed test lights really give different shadow answers; the routing rule of
csrc/dispatch_plan.h and the LightSet kernel argument's layout (tests/native/lights_check.cpp);
the header's and the binding's declarations.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import gbuffer_ref as gr
import lights_ref as lr
import oracle
import rtamd
import shade_ref as sr
import trace_rays as tr

W, H = tr.CAM_W, tr.CAM_H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("cfg2", "cfg3", "soup1")
# tests/test_shade_cpu.py's bound of shade_ref against the oracle's frame (numpy's powf against glibc's)
ORACLE_TOL = 1e-4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def one_light(name, fresnel, mt):
    """shade_ref's frame of the scene's own light; computed once, read-only."""
    o, d = gr.rays(name, W, H)
    out = sr.shade(tr.scene(name), o, d, sr.frame_sky(W, H), 3, bool(fresnel), bool(mt))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", SCENES)
def test_one_light_is_shade_ref_and_the_oracle(name):
    """Anchor 1: with one light the reference is shade_ref.shade bit for bit (Fresnel and the
    triangle test off and on), and that frame is oracle.render's within shade_ref's own bound."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    for fresnel, mt in ((0, 0), (1, 1)):
        got = lr.shade(fs, o, d, sr.frame_sky(W, H), fs.light, 3, bool(fresnel), bool(mt))
        assert np.array_equal(bits(got), bits(one_light(name, fresnel, mt))), (name, fresnel, mt)
    ref, _ = oracle.render(fs, W, H, oracle.params(W, H, 3, True, 0, 0))
    got = one_light(name, 0, 0).reshape(H, W, 4)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert not (diff > ORACLE_TOL).any(), f"{name}: max {np.nanmax(diff):.3g}"


@pytest.mark.parametrize("name", SCENES)
def test_a_black_light_changes_nothing(name):
    """Anchor 2: a second light of colour (0, 0, 0) at a finite distance from every hit gives
    the one-light frame as floats, NaN where that frame has NaN."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    lights = np.concatenate([rtamd.as_records(fs.light, rtamd.LIGHT_DTYPE).reshape(-1)[:1], lr.fixed_lights(fs, 2)[1:]])
    lights["color"][1] = 0
    for fresnel, mt in ((0, 0), (1, 1)):
        got = lr.shade(fs, o, d, sr.frame_sky(W, H), lights, 3, bool(fresnel), bool(mt))
        want = one_light(name, fresnel, mt)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert ((got == want) | np.isnan(want)).all(), (name, fresnel, mt)


@pytest.mark.parametrize("count", [3, 8])
@pytest.mark.parametrize("name", SCENES)
def test_the_fixed_lights_disagree_about_shadows(name, count):
    """Among the camera rays' hit pixels at least 5 % get different shadow answers from different
    lights (a kernel that reused one light's answer would not pass the GPU test), the frame has
    no NaN, and one more light only adds light."""
    fs = tr.scene(name)
    o, d = gr.rays(name, W, H)
    info = {}
    lights = lr.fixed_lights(fs, count)
    got = lr.shade(fs, o, d, sr.frame_sky(W, H), lights, 3, False, False, info=info)
    s0 = info["shadow0"]
    hit = s0[:, 0] >= 0
    differ = hit & (s0.min(axis=1) != s0.max(axis=1))
    assert hit.sum() > 0 and differ.sum() >= 0.05 * hit.sum(), (name, int(differ.sum()), int(hit.sum()))
    assert not np.isnan(got).any()
    assert len({tuple(c) for c in lights["color"].tolist()}) == count  # distinct colours
    # every term is a non-negative sum: a prefix of the set is no brighter anywhere it is finite
    fewer = lr.shade(fs, o, d, sr.frame_sky(W, H), lights[:count - 1], 3, False, False)
    assert (got[:, :3] >= fewer[:, :3]).all()
    assert (got[:, :3] > fewer[:, :3]).any()


def test_routing_rule_and_light_set_layout(tmp_path):
    """tests/native/lights_check.cpp: lights_route for every count, stats and accelerator case,
    what samples_plan makes of such a frame, and the LightSet argument as make_light_set fills it."""
    exe = str(tmp_path / "lights_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "lights_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lights_check ok" in r.stdout and " 0 failed" in r.stdout


def test_declarations():
    """The header declares the two calls, RT_MAX_LIGHTS = 8 and RT_KERNEL_LIGHTS = 4; the binding
    has both symbols and the constants; no device is needed for the argument checks."""
    with open(os.path.join(ROOT, "include", "rt_api.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"enum\s*\{\s*RT_MAX_LIGHTS\s*=\s*8\s*\}", text)
    assert re.search(r"RT_KERNEL_LIGHTS\s*=\s*4\b", text)
    assert re.search(r"int\s+rt_set_lights\(struct rt_ctx\* ctx, const FlatLight\* lights, int count\);", text)
    assert re.search(r"int\s+rt_get_lights\(struct rt_ctx\* ctx, FlatLight\* lights, int cap, int\* count\);", text)
    assert rtamd.MAX_LIGHTS == lr.MAX_LIGHTS == 8 and rtamd.KERNEL_LIGHTS == 4
    lib = rtamd.rt_lib()
    lights = lr.fixed_lights(tr.scene("cfg3"), 2)
    assert lib.rt_set_lights(None, lights.ctypes.data, 2) == -1
    assert lib.rt_get_lights(None, None, 0, None) == -1
