"""Geometry buffers (rt_dispatch_gbuffer), the parts that need no GPU.

1. The reference of tests/gbuffer_ref.py restates the normal and the distance in numpy; here
   that restatement is shown to be the oracle's own: position + normal * 1e-3 is, bit for bit,
   the origin of the shadow ray the oracle's main() casts from the same hit.
2. Every camera ray set tests/test_gpu_gbuffer.py renders is walked by the scalar emulation of
   the accelerated walk (tests/native/accel_check.cpp) and by the oracle: same shape, same
   distance bits, no ray left out. A mismatch on the device is then the device's.
3. rt_gbuffer's layout as a C compiler sees it against the ctypes structure, and the binding.
4. The row mapping of gbuffer_ref against image_row's formula.
1, 2 and 4 guard the inputs and pass without the feature; 3 needs it.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gbuffer_ref as gr
import rtamd
import trace_rays as tr
from test_accel_cpu import check_lib, compare  # noqa: F401  (check_lib: the emulation's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every (scene variant, size) the GPU tests compare with a reference
FRAMES = [("", gr.W0, gr.H0), ("", gr.W1, gr.H1), (":far", gr.W0, gr.H0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frames_of(name):
    out = [(name + v, W, H) for v, W, H in FRAMES]
    if name == "cfg3":
        out += [("cfg3:anim", gr.WA, gr.HA), ("cfg3", gr.WA, gr.HA), ("cfg3:ties", gr.W0, gr.H0)]
        out += [("cfg3", W, H) for W, H in gr.EDGE_SIZES if (W, H) != (gr.W1, gr.H1)]
    return out


@pytest.mark.parametrize("name", tr.SCENES)
def test_the_restatement_is_the_oracles(name):
    """1. Hit point + restated normal * 1e-3 == the oracle's shadow-ray origin, and the restated
    distance == the oracle's, bit for bit, for every hit pixel of every frame used on the GPU."""
    f = np.float32
    for key, W, H in frames_of(name):
        for mt in (0, 1):
            ref = gr.reference(key, W, H, mt)
            want, have = gr.shadow_origins(key, W, H, mt)
            shape = ref["shape"].reshape(-1)
            pos, nrm = ref["position"].reshape(-1, 4), ref["normal"].reshape(-1, 4)
            hit = shape >= 0
            assert np.array_equal(hit, have), (key, W, H, mt)
            got = (pos[:, :3] + nrm[:, :3] * f(1e-3)).astype(f)
            bad = np.where((bits(got) != bits(want)).any(axis=1) & hit)[0]
            assert bad.size == 0, f"{key} {W}x{H} mt {mt}: {bad.size} shadow origins differ, e.g. pixel {bad[0]}"
            o, _ = gr.rays(key, W, H)
            v = (o - pos[:, :3]).astype(f)
            dist = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=f)
            assert np.array_equal(bits(dist[hit]), bits(ref["depth"].reshape(-1)[hit])), (key, W, H, mt)
            # misses: the values rt_api.h fixes
            assert (ref["depth"].reshape(-1)[~hit] == f(1e20)).all() and (shape[~hit] == -1).all()
            assert not pos[~hit].any() and not nrm[~hit].any() and (pos[hit, 3] == 1).all() and not nrm[:, 3].any()
    # the full frame exercises the hit branch, and the sphere branch where the scene has spheres
    ref = gr.reference(name, gr.W0, gr.H0, 0)
    shape = ref["shape"].reshape(-1)
    hit = shape >= 0
    assert hit.sum() > 1000, name
    spheres = (gr.scene(name).shapes["type"][shape[hit]] == rtamd.SPHERE).sum()
    if name != "cfg5":
        assert spheres > 100, (name, spheres)


def test_far_camera_still_sees_the_scene():
    """The far camera of GPU test 3 hits the scene in the pixel counts the test plan states."""
    counts = [int((gr.reference(n + ":far", gr.W0, gr.H0, 0)["shape"] >= 0).sum()) for n in tr.SCENES]
    assert counts == [5184, 2301, 2974, 5184], counts


@pytest.mark.parametrize("name", tr.SCENES)
def test_camera_rays_are_exact_on_the_cpu(check_lib, name):
    """2. The emulated accelerated walk against the oracle for every frame's camera rays, both
    trees, both triangle tests, no ray left out."""
    for key, W, H in frames_of(name):
        fs = gr.scene(key)
        o, d = gr.rays(key, W, H)
        assert len(o) == W * H
        lim = np.full(len(o), 50.0, np.float32)
        for tree in (1, 0):
            for mt in (0, 1):
                compare(check_lib, fs, o, d, lim, tree, mt=mt)


def test_layout_and_binding(tmp_path):
    """3. sizeof / offsetof of rt_gbuffer as gcc lays include/rt_api.h out, against the ctypes
    structure; both entry points in RT_SYMBOLS, bound with an int result."""
    fields = ("shape", "shape_pitch", "depth", "depth_pitch", "normal", "normal_pitch", "position", "position_pitch")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_api.h"\n'
                   'int main(void) { printf("%zu", sizeof(rt_gbuffer));\n'
                   + "".join(f'printf(" %zu", offsetof(rt_gbuffer, {f}));\n' for f in fields)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    g = rtamd.rt_gbuffer
    assert got == [64, 0, 8, 16, 24, 32, 40, 48, 56]
    assert got == [C.sizeof(g)] + [getattr(g, f).offset for f in fields]
    assert [n for n, _ in g._fields_] == list(fields)
    assert all(C.sizeof(t) == 8 for _, t in g._fields_)
    lib = rtamd.rt_lib()
    for name in ("rt_dispatch_gbuffer", "rt_gbuffer_host"):
        assert name in rtamd.RT_SYMBOLS and getattr(lib, name).restype is C.c_int
    assert rtamd.GBUFFER_PLANES == gr.PLANES


def test_row_mapping():
    """4. gbuffer_ref's rows against rt_device.h's image_row: y0 + r + (r / stripe) * (period - stripe)."""
    for y0, stripe, period, out_rows in ((0, 1, 1, 54), (8, 8, 24, 24), (0, 3, 7, 24), (16, 8, 16, 20), (5, 2, 2, 9),
                                         (53, 1, 1, 3)):
        for r in range(out_rows):
            assert gr.image_row(r, y0, stripe, period) == y0 + r + (r // stripe) * (period - stripe)
        rows = gr.dispatch_rows(54, y0, stripe, period, out_rows)
        assert all(y < 54 for _, y in rows) and len({y for _, y in rows}) == len(rows)
        assert [r for r, _ in rows] == [r for r in range(out_rows) if gr.image_row(r, y0, stripe, period) < 54]
    assert gr.dispatch_rows(54, 16, 8, 16, 20) == [(r, 16 + r) for r in range(8)] + [(r, 24 + r) for r in range(8, 16)] \
        + [(r, 32 + r) for r in range(16, 20)]
    assert [y for _, y in gr.dispatch_rows(54, 8, 8, 24, 24)] == list(range(8, 16)) + list(range(32, 40))
