"""Ray queries (rt_trace_rays), the parts that need no GPU.

The ray sets tests/test_gpu_trace.py sends to the device (tests/trace_rays.py) are first
walked here by the scalar emulation of the accelerated walk (tests/native/accel_check.cpp)
and by the oracle's reference walk (orc_trace_rays_mt): same shape, same distance bit for
bit, same shadow answer for every ray, barycentric and Moller-Trumbore, over the scene tree
and over the reference tree. So a mismatch on the device is the device's, not an input
outside what the accelerator is built for. This guards the inputs and passes without the
feature; the layout test and tests/test_abi.py::test_exports need it.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtamd
import trace_rays as tr
from test_accel_cpu import check_lib, compare  # noqa: F401  (check_lib: the emulation's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mt", [0, 1])
@pytest.mark.parametrize("name", tr.SCENES)
def test_ray_sets_are_exact_on_the_cpu(check_lib, name, mt):
    fs = tr.scene(name)
    sets = tr.ray_sets(name)
    want = {"camera": tr.CAM_W * tr.CAM_H, "random": tr.N_RANDOM, "axis": tr.N_AXIS, "far": tr.N_FAR,
            "scaled": tr.N_SCALED}
    if (fs.shapes["type"] == 3).any():
        want["grazing"] = tr.N_GRAZING
    assert {k: len(o) for k, (o, d) in sets.items()} == want
    o, d, lim = tr.all_rays(name)
    assert len(o) == sum(want.values()) and o.dtype == d.dtype == lim.dtype == np.float32
    for tree in (1, 0):
        compare(check_lib, fs, o, d, lim, tree, mt=mt)  # asserts shape, distance bits and shadow, every ray
    # the oracle answers the GPU tests compare with are those the emulation was checked against
    shape, dist, shadow = tr.oracle_all(name, mt)
    assert (shape >= 0).sum() > len(o) // 10 and 0 < shadow.sum() < (shape >= 0).sum()


def test_record_layouts(tmp_path):
    """sizeof / offsetof of rt_ray and rt_hit as a C compiler lays include/rt_api.h out,
    against RAY_DTYPE and HIT_DTYPE."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_api.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_ray), '
                   'offsetof(rt_ray, origin), offsetof(rt_ray, limit), offsetof(rt_ray, dir), '
                   'offsetof(rt_ray, reserved), sizeof(rt_hit), offsetof(rt_hit, shape), '
                   'offsetof(rt_hit, distance), offsetof(rt_hit, occluded), offsetof(rt_hit, reserved)); '
                   'printf("%d %d\\n", RT_TRACE_CLOSEST, RT_TRACE_ANY); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in out]
    r, h = rtamd.RAY_DTYPE, rtamd.HIT_DTYPE
    assert got[:5] == [32, 0, 12, 16, 28]
    assert got[:5] == [r.itemsize] + [r.fields[f][1] for f in ("origin", "limit", "dir", "reserved")]
    assert got[5:10] == [16, 0, 4, 8, 12]
    assert got[5:10] == [h.itemsize] + [h.fields[f][1] for f in ("shape", "distance", "occluded", "reserved")]
    assert got[10:] == [rtamd.TRACE_CLOSEST, rtamd.TRACE_ANY]
    assert r.fields["origin"][0] == r.fields["dir"][0] == np.dtype(("<f4", 3))
    assert [h.fields[f][0] for f in ("shape", "distance", "occluded")] == [np.dtype("<i4"), np.dtype("<f4"),
                                                                           np.dtype("<i4")]


def test_query_entry_points_are_bound():
    lib = rtamd.rt_lib()
    for name in ("rt_trace_rays", "rt_trace_rays_host", "rt_trace_pixels"):
        assert name in rtamd.RT_SYMBOLS and getattr(lib, name).restype is C.c_int
    rays = rtamd.ComputeShader.make_rays(np.zeros((3, 3)), np.ones((3, 3)), [1.0, 2.0, 3.0])
    assert rays.dtype == rtamd.RAY_DTYPE and rays.nbytes == 96 and np.array_equal(rays["limit"], [1, 2, 3])
    assert np.isinf(rtamd.ComputeShader.make_rays(np.zeros(3), np.ones(3))["limit"]).all()
