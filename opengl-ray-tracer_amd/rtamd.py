"""rtamd — Python host binding of the MI355X ray tracer.

Thin ctypes layer over the two product libraries built in-tree by
``opengl-ray-tracer_amd/Makefile``:

* ``lib/librtamd.so``  — the HIP renderer, C ABI ``include/rt_api.h``: the drop-in
  for the reference's compute-shader dispatch (``src/computeShader.hpp``,
  ``src/main.cpp:238-370``).
* ``lib/librtscene.so`` — the host scene library, C ABI ``include/rt_scene.h``:
  shapes, ``buildBVH``/``split``, ``serializeScene`` (``src/main.cpp:806-1193``).

Class and method names mirror the reference (``Scene.buildBVH``,
``Scene.serializeScene``, ``ComputeShader.dispatch`` ...). Loading fails loudly:
there is no CPU fallback anywhere in this module.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RTAMD_LIBDIR: another build's directory (librtamd.so, librtscene.so, librthost.so), for
# A/B profiling of build variants (tools/build_var.sh); the default is the in-tree lib/
LIBDIR = os.environ.get("RTAMD_LIBDIR") or os.path.join(HERE, "lib")

# ---------------------------------------------------------------------------
# Record layouts (include/rt_flat.h; sizes pinned by static asserts there).

def _vec(off):
    return [("x", off), ("y", off + 4), ("z", off + 8)]


MATERIAL_DTYPE = np.dtype({
    "names": ["color", "fresnelStrength", "ambientStrength", "diffuseStrength", "specularStrength", "shininess"],
    "formats": [("<f4", 3), "<f4", "<f4", "<f4", "<f4", "<i4"],
    "offsets": [0, 12, 16, 20, 24, 28],
    "itemsize": 32,
})

SHAPE_DTYPE = np.dtype({
    "names": ["type", "material", "sphereCenter", "sphereRadius", "planeNormal", "planeD",
              "wallStart", "wallWidth", "wallHeight", "triP1", "triP2", "triP3"],
    "formats": ["<i4", MATERIAL_DTYPE, ("<f4", 3), "<f4", ("<f4", 3), "<f4",
                ("<f4", 3), "<f4", "<f4", ("<f4", 3), ("<f4", 3), ("<f4", 3)],
    "offsets": [0, 32, 64, 76, 80, 92, 96, 108, 112, 144, 160, 176],
    "itemsize": 192,
})

NODE_DTYPE = np.dtype({
    "names": ["boundsMin", "boundsMax", "leftChild", "rightChild", "startShapeIdx", "numShapes"],
    "formats": [("<f4", 3), ("<f4", 3), "<i4", "<i4", "<i4", "<i4"],
    "offsets": [0, 16, 32, 36, 40, 44],
    "itemsize": 48,
})

CAMERA_DTYPE = np.dtype({
    "names": ["Position", "aspectRatio", "Front", "Up", "Right", "fov"],
    "formats": [("<f4", 3), "<f4", ("<f4", 3), ("<f4", 3), ("<f4", 3), "<f4"],
    "offsets": [0, 12, 16, 32, 48, 64],
    "itemsize": 80,
})

LIGHT_DTYPE = np.dtype({
    "names": ["position", "color"],
    "formats": [("<f4", 3), ("<f4", 3)],
    "offsets": [0, 16],
    "itemsize": 32,
})

# rt_ray / rt_hit (include/rt_api.h): the records of the ray queries
RAY_DTYPE = np.dtype({
    "names": ["origin", "limit", "dir", "reserved"],
    "formats": [("<f4", 3), "<f4", ("<f4", 3), "<i4"],
    "offsets": [0, 12, 16, 28],
    "itemsize": 32,
})

HIT_DTYPE = np.dtype({
    "names": ["shape", "distance", "occluded", "reserved"],
    "formats": ["<i4", "<f4", "<i4", "<i4"],
    "offsets": [0, 4, 8, 12],
    "itemsize": 16,
})

# rt_view_ray (include/rt_api.h): the records of rt_shade_rays / rt_camera_rays
VIEW_RAY_DTYPE = np.dtype({
    "names": ["origin", "sky", "dir", "reserved"],
    "formats": [("<f4", 3), "<f4", ("<f4", 3), "<i4"],
    "offsets": [0, 12, 16, 28],
    "itemsize": 32,
})

SPHERE, PLANE, WALL, TRIANGLE = 0, 1, 2, 3
TRACE_CLOSEST, TRACE_ANY = 0, 1
KERNEL_AUTO, KERNEL_LANE, KERNEL_PACKET, KERNEL_ACCEL = 0, 1, 2, 3
KERNEL_LIGHTS = 4  # reported by accel_info()["last_kernel"] only: a frame of two or more lights (set_lights)
MAX_LIGHTS = 8     # RT_MAX_LIGHTS
KERNEL_SOFT = 5    # reported by accel_info()["last_kernel"] only: a frame of area lights (set_soft_shadows)
MAX_SHADOW_SAMPLES = 64  # RT_MAX_SHADOW_SAMPLES
SCHED_ROWS, SCHED_COST, SCHED_COST_XCD = 0, 1, 2
TREE_REFERENCE, TREE_SCENE = 0, 1


class rt_params(C.Structure):
    """Uniforms of gpu_shader.comp:126-130."""
    _fields_ = [("resX", C.c_float), ("resY", C.c_float), ("maxBounces", C.c_int), ("useBVH", C.c_int),
                ("useFresnel", C.c_int), ("useMollerTrumbore", C.c_int)]


class rt_gbuffer(C.Structure):
    """The planes of a geometry buffer (include/rt_api.h): pointer and pitch in bytes each,
    a null pointer = plane not wanted."""
    _fields_ = [("shape", C.c_void_p), ("shape_pitch", C.c_size_t), ("depth", C.c_void_p), ("depth_pitch", C.c_size_t),
                ("normal", C.c_void_p), ("normal_pitch", C.c_size_t), ("position", C.c_void_p),
                ("position_pitch", C.c_size_t)]


GBUFFER_PLANES = ("shape", "depth", "normal", "position")


class rt_ao_params(C.Structure):
    """rt_dispatch_ao's parameters (include/rt_api.h): rays 1..64, radius > 0 (may be inf),
    bias >= 0, reserved 0."""
    _fields_ = [("rays", C.c_int), ("radius", C.c_float), ("bias", C.c_float), ("reserved", C.c_int)]


class rt_ao(C.Structure):
    """The planes of an ambient-occlusion dispatch: pointer and pitch in bytes each, a null
    pointer = plane not wanted."""
    _fields_ = [("count", C.c_void_p), ("count_pitch", C.c_size_t), ("visibility", C.c_void_p),
                ("visibility_pitch", C.c_size_t)]


AO_PLANES = ("count", "visibility")


class rt_accel_info(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("built", "local_nodes", "local_leaves", "bounded_prims", "always_prims",
                                       "max_stack", "last_kernel", "scene_tree", "scene_nodes", "scene_items",
                                       "scene_height", "tree_nested", "record_bytes")]


class rt_stats(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("node_visits", C.c_uint64), ("bvh_tests", C.c_uint64 * 4), ("brute_tests", C.c_uint64 * 4),
                ("closest_updates", C.c_uint64), ("hits", C.c_uint64)]

    def as_dict(self):
        return {"pixels": self.pixels, "closest_rays": self.closest_rays, "shadow_rays": self.shadow_rays,
                "node_visits": self.node_visits, "bvh_tests": list(self.bvh_tests),
                "brute_tests": list(self.brute_tests), "closest_updates": self.closest_updates, "hits": self.hits}


# Bytes of the reference's records that a test of each shape type reads
# (SURVEY §8(d)): 4 B type tag + sphere 16 | plane 16 | wall 36 | triangle 52 (36 for MT).
P_TYPE = {0: 4 + 16, 1: 4 + 16, 2: 4 + 36, 3: 4 + 52}
P_TYPE_MT = {0: 4 + 16, 1: 4 + 16, 2: 4 + 36, 3: 4 + 36}


def algorithmic_bytes(st: dict, pixels_written: int, use_mt: bool = False) -> int:
    """B_alg of SURVEY §8(d): 40 B per node visit, (4 B index + record bytes) per
    BVH leaf test, record bytes per brute-force test, 32 B material per closest
    update, 16 B per RGBA32F pixel store."""
    p = P_TYPE_MT if use_mt else P_TYPE
    b = 40 * st["node_visits"] + 32 * st["closest_updates"] + 16 * pixels_written
    b += sum((4 + p[t]) * n for t, n in enumerate(st["bvh_tests"]))
    b += sum(p[t] * n for t, n in enumerate(st["brute_tests"]))
    return int(b)


STATUS = {0: "ok", -1: "invalid argument", -2: "HIP runtime error", -3: "device allocation failed",
          -4: "scene, camera or light not uploaded", -5: "node/index arrays out of range or deeper than the 64-entry stack",
          -6: "no such HIP device", -7: "RCCL call failed (the group's communicator is aborted)",
          -8: "timed out waiting for a group's frames (the communicator is aborted)"}


class RTError(RuntimeError):
    def __init__(self, what, code):
        super().__init__(f"{what} failed: {STATUS.get(code, code)} ({code})")
        self.code = code


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def as_records(a, dtype):
    """Contiguous array with exactly the C record layout. numpy may pack a
    padded structured dtype (np.concatenate does), which would hand the C side
    records of the wrong size."""
    a = np.asarray(a)
    if a.dtype != dtype:
        a = a.astype(dtype)
    return np.ascontiguousarray(a)


_P = C.c_void_p
_I = C.c_int


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C opengl-ray-tracer_amd` "
                           f"(or __graft_entry__.build()); there is no fallback path")
    return C.CDLL(path)


_scene_lib = None
_rt_lib = None

SCENE_SYMBOLS = {
    "rts_new": (_P, []), "rts_free": (None, [_P]), "rts_clear": (_I, [_P]),
    "rts_add_sphere": (_I, [_P, _P, C.c_float, _P]),
    "rts_add_plane": (_I, [_P, _P, _P, _P]),
    "rts_add_wall": (_I, [_P, _P, C.c_float, C.c_float, _P, _P]),
    "rts_add_triangle": (_I, [_P, _P, _P, _P, _I, _P]),
    "rts_add_mesh": (_I, [_P, _P, _I, _P, _I, _P, _P]),
    "rts_add_mesh_oriented": (_I, [_P, _P, _I, _P, _I, _P, _P]),
    "rts_set_camera": (_I, [_P, _P, C.c_float, C.c_float]),
    "rts_camera_look_at": (_I, [_P, _P]),
    "rts_set_light": (_I, [_P, _P, _P, C.c_float]),
    "rts_build_bvh": (_I, [_P, _I]),
    "rts_counts": (_I, [_P, _P, _P, _P]),
    "rts_serialize": (_I, [_P, _P, _P, _P, _P, _P]),
    "rts_bvh_stats": (_I, [_P, _P, _P, _P, _P]),
    "rts_generate": (_I, [_P, _I, _I, C.c_float]),
    "rts_load_obj": (_I, [_P, C.c_char_p, _P, _P, _I]),
    "rts_parse_obj": (_I, [_P, C.c_char_p, C.c_long, _P, _P, _I]),
    "rts_write_image": (_I, [C.c_char_p, _P, _I, _I, C.c_long, _I]),
    "rts_update_bvh": (_I, [_P, _I, _P, _I, _P, _I, _P, _I]),
}

# include/rt_host.h (librthost.so: the reference's render loop as a C++ host)
HOST_SYMBOLS = {
    "rth_render_loop": (_I, [_P, _P, _I, _P, _I, _I, _P, C.c_size_t, _I, _I, _P]),
    "rth_render_loop_anim": (_I, [_P, _P, _I, _P, _I, _I, _P, C.c_size_t, _I, _I, _P, _I, _I, _P]),
    "rth_upload_animated": (_I, [_P, _P, _I, _P, _P, _I, _P, _I, _P, _I]),
    "rth_group_upload_animated": (_I, [_P, _P, _I, _P, _P, _I, _P, _I, _P, _I]),
    "rth_render_rows_loop": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _I, _I, _P]),
    "rth_render_loop_ref": (_I, [_P, _P, _I, _P, _I, _I, _P, C.c_size_t, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I,
                                 _P, _I, _P]),
}

RT_SYMBOLS = {
    "rt_create": (_I, [_P, _I]), "rt_destroy": (_I, [_P]), "rt_set_stream": (_I, [_P, _P]),
    "rt_upload_scene": (_I, [_P, _P, _I, _P, _I, _P, _I]),
    "rt_update_shapes": (_I, [_P, _I, _I, _P]),
    "rt_update_nodes": (_I, [_P, _P, _I]),
    "rt_set_animated": (_I, [_P, _P, _I]), "rt_animate": (_I, [_P, _P]),
    "rt_read_nodes": (_I, [_P, _P, _I]),
    "rt_set_camera": (_I, [_P, _P]), "rt_set_light": (_I, [_P, _P]),
    "rt_set_lights": (_I, [_P, _P, _I]), "rt_get_lights": (_I, [_P, _P, _I, _P]),
    "rt_set_soft_shadows": (_I, [_P, _P, _I, _I]), "rt_get_soft_shadows": (_I, [_P, _P, _I, _P, _P]),
    "rt_set_params": (_I, [_P, _P]), "rt_set_kernel": (_I, [_P, _I]),
    "rt_dispatch": (_I, [_P, _I, _I, _I, _I]),
    "rt_dispatch_rows": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t]),
    "rt_dispatch_rows_fmt": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _I]),
    "rt_dispatch_rows_ex": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _I]),
    "rt_sync": (_I, [_P]), "rt_sync_frame": (_I, [_P]), "rt_read_image": (_I, [_P, _P, C.c_size_t, _I, _I]),
    "rt_device_image": (_I, [_P, _P, _P]),
    "rt_set_surface_format": (_I, [_P, _I]), "rt_surface_format": (_I, [_P, _P]),
    "rt_read_surface": (_I, [_P, _P, C.c_size_t, _I, _I]),
    "rt_srgb_thresholds": (_I, [_P]),
    "rt_collect_stats": (_I, [_P, _I, _I, _I, _I, _I, _I, _P]),
    "rt_collect_stats_ex": (_I, [_P, _I, _I, _I, _I, _I, _I, _P]),
    "rt_last_kernel_ms": (_I, [_P, _P]),
    "rt_kernel_times": (_I, [_P, _P, _I]),
    "rt_accel_info_get": (_I, [_P, _P]),
    "rt_set_walk": (_I, [_P, _I]),
    "rt_set_tree": (_I, [_P, _I]),
    "rt_build_lbvh": (_I, [_P, _P]),
    "rt_scene_size": (_I, [_P, _P, _P, _P]),
    "rt_read_indices": (_I, [_P, _P, _I]),
    "rt_set_schedule": (_I, [_P, _I]),
    "rt_set_latency_mode": (_I, [_P, _I]),
    "rt_set_kernel_timing": (_I, [_P, _I]),
    "rt_set_tail": (_I, [_P, _I]),
    "rt_set_samples": (_I, [_P, _I]),
    "rt_set_adaptive": (_I, [_P, C.c_float]),
    "rt_adaptive_stats": (_I, [_P, _P, _P]),
    "rt_trace_rays": (_I, [_P, _P, _I, _P, _I]),
    "rt_trace_rays_host": (_I, [_P, _P, _I, _P, _I]),
    "rt_trace_pixels": (_I, [_P, _I, _I, _P, _I, _P]),
    "rt_dispatch_gbuffer": (_I, [_P, _I, _I, _I, _I, _I, _I, _P]),
    "rt_gbuffer_host": (_I, [_P, _I, _I, _P]),
    "rt_dispatch_ao": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "rt_ao_host": (_I, [_P, _I, _I, _P, _P]),
    "rt_ao_table": (_I, [_P, _P]),
    "rt_shade_rays": (_I, [_P, _P, _I, _P, _I]),
    "rt_shade_rays_host": (_I, [_P, _P, _I, _P, _I]),
    "rt_camera_rays": (_I, [_P, _I, _I, _I, _I, _P]),
    "rt_camera_rays_host": (_I, [_P, _I, _I, _I, _I, _P]),
    "rt_status_string": (C.c_char_p, [_I]),
}

# include/rt_group.h (also in librtamd.so)
GROUP_SYMBOLS = {
    "rt_group_unique_id": (_I, [_P, C.c_size_t]),
    "rt_group_create": (_I, [_P, _P, _I, _I]),
    "rt_group_create_rank": (_I, [_P, _P, _I, _I, _I]),
    "rt_group_destroy": (_I, [_P]),
    "rt_group_info": (_I, [_P, _P, _P, _P]),
    "rt_group_member": (_I, [_P, _I, _P]),
    "rt_group_member_slot": (_I, [_P, _I, _I, _P]),
    "rt_group_set_frames": (_I, [_P, _I]),
    "rt_group_frames": (_I, [_P]),
    "rt_group_set_timeout": (_I, [_P, C.c_double]),
    "rt_group_set_phase_timing": (_I, [_P, _I]),
    "rt_group_set_sky_rows": (_I, [_P, _I]),
    "rt_group_sky_band": (_I, [_P, _P, _P]),
    "rt_group_check": (_I, [_P]),
    "rt_group_phase_times": (_I, [_P, _P]),
    "rt_group_upload_scene": (_I, [_P, _P, _I, _P, _I, _P, _I]),
    "rt_group_set_camera": (_I, [_P, _P]), "rt_group_set_light": (_I, [_P, _P]),
    "rt_group_set_params": (_I, [_P, _P]),
    "rt_group_update_shapes": (_I, [_P, _I, _I, _P]),
    "rt_group_update_nodes": (_I, [_P, _P, _I]),
    "rt_group_set_animated": (_I, [_P, _P, _I]), "rt_group_animate": (_I, [_P, _P]),
    "rt_group_dispatch": (_I, [_P, _I, _I, _I]),
    "rt_group_set_root_share": (_I, [_P, _I]),
    "rt_group_collect_stats": (_I, [_P, _I, _I, _I, _P]),
    "rt_group_sync": (_I, [_P]),
    "rt_group_read_image": (_I, [_P, _P, C.c_size_t, _I, _I]),
    "rt_group_device_image": (_I, [_P, _P, _P]),
}
GATHER_AUTO, GATHER_RCCL, GATHER_COPY = 0, 1, 2
FORMAT_RGBA32F, FORMAT_RGB32F, FORMAT_RGBA32F_IMAGE = 0, 1, 2  # rt_format
FORMAT_RGBA8, FORMAT_SRGBA8, FORMAT_RGBA16F = 3, 4, 5  # rt_format: the display formats
# bytes per pixel and the numpy type of one channel, for the formats a context surface can have
SURFACE_DTYPE = {FORMAT_RGBA32F: np.float32, FORMAT_RGBA8: np.uint8, FORMAT_SRGBA8: np.uint8,
                 FORMAT_RGBA16F: np.float16}
GROUP_ID_BYTES = 128


def _bind(lib, table, partial=False):
    """partial: skip symbols the library lacks (an older build compared by tools/ab.py)."""
    for name, (res, args) in table.items():
        if partial and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def scene_lib():
    global _scene_lib
    if _scene_lib is None:
        _scene_lib = _bind(_load("librtscene.so"), SCENE_SYMBOLS)
    return _scene_lib


def rt_lib():
    global _rt_lib
    if _rt_lib is None:
        _rt_lib = _bind(_bind(_load("librtamd.so"), RT_SYMBOLS), GROUP_SYMBOLS)
    return _rt_lib


def ao_table():
    """rt_ao_table: the tables that define rt_dispatch_ao's rays, (D [64, 3], ROT [16, 2]) float32.
    Needs no device."""
    d, rot = np.zeros((64, 3), np.float32), np.zeros((16, 2), np.float32)
    rc = rt_lib().rt_ao_table(_ptr(d), _ptr(rot))
    if rc != 0:
        raise RTError("rt_ao_table", rc)
    return d, rot


_host_lib = None


def host_lib():
    """librthost.so: rth_render_loop, the reference's render loop (src/main.cpp:290-462)
    as a C++ host over the C ABI (include/rt_host.h)."""
    global _host_lib
    if _host_lib is None:
        rt_lib()  # librtamd.so first: librthost.so links it
        _host_lib = _bind(_load("librthost.so"), HOST_SYMBOLS)
    return _host_lib


def update_bvh(fs, ids):
    """updateBVH (src/main.cpp:1068-1077) on the scene's arrays in place (librtscene.so
    rts_update_bvh): every node listing one of the shapes `ids` grows to hold its
    current record in fs.shapes."""
    ids = np.ascontiguousarray(ids, np.int32)
    rc = scene_lib().rts_update_bvh(_ptr(fs.shapes), len(fs.shapes), _ptr(fs.nodes), len(fs.nodes),
                                    _ptr(fs.indices), len(fs.indices), _ptr(ids), len(ids))
    if rc != 0:
        raise RTError("rts_update_bvh", rc)


class ReferenceUpload:
    """A host that keeps the reference's own per-frame upload of an animated scene
    (src/main.cpp:336-346): its own copies of the shape and node arrays, moved
    frame by frame; upload() is one rth_upload_animated (librthost.so): one
    rt_update_shapes per animated index, updateBVH on the host's nodes, one
    rt_update_nodes."""

    def __init__(self, fs, ids):
        self.shapes = as_records(fs.shapes, SHAPE_DTYPE).copy()
        self.nodes = as_records(fs.nodes, NODE_DTYPE).copy()
        self.indices = np.ascontiguousarray(fs.indices, np.int32)
        self.ids = np.ascontiguousarray(ids, np.int32)

    def upload(self, ctx, recs):
        """ctx: a ComputeShader (rth_upload_animated) or a Group (rth_group_upload_animated:
        every member and frame slot is given the calls)."""
        recs = as_records(np.asarray(recs).reshape(-1), SHAPE_DTYPE)
        fn = host_lib().rth_group_upload_animated if isinstance(ctx, Group) else host_lib().rth_upload_animated
        rc = fn(ctx._h, _ptr(self.shapes), len(self.shapes), _ptr(self.ids), _ptr(recs), len(self.ids),
                _ptr(self.nodes), len(self.nodes), _ptr(self.indices), len(self.indices))
        if rc != 0:
            raise RTError("rth_group_upload_animated" if isinstance(ctx, Group) else "rth_upload_animated", rc)

    def scene(self, fs):
        """The scene this host has uploaded (for the oracle)."""
        return FlatScene(self.shapes.copy(), self.nodes.copy(), self.indices, fs.camera, fs.light)


def render_loop(ctx, cams, light, width, height, dst_ptr, pitch, frames, wait_each=True, anim=None, ref=None):
    """rth_render_loop(_anim / _ref) on ComputeShader `ctx`: `frames` frames (camera cams[i % len]),
    each waited for (wait_each) or back to back; anim: a list of per-frame record
    arrays of the animated shapes, frame i animated with anim[i % len] first -- by
    rt_animate, or with `ref` (a ReferenceUpload) by the reference's own upload.
    Returns the host wall times in ms: one per frame, or [total] when not waiting."""
    cams = as_records(np.asarray(cams), CAMERA_DTYPE).reshape(-1)
    light = as_records(np.asarray(light), LIGHT_DTYPE).reshape(1)
    out = np.zeros(max(1, frames), np.float64)
    if ref is not None:
        recs = as_records(np.concatenate([np.asarray(f).reshape(-1) for f in anim]), SHAPE_DTYPE)
        rc = host_lib().rth_render_loop_ref(ctx._h, _ptr(cams), len(cams), _ptr(light), int(width), int(height),
                                            C.c_void_p(dst_ptr), int(pitch), int(frames), int(bool(wait_each)),
                                            _ptr(ref.shapes), len(ref.shapes), _ptr(ref.ids), len(ref.ids), _ptr(recs),
                                            len(anim), _ptr(ref.nodes), len(ref.nodes), _ptr(ref.indices),
                                            len(ref.indices), _ptr(out))
    elif anim is not None:
        recs = as_records(np.concatenate([np.asarray(f).reshape(-1) for f in anim]), SHAPE_DTYPE)
        per = len(np.asarray(anim[0]).reshape(-1))
        rc = host_lib().rth_render_loop_anim(ctx._h, _ptr(cams), len(cams), _ptr(light), int(width), int(height),
                                             C.c_void_p(dst_ptr), int(pitch), int(frames), int(bool(wait_each)),
                                             _ptr(recs), per, len(anim), _ptr(out))
    else:
        rc = host_lib().rth_render_loop(ctx._h, _ptr(cams), len(cams), _ptr(light), int(width), int(height),
                                        C.c_void_p(dst_ptr), int(pitch), int(frames), int(bool(wait_each)),
                                        _ptr(out))
    if rc != 0:
        raise RTError("rth_render_loop", rc)
    return out if wait_each else out[:1]


def render_rows_loop(ctx, cams, light, width, height, y0, stripe, period, out_rows, dst_ptr, pitch, frames,
                     wait_each=True, fmt=FORMAT_RGB32F):
    """rth_render_rows_loop: rth_render_loop over one rank's rows (rt_dispatch_rows_ex).
    Returns the host wall times in ms: one per frame, or [total] when not waiting."""
    cams = as_records(np.asarray(cams), CAMERA_DTYPE).reshape(-1)
    light = as_records(np.asarray(light), LIGHT_DTYPE).reshape(1)
    out = np.zeros(max(1, frames), np.float64)
    rc = host_lib().rth_render_rows_loop(ctx._h, _ptr(cams), len(cams), _ptr(light), int(width), int(height), int(y0),
                                         int(stripe), int(period), int(out_rows), int(fmt), C.c_void_p(dst_ptr),
                                         int(pitch), int(frames), int(bool(wait_each)), _ptr(out))
    if rc != 0:
        raise RTError("rth_render_rows_loop", rc)
    return out if wait_each else out[:1]


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def material(color=(1, 1, 1), fresnel=1.0, ambient=0.4, diffuse=1.0, specular=0.5, shininess=32):
    """Material(c, fresnel, ambient, diffuse, specular, shine) (src/material.hpp:23)."""
    m = np.zeros(1, MATERIAL_DTYPE)
    m["color"] = color
    m["fresnelStrength"] = fresnel
    m["ambientStrength"] = ambient
    m["diffuseStrength"] = diffuse
    m["specularStrength"] = specular
    m["shininess"] = shininess
    return m


# ---------------------------------------------------------------------------
@dataclass
class FlatScene:
    """serializeScene output: the five SSBO images (src/flatStructures.hpp:80-108)."""
    shapes: np.ndarray
    nodes: np.ndarray
    indices: np.ndarray
    camera: np.ndarray
    light: np.ndarray

    def __post_init__(self):
        self.shapes = as_records(self.shapes, SHAPE_DTYPE)
        self.nodes = as_records(self.nodes, NODE_DTYPE)
        self.indices = np.ascontiguousarray(self.indices, np.int32)
        self.camera = as_records(self.camera, CAMERA_DTYPE).reshape(1)
        self.light = as_records(self.light, LIGHT_DTYPE).reshape(1)


class Scene:
    """The reference's `Scene` (src/main.cpp:92-100) on the host scene library."""

    def __init__(self):
        self._lib = scene_lib()
        self._h = self._lib.rts_new()
        if not self._h:
            raise MemoryError("rts_new")

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.rts_free(self._h)
            self._h = None

    def _chk(self, rc, what):
        if rc < 0:
            raise RTError(what, rc)
        return rc

    @staticmethod
    def _mat(m):
        return _ptr(m) if m is not None else None

    def add_sphere(self, center, radius, mat=None):
        return self._chk(self._lib.rts_add_sphere(self._h, _f3(center), radius, self._mat(mat)), "add_sphere")

    def add_plane(self, normal, point, mat=None):
        return self._chk(self._lib.rts_add_plane(self._h, _f3(normal), _f3(point), self._mat(mat)), "add_plane")

    def add_wall(self, start, width, height, normal, mat=None):
        return self._chk(self._lib.rts_add_wall(self._h, _f3(start), width, height, _f3(normal), self._mat(mat)),
                         "add_wall")

    def add_triangle(self, a, b, c, invert=False, mat=None):
        return self._chk(self._lib.rts_add_triangle(self._h, _f3(a), _f3(b), _f3(c), int(invert), self._mat(mat)),
                         "add_triangle")

    def add_mesh(self, vertices, indices, origin=(0, 0, 0), mat=None, oriented=False):
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        fn = self._lib.rts_add_mesh_oriented if oriented else self._lib.rts_add_mesh
        return self._chk(fn(self._h, _ptr(v), len(v), _ptr(i), len(i), _f3(origin), self._mat(mat)), "add_mesh")

    def load_obj(self, path, origin=(0, 0, 0), mat=None, oriented=False):
        """Wavefront OBJ file -> triangles (rts_load_obj); returns the triangle count."""
        return self._chk(self._lib.rts_load_obj(self._h, os.fsencode(path), _f3(origin), self._mat(mat),
                                                int(bool(oriented))), "load_obj")

    def parse_obj(self, text, origin=(0, 0, 0), mat=None, oriented=False):
        b = text.encode() if isinstance(text, str) else bytes(text)
        return self._chk(self._lib.rts_parse_obj(self._h, b, len(b), _f3(origin), self._mat(mat),
                                                 int(bool(oriented))), "parse_obj")

    def set_camera(self, position, fov=60.0, aspect=1.0):
        self._chk(self._lib.rts_set_camera(self._h, _f3(position), fov, aspect), "set_camera")

    def LookAt(self, target):
        self._chk(self._lib.rts_camera_look_at(self._h, _f3(target)), "LookAt")

    def set_light(self, position, color=(1, 1, 1), intensity=1.0):
        self._chk(self._lib.rts_set_light(self._h, _f3(position), _f3(color), intensity), "set_light")

    def camera(self):
        """serializeCamera (src/main.cpp:806-816) alone."""
        cam = np.zeros(1, CAMERA_DTYPE)
        self._chk(self._lib.rts_serialize(self._h, None, None, None, _ptr(cam), None), "serializeCamera")
        return cam

    def orbit(self, target, degrees):
        """Turn the camera `degrees` about the vertical axis through `target` and
        look at `target` again (the weak bench mode's per-rank frames of an orbit).
        The rotation is done in float64 on the serialised position."""
        cam = self.camera()
        p = cam["Position"][0].astype(np.float64) - np.asarray(target, np.float64)
        ang = np.radians(float(degrees))
        q = (p[0] * np.cos(ang) + p[2] * np.sin(ang), p[1], -p[0] * np.sin(ang) + p[2] * np.cos(ang))
        self.set_camera(np.asarray(q) + np.asarray(target, np.float64), float(cam["fov"][0]),
                        float(cam["aspectRatio"][0]))
        self.LookAt(target)

    def buildBVH(self, maxDepth=15):
        self._chk(self._lib.rts_build_bvh(self._h, maxDepth), "buildBVH")

    def generate(self, config, variant=0, aspect=16 / 9):
        self._chk(self._lib.rts_generate(self._h, config, variant, aspect), "generate")
        return self

    def counts(self):
        s, n, i = C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.rts_counts(self._h, C.byref(s), C.byref(n), C.byref(i)), "counts")
        return s.value, n.value, i.value

    def bvh_stats(self):
        v = [C.c_int() for _ in range(4)]
        self._chk(self._lib.rts_bvh_stats(self._h, *[C.byref(x) for x in v]), "bvh_stats")
        return dict(zip(["leaves", "max_leaf", "depth", "max_stack"], [x.value for x in v]))

    def serializeScene(self) -> FlatScene:
        s, n, i = self.counts()
        shapes = np.zeros(s, SHAPE_DTYPE)
        nodes = np.zeros(n, NODE_DTYPE)
        idx = np.zeros(i, np.int32)
        cam = np.zeros(1, CAMERA_DTYPE)
        light = np.zeros(1, LIGHT_DTYPE)
        self._chk(self._lib.rts_serialize(self._h, _ptr(shapes), _ptr(nodes), _ptr(idx), _ptr(cam), _ptr(light)),
                  "serializeScene")
        return FlatScene(shapes, nodes, idx, cam, light)


IMAGE_PPM, IMAGE_PFM = 0, 1


def write_image(path, img, fmt=IMAGE_PPM):
    """[H, W, 4] float32 image (row 0 = NDC y +1) -> binary PPM (clamped, 8-bit) or PFM (exact)."""
    a = np.ascontiguousarray(img, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("write_image expects [H, W, 4] float32")
    rc = scene_lib().rts_write_image(os.fsencode(path), _ptr(a), a.shape[1], a.shape[0], a.shape[1] * 16, int(fmt))
    if rc != 0:
        raise RTError("rts_write_image", rc)


def srgb_thresholds():
    """rt_srgb_thresholds: the 255 float32 thresholds T[1..255] that define FORMAT_SRGBA8
    (result[k - 1] = T[k]): a channel c encodes to the count of k with clamp(c, 0, 1) >= T[k]."""
    out = np.zeros(255, np.float32)
    rc = rt_lib().rt_srgb_thresholds(_ptr(out))
    if rc != 0:
        raise RTError("rt_srgb_thresholds", rc)
    return out


def generate(config, variant=0, width=1920, height=1080) -> FlatScene:
    """One of the BASELINE configurations as serialised arrays."""
    sc = Scene().generate(config, variant, float(width) / float(height))
    return sc.serializeScene()


# ---------------------------------------------------------------------------
class ComputeShader:
    """The GPU operator: ComputeShader("gpu_shader.comp") + its SSBOs + uniforms
    (src/computeShader.hpp, src/main.cpp:238-370) on one HIP device."""

    def __init__(self, device=0, lib_path=None):
        # lib_path: another build of librtamd.so (A/B of two builds in one process, tools/ab.py)
        self._lib = rt_lib() if lib_path is None else _bind(C.CDLL(os.path.abspath(lib_path)), RT_SYMBOLS, partial=True)
        h = C.c_void_p()
        self._chk(self._lib.rt_create(C.byref(h), device), "rt_create")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _chk(rc, what):
        if rc != 0:
            raise RTError(what, rc)

    def set_stream(self, stream_handle):
        self._chk(self._lib.rt_set_stream(self._h, C.c_void_p(stream_handle) if stream_handle else None),
                  "rt_set_stream")

    def upload(self, fs: FlatScene):
        self._keep = fs
        self._chk(self._lib.rt_upload_scene(self._h, _ptr(fs.shapes), len(fs.shapes), _ptr(fs.nodes), len(fs.nodes),
                                            _ptr(fs.indices), len(fs.indices)), "rt_upload_scene")
        self.set_camera(fs.camera)
        self.set_light(fs.light)

    def update_shapes(self, first, shapes):
        shapes = as_records(shapes, SHAPE_DTYPE)
        self._chk(self._lib.rt_update_shapes(self._h, first, len(shapes), _ptr(shapes)), "rt_update_shapes")

    def update_nodes(self, nodes):
        nodes = as_records(nodes, NODE_DTYPE)
        self._chk(self._lib.rt_update_nodes(self._h, _ptr(nodes), len(nodes)), "rt_update_nodes")

    def set_animated(self, ids):
        """Marks the animated shapes (animatedIndices, src/main.cpp:120,706-708)."""
        ids = np.ascontiguousarray(ids, np.int32)
        self._n_animated = len(ids)
        self._chk(self._lib.rt_set_animated(self._h, _ptr(ids), len(ids)), "rt_set_animated")

    def animate(self, shapes):
        """New records of the animated shapes, in set_animated order: updateScene +
        updateBVH + serializeBVH + upload (src/main.cpp:336-346), on the device."""
        shapes = as_records(shapes, SHAPE_DTYPE)
        if len(shapes) != getattr(self, "_n_animated", -1):
            raise ValueError("animate: one record per animated shape")
        self._chk(self._lib.rt_animate(self._h, _ptr(shapes)), "rt_animate")

    def read_nodes(self, num_nodes):
        """The current node records (boxes grown by animate)."""
        out = np.zeros(num_nodes, NODE_DTYPE)
        self._chk(self._lib.rt_read_nodes(self._h, _ptr(out), num_nodes), "rt_read_nodes")
        return out

    def set_camera(self, cam):
        cam = as_records(cam, CAMERA_DTYPE)
        self._chk(self._lib.rt_set_camera(self._h, _ptr(cam)), "rt_set_camera")

    def set_light(self, light):
        light = as_records(light, LIGHT_DTYPE)
        self._chk(self._lib.rt_set_light(self._h, _ptr(light)), "rt_set_light")

    def set_lights(self, lights):
        """rt_set_lights: 1..MAX_LIGHTS point lights (LIGHT_DTYPE records) from the next dispatch
        on, replacing the whole set; one record is set_light."""
        lights = as_records(lights, LIGHT_DTYPE).reshape(-1)
        self._chk(self._lib.rt_set_lights(self._h, _ptr(lights), len(lights)), "rt_set_lights")

    def get_lights(self):
        """rt_get_lights: the set in force as LIGHT_DTYPE records."""
        out = np.zeros(MAX_LIGHTS, LIGHT_DTYPE)
        n = C.c_int()
        self._chk(self._lib.rt_get_lights(self._h, _ptr(out), MAX_LIGHTS, C.byref(n)), "rt_get_lights")
        return out[:n.value]

    def set_soft_shadows(self, radii, samples=16):
        """rt_set_soft_shadows: light i of the set in force gets the radius radii[i] (lights past
        the list stay points) and every light with a radius > 0 `samples` shadow rays, from the
        next dispatch on; None or an empty list turns soft shadows off."""
        radii = np.zeros(0, np.float32) if radii is None else np.ascontiguousarray(radii, np.float32).reshape(-1)
        self._chk(self._lib.rt_set_soft_shadows(self._h, _ptr(radii), len(radii), int(samples)), "rt_set_soft_shadows")

    def get_soft_shadows(self):
        """rt_get_soft_shadows: (radii as float32, samples); (empty, 0) while soft shadows are off."""
        out = np.zeros(MAX_LIGHTS, np.float32)
        n, k = C.c_int(), C.c_int()
        self._chk(self._lib.rt_get_soft_shadows(self._h, _ptr(out), MAX_LIGHTS, C.byref(n), C.byref(k)),
                  "rt_get_soft_shadows")
        return out[:n.value], k.value

    def set_params(self, resX, resY, maxBounces=3, useBVH=True, useFresnel=False, useMollerTrumbore=False):
        p = rt_params(float(resX), float(resY), int(maxBounces), int(bool(useBVH)), int(bool(useFresnel)),
                      int(bool(useMollerTrumbore)))
        self._chk(self._lib.rt_set_params(self._h, C.byref(p)), "rt_set_params")

    def set_kernel(self, kernel):
        self._chk(self._lib.rt_set_kernel(self._h, int(kernel)), "rt_set_kernel")

    def dispatch(self, width, height, y0=0, y1=None):
        self._chk(self._lib.rt_dispatch(self._h, width, height, y0, height if y1 is None else y1), "rt_dispatch")

    def dispatch_rows(self, width, height, y0, stripe, step, out_rows, dst_ptr, pitch):
        self._chk(self._lib.rt_dispatch_rows(self._h, width, height, y0, stripe, step, out_rows,
                                             C.c_void_p(dst_ptr), pitch), "rt_dispatch_rows")

    def dispatch_rows_rgb(self, width, height, y0, stripe, step, out_rows, dst_ptr, pitch):
        """rt_dispatch_rows_fmt with RT_FORMAT_RGB32F: packed 12-byte pixels."""
        self._chk(self._lib.rt_dispatch_rows_fmt(self._h, width, height, y0, stripe, step, out_rows,
                                                 C.c_void_p(dst_ptr), pitch, 1), "rt_dispatch_rows_fmt")

    def dispatch_rows_ex(self, width, height, y0, stripe, period, out_rows, dst_ptr, pitch, rgb=False, fmt=None):
        """rt_dispatch_rows_ex: stripes of `stripe` rows from y0, one every `period` rows.
        fmt: FORMAT_RGBA32F / FORMAT_RGB32F / FORMAT_RGBA32F_IMAGE (default: RGB32F if rgb)."""
        f = int(fmt) if fmt is not None else int(bool(rgb))
        self._chk(self._lib.rt_dispatch_rows_ex(self._h, width, height, y0, stripe, period, out_rows,
                                                C.c_void_p(dst_ptr), pitch, f), "rt_dispatch_rows_ex")

    def sync(self):
        self._chk(self._lib.rt_sync(self._h), "rt_sync")

    def sync_frame(self):
        """Waits for the last dispatch's frame (rt_sync_frame), not the renderer's order work behind it."""
        self._chk(self._lib.rt_sync_frame(self._h), "rt_sync_frame")

    def read_image(self, width, height):
        out = np.empty((height, width, 4), np.float32)
        self._chk(self._lib.rt_read_image(self._h, _ptr(out), width * 16, width, height), "rt_read_image")
        return out

    def set_surface_format(self, fmt):
        """rt_set_surface_format: the context surface's format from the next dispatch on
        (FORMAT_RGBA32F, FORMAT_RGBA8, FORMAT_SRGBA8 or FORMAT_RGBA16F)."""
        self._chk(self._lib.rt_set_surface_format(self._h, int(fmt)), "rt_set_surface_format")
        self._surface_fmt = int(fmt)  # render() reads floats through rt_read_image while this is RGBA32F

    def surface_format(self):
        f = C.c_int()
        self._chk(self._lib.rt_surface_format(self._h, C.byref(f)), "rt_surface_format")
        return f.value

    def device_image(self):
        """(pointer, pitch in bytes) of the context surface, in its format (rt_device_image)."""
        p, pitch = C.c_void_p(), C.c_size_t()
        self._chk(self._lib.rt_device_image(self._h, C.byref(p), C.byref(pitch)), "rt_device_image")
        return p.value, pitch.value

    def read_surface(self, width, height, out=None):
        """rt_read_surface: the surface in the format set: [H, W, 4] uint8 (RGBA8, SRGBA8),
        float16 (RGBA16F) or float32. out: a C-contiguous [H, W, 4] array of that type to
        fill (pinned memory, say) instead of a new one."""
        dt = np.dtype(SURFACE_DTYPE[self.surface_format()])
        if out is None:
            out = np.empty((height, width, 4), dt)
        elif out.dtype != dt or out.shape != (height, width, 4) or not out.flags.c_contiguous:
            raise ValueError(f"read_surface: out must be a C-contiguous [{height}, {width}, 4] {dt} array")
        self._chk(self._lib.rt_read_surface(self._h, _ptr(out), width * 4 * dt.itemsize, width, height),
                  "rt_read_surface")
        return out

    def render(self, width, height, y0=0, y1=None, fmt=None):
        """dispatch + barrier + readback of the full surface. fmt: render and return the frame
        in this surface format (set_surface_format; it stays set), float32 RGBA when None and
        no other format is set."""
        if fmt is not None:
            self.set_surface_format(fmt)
        self.dispatch(width, height, y0, y1)
        self.sync()
        if getattr(self, "_surface_fmt", FORMAT_RGBA32F) == FORMAT_RGBA32F:
            return self.read_image(width, height)
        return self.read_surface(width, height)

    def collect_stats(self, width, height, y0=0, stripe=1, step=1, out_rows=None):
        st = rt_stats()
        rows = height - y0 if out_rows is None else out_rows
        self._chk(self._lib.rt_collect_stats(self._h, width, height, y0, stripe, step, rows, C.byref(st)),
                  "rt_collect_stats")
        return st.as_dict()

    def kernel_times(self, cap=1024):
        """Device ms of each render dispatch since the last call (HIP events on the ctx stream)."""
        buf = np.zeros(cap, np.float32)
        n = self._lib.rt_kernel_times(self._h, _ptr(buf), cap)
        if n < 0:
            raise RTError("rt_kernel_times", n)
        return buf[:min(n, cap)].copy()

    def set_walk(self, lane_from_depth):
        self._chk(self._lib.rt_set_walk(self._h, int(lane_from_depth)), "rt_set_walk")

    def build_lbvh(self):
        """Device LBVH over the current shapes (rt_build_lbvh); returns the build's device ms."""
        ms = C.c_float()
        self._chk(self._lib.rt_build_lbvh(self._h, C.byref(ms)), "rt_build_lbvh")
        return ms.value

    def scene_size(self):
        s, n, i = C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.rt_scene_size(self._h, C.byref(s), C.byref(n), C.byref(i)), "rt_scene_size")
        return s.value, n.value, i.value

    def read_tree(self):
        """(nodes, indices) of the current scene tree as FlatNode records and int32."""
        _, n, i = self.scene_size()
        nodes = np.zeros(n, NODE_DTYPE)
        idx = np.zeros(i, np.int32)
        if n:
            self._chk(self._lib.rt_read_nodes(self._h, _ptr(nodes), n), "rt_read_nodes")
        self._chk(self._lib.rt_read_indices(self._h, _ptr(idx) if i else None, i), "rt_read_indices")
        return nodes, idx

    def set_tree(self, mode):
        """TREE_SCENE (default): one SAH tree over the reference leaves where exact; TREE_REFERENCE: the reference tree."""
        self._chk(self._lib.rt_set_tree(self._h, int(mode)), "rt_set_tree")

    def set_tail(self, from_bounce):
        """Bounces >= from_bounce of the rays still alive run compacted in a second kernel; 0 = off."""
        self._chk(self._lib.rt_set_tail(self._h, int(from_bounce)), "rt_set_tail")

    def set_samples(self, n):
        """rt_set_samples: every pixel is the mean of n x n samples (n in 1, 2, 4, 8) on the regular
        sub-pixel grid, i.e. the box filter of the n*W x n*H frame; applies to every dispatch form."""
        self._chk(self._lib.rt_set_samples(self._h, int(n)), "rt_set_samples")

    def set_adaptive(self, threshold):
        """rt_set_adaptive: with set_samples(n > 1), only the pixels whose one-sample value differs
        from a 4-neighbour's by more than `threshold` in some channel take the n x n samples; the
        rest keep the one-sample value. threshold < 0: off (default); inf: the one-sample frame."""
        self._chk(self._lib.rt_set_adaptive(self._h, C.c_float(threshold)), "rt_set_adaptive")

    def adaptive_stats(self):
        """(refined, pixels) of the last dispatch that ran adaptively (rt_adaptive_stats; waits for it)."""
        refined, pixels = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.rt_adaptive_stats(self._h, C.byref(refined), C.byref(pixels)), "rt_adaptive_stats")
        return refined.value, pixels.value

    @staticmethod
    def make_rays(origins, dirs, limits=None):
        """RAY_DTYPE records of n rays; limits default to infinity (any hit occludes)."""
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        rays = np.zeros(len(origins), RAY_DTYPE)
        rays["origin"] = origins
        rays["dir"] = np.asarray(dirs, np.float32).reshape(-1, 3)
        rays["limit"] = np.inf if limits is None else np.asarray(limits, np.float32)
        return rays

    def trace_rays(self, origins, dirs, limits=None, any_hit=False):
        """rt_trace_rays_host: the reference walk's closest INNER hit of each ray over the current
        scene, as (shape, distance, occluded) arrays: shape index or -1, distance or 1e20, and
        whether a hit lies nearer than the ray's limit. any_hit: the shadow walk (TRACE_ANY), which
        fills occluded only (shape -1, distance 1e20)."""
        rays = self.make_rays(origins, dirs, limits)
        hits = np.zeros(len(rays), HIT_DTYPE)
        self._chk(self._lib.rt_trace_rays_host(self._h, _ptr(rays), len(rays), _ptr(hits),
                                               TRACE_ANY if any_hit else TRACE_CLOSEST), "rt_trace_rays_host")
        return hits["shape"].copy(), hits["distance"].copy(), hits["occluded"].copy()

    def trace_rays_device(self, rays_ptr, n, hits_ptr, mode=TRACE_CLOSEST):
        """rt_trace_rays: n RAY_DTYPE records at device address rays_ptr (a torch tensor's
        data_ptr()), HIT_DTYPE records to hits_ptr; stream-ordered, asynchronous."""
        self._chk(self._lib.rt_trace_rays(self._h, C.c_void_p(rays_ptr) if rays_ptr else None, int(n),
                                          C.c_void_p(hits_ptr) if hits_ptr else None, int(mode)), "rt_trace_rays")

    def trace_pixels(self, width, height, xy):
        """rt_trace_pixels: what the camera ray of each pixel (x, y) of a width x height frame
        hits, as (shape, distance, occluded) arrays."""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        hits = np.zeros(len(xy), HIT_DTYPE)
        self._chk(self._lib.rt_trace_pixels(self._h, int(width), int(height), _ptr(xy), len(xy), _ptr(hits)),
                  "rt_trace_pixels")
        return hits["shape"].copy(), hits["distance"].copy(), hits["occluded"].copy()

    @staticmethod
    def make_view_rays(o, d, sky=None):
        """VIEW_RAY_DTYPE records of n rays; sky (the background parameter, a frame's y / resY)
        defaults to 0."""
        o = np.asarray(o, np.float32).reshape(-1, 3)
        rays = np.zeros(len(o), VIEW_RAY_DTYPE)
        rays["origin"] = o
        rays["dir"] = np.asarray(d, np.float32).reshape(-1, 3)
        rays["sky"] = 0.0 if sky is None else np.asarray(sky, np.float32)
        return rays

    @staticmethod
    def _pixel_array(n, fmt):
        if fmt == FORMAT_RGB32F:
            return np.empty((n, 3), np.float32)
        if fmt not in SURFACE_DTYPE:
            raise ValueError(f"shade_rays: no pixel list of format {fmt!r}")
        return np.empty((n, 4), SURFACE_DTYPE[fmt])

    def shade_rays(self, origins, dirs, sky=None, fmt=None):
        """rt_shade_rays_host: the frame's shading (Phong, shadow, mirror bounces, Fresnel; the
        background at each ray's own sky) for n caller rays, as an [n, 4] array of the format's
        channel type ([n, 3] float32 for FORMAT_RGB32F). origins may also be a ready
        VIEW_RAY_DTYPE array (dirs and sky None)."""
        fmt = FORMAT_RGBA32F if fmt is None else fmt
        if isinstance(origins, np.ndarray) and origins.dtype == VIEW_RAY_DTYPE and dirs is None:
            rays = np.ascontiguousarray(origins).reshape(-1)
        else:
            rays = self.make_view_rays(origins, dirs, sky)
        out = self._pixel_array(len(rays), fmt)
        self._chk(self._lib.rt_shade_rays_host(self._h, _ptr(rays) if len(rays) else None, len(rays),
                                               _ptr(out) if len(rays) else None, int(fmt)), "rt_shade_rays_host")
        return out

    def shade_rays_device(self, rays_ptr, n, dst_ptr, fmt=FORMAT_RGBA32F):
        """rt_shade_rays: n VIEW_RAY_DTYPE records at device address rays_ptr (a torch tensor's
        data_ptr()), compact pixels of format fmt to dst_ptr; stream-ordered, asynchronous."""
        self._chk(self._lib.rt_shade_rays(self._h, C.c_void_p(rays_ptr) if rays_ptr else None, int(n),
                                          C.c_void_p(dst_ptr) if dst_ptr else None, int(fmt)), "rt_shade_rays")

    def camera_rays(self, width, height, y0=0, rows=None):
        """rt_camera_rays_host: the camera rays a dispatch generates for rows [y0, y0 + rows) of a
        width x height frame (current camera and params), as VIEW_RAY_DTYPE records, row-major."""
        rows = height - y0 if rows is None else rows
        rays = np.zeros(max(0, int(width)) * max(0, int(rows)), VIEW_RAY_DTYPE)
        self._chk(self._lib.rt_camera_rays_host(self._h, int(width), int(height), int(y0), int(rows),
                                                _ptr(rays) if len(rays) else None), "rt_camera_rays_host")
        return rays

    def camera_rays_device(self, width, height, y0, rows, rays_ptr):
        """rt_camera_rays: the same records to device address rays_ptr; stream-ordered, asynchronous."""
        self._chk(self._lib.rt_camera_rays(self._h, int(width), int(height), int(y0), int(rows),
                                           C.c_void_p(rays_ptr) if rays_ptr else None), "rt_camera_rays")

    def debug_shade(self, split=0):
        """Diagnostics: the barycentric k_shade instance with plain walks (1) or with the split
        walks of sparse waves (2); 0: the default choice. Same pixels either way."""
        fn = self._lib.rt_debug_shade
        fn.argtypes = [_P, _I]
        fn.restype = _I
        self._chk(fn(self._h, int(split)), "rt_debug_shade")

    def gbuffer(self, width, height, planes=GBUFFER_PLANES):
        """rt_gbuffer_host: the geometry buffer of the whole width x height frame as a dict of
        numpy arrays: "shape" [H, W] int32 (-1 on a miss), "depth" [H, W] float32 (1e20 on a
        miss), "normal" and "position" [H, W, 4] float32 (position's w is 1 on a hit, 0 on a
        miss). planes: which of them to compute."""
        out, g = {}, rt_gbuffer()
        for name in planes:
            if name not in GBUFFER_PLANES:
                raise ValueError(f"gbuffer: unknown plane {name!r}")
            a = np.empty((height, width) if name in ("shape", "depth") else (height, width, 4),
                         np.int32 if name == "shape" else np.float32)
            out[name] = a
            setattr(g, name, a.ctypes.data)
            setattr(g, name + "_pitch", a.strides[0])
        self._chk(self._lib.rt_gbuffer_host(self._h, int(width), int(height), C.byref(g)), "rt_gbuffer_host")
        return out

    def gbuffer_device(self, width, height, y0, stripe, period, out_rows, shape=None, depth=None, normal=None,
                       position=None):
        """rt_dispatch_gbuffer: compact rows as dispatch_rows_ex; each plane a (device pointer,
        pitch in bytes) pair or None. Stream-ordered, asynchronous."""
        g = rt_gbuffer()
        for name, plane in (("shape", shape), ("depth", depth), ("normal", normal), ("position", position)):
            if plane is not None:
                setattr(g, name, plane[0])
                setattr(g, name + "_pitch", plane[1])
        self._chk(self._lib.rt_dispatch_gbuffer(self._h, int(width), int(height), int(y0), int(stripe), int(period),
                                                int(out_rows), C.byref(g)), "rt_dispatch_gbuffer")

    def debug_gbuffer(self, walk=0, waves=0):
        """Diagnostics: the accelerated geometry-buffer kernel walks per lane (walk 1) instead of
        as packets, with `waves` 8x8 tiles to a block (0: default). Same planes either way."""
        fn = self._lib.rt_debug_gbuffer
        fn.argtypes = [_P, _I, _I]
        fn.restype = _I
        self._chk(fn(self._h, int(walk), int(waves)), "rt_debug_gbuffer")

    def ao(self, width, height, rays, radius, bias=1e-3, planes=AO_PLANES):
        """rt_ao_host: ambient occlusion of the whole width x height frame as a dict of numpy
        arrays: "count" [H, W] uint8, the occluded ones of each pixel's `rays` hemisphere rays
        within `radius`, and "visibility" [H, W] float32 = (rays - count) / rays (1 on a miss)."""
        out, g = {}, rt_ao()
        for name in planes:
            if name not in AO_PLANES:
                raise ValueError(f"ao: unknown plane {name!r}")
            a = np.empty((height, width), np.uint8 if name == "count" else np.float32)
            out[name] = a
            setattr(g, name, a.ctypes.data)
            setattr(g, name + "_pitch", a.strides[0])
        p = rt_ao_params(int(rays), float(radius), float(bias), 0)
        self._chk(self._lib.rt_ao_host(self._h, int(width), int(height), C.byref(p), C.byref(g)), "rt_ao_host")
        return out

    def ao_device(self, width, height, y0, stripe, period, out_rows, rays, radius, bias=1e-3, count=None,
                  visibility=None):
        """rt_dispatch_ao: compact rows as dispatch_rows_ex; each plane a (device pointer, pitch
        in bytes) pair or None. Stream-ordered, asynchronous."""
        g = rt_ao()
        for name, plane in (("count", count), ("visibility", visibility)):
            if plane is not None:
                setattr(g, name, plane[0])
                setattr(g, name + "_pitch", plane[1])
        p = rt_ao_params(int(rays), float(radius), float(bias), 0)
        self._chk(self._lib.rt_dispatch_ao(self._h, int(width), int(height), int(y0), int(stripe), int(period),
                                           int(out_rows), C.byref(p), C.byref(g)), "rt_dispatch_ao")

    def debug_ao(self, form=0, waves=0):
        """Diagnostics: the accelerated ambient-occlusion kernel walks its rays repacked over the
        wave (form 1) or per hit lane (form 2; 0: the default form, per hit lane), with `waves` 8x8 tiles to a
        block (0: default). Same planes either way."""
        fn = self._lib.rt_debug_ao
        fn.argtypes = [_P, _I, _I]
        fn.restype = _I
        self._chk(fn(self._h, int(form), int(waves)), "rt_debug_ao")

    def debug_soft(self, form=0):
        """Diagnostics: the soft-shadow kernel walks the sample rays of bounces >= 1 repacked over
        the wave (form 1) or per live lane (form 2; 0: the default form). Same pixels either way."""
        fn = self._lib.rt_debug_soft
        fn.argtypes = [_P, _I]
        fn.restype = _I
        self._chk(fn(self._h, int(form)), "rt_debug_soft")

    def debug_ss_general(self, on):
        """Diagnostics: supersampled frames render the sample frame and filter it with a second
        kernel even where the accelerated kernel would average the samples in its store."""
        fn = self._lib.rt_debug_ss_general
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(bool(on))), "rt_debug_ss_general")

    def debug_convert_pass(self, on):
        """Diagnostics: display-format frames render as a float frame followed by a conversion
        kernel instead of converting in the render kernel's store (tools/bench_formats.py)."""
        fn = self._lib.rt_debug_convert_pass
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(bool(on))), "rt_debug_convert_pass")

    def debug_convert(self, src_ptr, src_pitch, dst_ptr, pitch, width, rows, fmt):
        """Diagnostics: the display conversion alone: rows x width RGBA32F pixels at device pointer
        src_ptr become pixels of display format fmt at dst_ptr (stream-ordered, asynchronous)."""
        fn = self._lib.rt_debug_convert
        fn.argtypes = [_P, _P, C.c_size_t, _P, C.c_size_t, _I, _I, _I]
        self._chk(fn(self._h, C.c_void_p(src_ptr), src_pitch, C.c_void_p(dst_ptr), pitch, int(width), int(rows),
                     int(fmt)), "rt_debug_convert")

    def debug_shadow_walk(self, from_bounce):
        fn = self._lib.rt_debug_shadow_walk
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(from_bounce)), "rt_debug_shadow_walk")

    def debug_tail_lanes(self, lanes):
        fn = self._lib.rt_debug_tail_lanes
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(lanes)), "rt_debug_tail_lanes")

    def set_kernel_timing(self, on):
        """rt_set_kernel_timing: record the device-time events around each dispatch (default on)."""
        self._chk(self._lib.rt_set_kernel_timing(self._h, int(bool(on))), "rt_set_kernel_timing")

    def set_latency_mode(self, on):
        """rt_set_latency_mode: tune for one frame at a time (split walks, heaviest tiles as 2 waves)."""
        self._chk(self._lib.rt_set_latency_mode(self._h, int(bool(on))), "rt_set_latency_mode")

    def set_schedule(self, mode):
        """SCHED_COST (default): tiles start longest-first by their last work; SCHED_COST_XCD: the same
        order dealt to the 8 XCDs as screen bands; SCHED_ROWS: row-major."""
        self._chk(self._lib.rt_set_schedule(self._h, int(mode)), "rt_set_schedule")

    def debug_scene_stack(self, n):
        """Diagnostics: cap the stack a scene-tree walk may use (0 = no cap); exact at any value."""
        fn = self._lib.rt_debug_scene_stack
        fn.argtypes = [C.c_void_p, C.c_int]
        self._chk(fn(self._h, int(n)), "rt_debug_scene_stack")

    def debug_sched_period(self, period):
        fn = self._lib.rt_debug_sched_period
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(period)), "rt_debug_sched_period")

    def debug_lane_stack(self, n):
        fn = self._lib.rt_debug_lane_stack
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(n)), "rt_debug_lane_stack")

    def debug_tile_order(self, order):
        fn = self._lib.rt_debug_tile_order
        fn.argtypes = [_P, _P, _I]
        o = np.ascontiguousarray(order if order is not None else [], np.int32)
        self._chk(fn(self._h, _ptr(o) if o.size else None, int(o.size)), "rt_debug_tile_order")

    def debug_anim_rebuilds(self):
        """Host rebuilds rt_animate fell back to since the context was made."""
        fn = self._lib.rt_debug_anim_rebuilds
        fn.argtypes = [_P]
        fn.restype = _I
        return int(fn(self._h))

    def debug_refit(self, mode):
        """rt_debug_refit: 1 two launches (records, then boxes), 2 one launch whose box roles
        read the records themselves; -1 (the default) 2 for few records, else 1. Anything else is
        refused: the one-launch shapes with device-side waits and the device copy of the records
        measured slower (profiles/r05x_refit_record_probe.txt, r06_anim_probe_modes.txt)."""
        fn = self._lib.rt_debug_refit
        fn.argtypes = [_P, _I]
        fn.restype = _I
        self._chk(fn(self._h, int(mode)), "rt_debug_refit")

    def debug_refits(self):
        """Device refits that applied rt_update_shapes / rt_update_nodes / rt_animate
        without a host rebuild, since the context was made."""
        fn = self._lib.rt_debug_refits
        fn.argtypes = [_P]
        fn.restype = _I
        return int(fn(self._h))

    def debug_split(self, max_rays, group=8):
        """Split per-lane walks of waves with <= max_rays rays over groups of <= group lanes (0: off)."""
        fn = self._lib.rt_debug_split
        fn.argtypes = [_P, _I, _I]
        self._chk(fn(self._h, int(max_rays), int(group)), "rt_debug_split")

    def debug_heavy(self, k, parts):
        """Run the k heaviest tiles of the cost order as `parts` waves each (parts 1: off)."""
        fn = self._lib.rt_debug_heavy
        fn.argtypes = [_P, _I, _I]
        self._chk(fn(self._h, int(k), int(parts)), "rt_debug_heavy")

    def debug_sched_order(self, n):
        """The current cost order's first n tiles (longest first); empty before one exists."""
        fn = self._lib.rt_debug_sched_order
        fn.argtypes = [_P, _P, _I]
        buf = np.zeros(max(n, 1), np.int32)
        k = fn(self._h, _ptr(buf), int(n))
        if k < 0:
            raise RTError("rt_debug_sched_order", k)
        return buf[:k].copy()

    def debug_sched_cost(self, n):
        """The first n tiles' costs as the last cost-recording dispatch wrote them (raw, not
        dilated): what the current cost order was made from; empty before one exists."""
        fn = self._lib.rt_debug_sched_cost
        fn.argtypes = [_P, _P, _I]
        buf = np.zeros(max(n, 1), np.uint32)
        k = fn(self._h, _ptr(buf), int(n))
        if k < 0:
            raise RTError("rt_debug_sched_cost", k)
        return buf[:k].copy()

    def debug_refit_stats(self):
        """The refit's shape: dirty slots, largest / total prim range, nodes, entries."""
        fn = self._lib.rt_debug_refit_stats
        fn.argtypes = [_P, C.c_void_p]
        out = np.zeros(7, np.int64)
        self._chk(fn(self._h, out.ctypes.data), "rt_debug_refit_stats")
        return dict(zip(["dirty_slots", "max_range", "sum_range", "nodes", "entries", "flush_bytes", "compactions"],
                        out.tolist()))

    _DUMP = [("staging_shapes", SHAPE_DTYPE), ("staging_nodes", NODE_DTYPE), ("nodes", "<f4"), ("geo_lin", "<f4"),
             ("geo_leaf", "<f4"), ("mat", "<f4"), ("prims", "<f4"), ("anodes", "<f4"), ("wnodes", "<f4"),
             ("titems", "<f4"), ("lnodes", "<f4"), ("pbox", "<f4"), ("info", "<i4"), ("finfo", "<f4"),
             ("slots", "<i4"), ("prim_shape", "<i4"), ("shape_cls", "<i4"), ("titem_ref", "<i4"), ("refit_of", "<i4")]

    def debug_accel_dump(self, which="own"):
        """rt_debug_accel_dump: the device state the refit maintains (pending updates applied
        first, as a dispatch does) and the host's topology facts, as numpy arrays. which:
        "own", "brute" or "mtc" (RTError -1 while that sub-context does not exist). float4
        arrays come as (n, 4) float32, `slots` as (wide slots, 4) int32 (has a child, first
        prim, end prim, 1 scene tree | 2 kNoPrune); the info words are also unpacked by name."""
        fn = self._lib.rt_debug_accel_dump
        fn.restype = C.c_int
        fn.argtypes = [_P, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
        w = {"own": 0, "brute": 1, "mtc": 2}[which]
        out = {}
        need = np.zeros(1, np.int64)
        self._chk(fn(self._h, w, -1, None, 0, need.ctypes.data), "rt_debug_accel_dump")  # flush, once
        for sec, (name, dt) in enumerate(self._DUMP):
            self._chk(fn(self._h, w, sec, None, 0, need.ctypes.data), "rt_debug_accel_dump")
            a = np.zeros(int(need[0]) // np.dtype(dt).itemsize, dt)
            if a.size:
                self._chk(fn(self._h, w, sec, a.ctypes.data, a.nbytes, need.ctypes.data), "rt_debug_accel_dump")
            out[name] = a.reshape(-1, 4) if (dt == "<f4" and name != "finfo") or name == "slots" else a
        for k, v in zip(["rec", "mt", "cone_cull", "n_local_wide", "n_wide", "P", "S", "N", "I", "n_titems", "nfew",
                         "n_refit", "built"], out["info"].tolist()):
            out[k] = v
        out["origin_lim"] = np.float32(out["finfo"][0])
        out["mt_z"] = out["finfo"][1:4].copy()
        return out

    def debug_moving(self, period, dilate, split):
        """Cost order of dispatches whose camera moved: re-derived every `period` frames
        (0: as still frames), over costs dilated by `dilate` tiles, split tiles kept on
        its cost frames (`split`)."""
        fn = self._lib.rt_debug_moving
        fn.argtypes = [_P, _I, _I, _I]
        self._chk(fn(self._h, int(period), int(dilate), int(split)), "rt_debug_moving")

    def debug_frame_event(self, on):
        """Latency-mode cost frames record the event rt_sync_frame waits for (1) or not (0)."""
        fn = self._lib.rt_debug_frame_event
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(on)), "rt_debug_frame_event")

    def debug_cost_dilate(self, r):
        """Cost order over each tile's largest cost within r tiles (0: off)."""
        fn = self._lib.rt_debug_cost_dilate
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(r)), "rt_debug_cost_dilate")

    def debug_cost_time(self, mode):
        """Cost-order measure: 1 the tiles' wave wall time, 0 their lanes' steps + tests, -1 default."""
        fn = self._lib.rt_debug_cost_time
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(mode)), "rt_debug_cost_time")

    def debug_lane_k(self, k, mode):
        """The first k dispatch slots walk camera rays (bit 0) / their shadows (bit 1) per lane."""
        fn = self._lib.rt_debug_lane_k
        fn.argtypes = [_P, _I, _I]
        self._chk(fn(self._h, int(k), int(mode)), "rt_debug_lane_k")

    def debug_cone_cull(self, on):
        fn = self._lib.rt_debug_cone_cull
        fn.argtypes = [_P, _I]
        self._chk(fn(self._h, int(bool(on))), "rt_debug_cone_cull")

    def debug_tile_times(self, cap):
        """cap > 0: enable per-tile stamps (diagnostics); then tile_times(cap) reads them."""
        fn = self._lib.rt_debug_tile_times
        fn.argtypes = [_P, _I, _P]
        self._chk(fn(self._h, int(cap), None), "rt_debug_tile_times")

    def tile_times(self, cap):
        """[n, 24] per-tile records of k_accel (layout: kTileRec in rt_kernels.hip)."""
        buf = np.zeros((cap, 24), np.uint64)
        fn = self._lib.rt_debug_tile_times
        fn.argtypes = [_P, _I, _P]
        n = fn(self._h, int(cap), _ptr(buf))
        if n < 0:
            raise RTError("rt_debug_tile_times", n)
        return buf[:n]

    def accel_info(self):
        a = rt_accel_info()
        self._chk(self._lib.rt_accel_info_get(self._h, C.byref(a)), "rt_accel_info_get")
        return {n: getattr(a, n) for n, _ in rt_accel_info._fields_}

    def last_kernel_ms(self):
        ms = C.c_float()
        self._chk(self._lib.rt_last_kernel_ms(self._h, C.byref(ms)), "rt_last_kernel_ms")
        return ms.value


# ---------------------------------------------------------------------------
def group_unique_id() -> bytes:
    """ncclGetUniqueId for rt_group_create_rank (rank 0 makes it, the others receive it)."""
    buf = (C.c_char * GROUP_ID_BYTES)()
    rc = rt_lib().rt_group_unique_id(buf, GROUP_ID_BYTES)
    if rc != 0:
        raise RTError("rt_group_unique_id", rc)
    return bytes(buf)


class _Member(ComputeShader):
    """A group member's context: owned (and destroyed) by its Group."""

    def __init__(self, lib, handle, device):
        self._lib = lib
        self._h = handle
        self.device = device

    def close(self):
        self._h = None


class GroupPhases(C.Structure):
    _fields_ = [("frames", C.c_int), ("render_ms", C.c_float), ("fanin_ms", C.c_float),
                ("unstripe_ms", C.c_float), ("frame_ms", C.c_float)]


class Group:
    """One frame over several GPUs (include/rt_group.h): interleaved row stripes
    per rank (rank 0 may take `share` stripes per period, set_root_share), gathered
    to rank 0 by one grouped ncclSend/ncclRecv per frame over xGMI (RCCL) or by
    device copies, then unstriped on rank 0.

    Group(devices=[0, 1, ...])            one process drives every device
    Group(uid=..., nranks=P, rank=r, device=d)   one process per GPU
    frames=F: F frames in flight (slots), one communicator and one fan-in stream.
    `members` holds each local member's slot-0 context, `contexts` every slot's.
    """

    def __init__(self, devices=None, transport=GATHER_AUTO, uid=None, nranks=None, rank=None, device=None,
                 frames=1):
        self._lib = rt_lib()
        h = C.c_void_p()
        if uid is not None:
            idb = (C.c_char * GROUP_ID_BYTES).from_buffer_copy(uid)
            self._chk(self._lib.rt_group_create_rank(C.byref(h), idb, int(nranks), int(rank), int(device)),
                      "rt_group_create_rank")
        else:
            d = np.ascontiguousarray(devices, np.int32)
            self._chk(self._lib.rt_group_create(C.byref(h), _ptr(d), len(d), int(transport)), "rt_group_create")
        self._h = h
        n, nl, tr = C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.rt_group_info(h, C.byref(n), C.byref(nl), C.byref(tr)), "rt_group_info")
        self.nranks, self.nlocal, self.transport = n.value, nl.value, tr.value
        if frames != 1:
            self._chk(self._lib.rt_group_set_frames(h, int(frames)), "rt_group_set_frames")
        self.frames = self._lib.rt_group_frames(h)
        self.members, self.contexts = [], []
        for k in range(self.nlocal):
            dev = device if uid is not None else int(devices[k])
            for j in range(self.frames):
                c = C.c_void_p()
                self._chk(self._lib.rt_group_member_slot(h, k, j, C.byref(c)), "rt_group_member_slot")
                self.contexts.append(_Member(self._lib, c, dev))
                if j == 0:
                    self.members.append(self.contexts[-1])

    @staticmethod
    def _chk(rc, what):
        if rc != 0:
            raise RTError(what, rc)

    def close(self):
        if getattr(self, "_h", None):
            for m in self.contexts:
                m.close()
            self._lib.rt_group_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def upload(self, fs: FlatScene):
        self._keep = fs
        self._chk(self._lib.rt_group_upload_scene(self._h, _ptr(fs.shapes), len(fs.shapes), _ptr(fs.nodes),
                                                  len(fs.nodes), _ptr(fs.indices), len(fs.indices)),
                  "rt_group_upload_scene")
        self.set_camera(fs.camera)
        self.set_light(fs.light)

    def set_camera(self, cam):
        cam = as_records(cam, CAMERA_DTYPE)
        self._chk(self._lib.rt_group_set_camera(self._h, _ptr(cam)), "rt_group_set_camera")

    def set_light(self, light):
        light = as_records(light, LIGHT_DTYPE)
        self._chk(self._lib.rt_group_set_light(self._h, _ptr(light)), "rt_group_set_light")

    def set_params(self, resX, resY, maxBounces=3, useBVH=True, useFresnel=False, useMollerTrumbore=False):
        p = rt_params(float(resX), float(resY), int(maxBounces), int(bool(useBVH)), int(bool(useFresnel)),
                      int(bool(useMollerTrumbore)))
        self._chk(self._lib.rt_group_set_params(self._h, C.byref(p)), "rt_group_set_params")

    def dispatch(self, width, height, stripe=8):
        self._chk(self._lib.rt_group_dispatch(self._h, width, height, stripe), "rt_group_dispatch")

    # the reference's animated-frame upload on every member and frame slot (rt_group.h)
    def update_shapes(self, first, shapes):
        shapes = as_records(shapes, SHAPE_DTYPE)
        self._chk(self._lib.rt_group_update_shapes(self._h, first, len(shapes), _ptr(shapes)),
                  "rt_group_update_shapes")

    def update_nodes(self, nodes):
        nodes = as_records(nodes, NODE_DTYPE)
        self._chk(self._lib.rt_group_update_nodes(self._h, _ptr(nodes), len(nodes)), "rt_group_update_nodes")

    def set_animated(self, ids):
        """animatedIndices (src/main.cpp:120,706-708) on every member and frame slot."""
        ids = np.ascontiguousarray(ids, np.int32)
        self._n_animated = len(ids)
        self._chk(self._lib.rt_group_set_animated(self._h, _ptr(ids), len(ids)), "rt_group_set_animated")

    def animate(self, shapes):
        """The animated shapes' new records, in set_animated order: updateScene +
        updateBVH + upload (src/main.cpp:336-346) on the device of every member and slot."""
        shapes = as_records(shapes, SHAPE_DTYPE)
        if len(shapes) != getattr(self, "_n_animated", -1):
            raise ValueError("animate: one record per animated shape")
        self._chk(self._lib.rt_group_animate(self._h, _ptr(shapes)), "rt_group_animate")

    def set_root_share(self, share):
        """Rank 0's stripes per period of share + P - 1 (rt_group_set_root_share)."""
        self._chk(self._lib.rt_group_set_root_share(self._h, int(share)), "rt_group_set_root_share")

    def collect_stats(self, width, height, stripe=8):
        """Reference-walk totals of this process's members' rows (rt_group_collect_stats)."""
        st = rt_stats()
        self._chk(self._lib.rt_group_collect_stats(self._h, width, height, stripe, C.byref(st)),
                  "rt_group_collect_stats")
        return st.as_dict()

    def sync(self):
        """Bounded wait (rt_group_set_timeout); RTError -8 / -7 with the communicator aborted."""
        self._chk(self._lib.rt_group_sync(self._h), "rt_group_sync")

    def set_timeout(self, ms):
        self._chk(self._lib.rt_group_set_timeout(self._h, float(ms)), "rt_group_set_timeout")

    def check(self):
        """Non-blocking RCCL asynchronous-error poll (rt_group_check)."""
        self._chk(self._lib.rt_group_check(self._h), "rt_group_check")

    def set_sky_rows(self, on):
        """rt_group_set_sky_rows: keep background-only rows off the links (default on)."""
        self._chk(self._lib.rt_group_set_sky_rows(self._h, int(bool(on))), "rt_group_set_sky_rows")

    def sky_band(self):
        """The image rows [y0, y1) the last dispatch sent over the links (rt_group_sky_band)."""
        y0, y1 = C.c_int(), C.c_int()
        self._chk(self._lib.rt_group_sky_band(self._h, C.byref(y0), C.byref(y1)), "rt_group_sky_band")
        return y0.value, y1.value

    def device_image(self):
        """(pointer, pitch) of rank 0's surface of the last dispatched frame (rt_group_device_image):
        the frame after sync(), until `frames` more dispatches reuse the slot."""
        p, pitch = C.c_void_p(), C.c_size_t()
        self._chk(self._lib.rt_group_device_image(self._h, C.byref(p), C.byref(pitch)), "rt_group_device_image")
        return p.value, pitch.value

    def set_phase_timing(self, on):
        """rt_group_set_phase_timing: record the render / fan-in / unstripe events (default on)."""
        self._chk(self._lib.rt_group_set_phase_timing(self._h, int(bool(on))), "rt_group_set_phase_timing")

    def phase_times(self):
        """Mean device ms of render / fan-in / unstripe / whole frame since the last call."""
        p = GroupPhases()
        self._chk(self._lib.rt_group_phase_times(self._h, C.byref(p)), "rt_group_phase_times")
        return {"frames": p.frames, "render_ms": p.render_ms, "fanin_ms": p.fanin_ms,
                "unstripe_ms": p.unstripe_ms, "frame_ms": p.frame_ms}

    def read_image(self, width, height):
        out = np.empty((height, width, 4), np.float32)
        self._chk(self._lib.rt_group_read_image(self._h, _ptr(out), width * 16, width, height),
                  "rt_group_read_image")
        return out

    def render(self, width, height, stripe=8):
        self.dispatch(width, height, stripe)
        self.sync()
        return self.read_image(width, height)
