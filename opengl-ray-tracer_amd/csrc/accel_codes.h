// accel_codes.h — the constants of the accelerator's device layout that the host packer
// (accel_pack.h, refit_plan.h) and the kernels (rt_kernels.hip) share: child codes, record
// strides, build thresholds. No HIP: plain C++.
#pragma once

#include <cstring>

namespace rta {

constexpr int kMaxStack = 64;  // gpu_shader.comp:384
constexpr int kLeafScan = 8;   // leaves with more shapes get a local BVH (accel.h)

// Child codes of the walks' stacks and of lnodes / wnodes entries.
constexpr unsigned kLocal = 0x80000000u, kLeaf = 0x40000000u, kTopLeaf = 0x20000000u, kItem = 0x10000000u;
// A wide-node code (kLocal without kLeaf) with kPair names a node of two consecutive
// records (accel.h kWideKids, AccelHost::wpair): both are tested at one step.
constexpr unsigned kPair = 0x08000000u, kRecMask = 0x07ffffffu;
constexpr int kNoChild = 0x7fffffff;

// Wide-node record stride in float4: 8 (quantized cones), 17 for the
// Moller-Trumbore accelerator: boxes (6), float grazing cones (4: axis, s),
// the per-ray padding constants (6, accel.h AccelHost::lmt) and the codes.
constexpr int kWideRec = 8, kWideRecMt = 17;

constexpr int kBigList = 256;  // a slot's refit list a wave unions in one step

// float4 / int4 of the device arrays (rt_kernels.hip asserts size and alignment), so
// that arrays packed on the host upload without a conversion pass.
struct alignas(16) F4 {
    float x, y, z, w;
};
struct alignas(16) I4 {
    int x, y, z, w;
};

inline float bits_f(int v) {
    float f;
    std::memcpy(&f, &v, sizeof f);
    return f;
}

}  // namespace rta
