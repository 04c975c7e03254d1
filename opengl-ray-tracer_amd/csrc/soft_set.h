// soft_set.h — the area-light setting of rt_set_soft_shadows as the k_soft kernels take it
// (host and device; rt_device.h, rt_kernels.hip, tests/native/soft_check.cpp). No HIP: plain
// floats and ints, so a CPU test can state the layout the host fills.
#ifndef RT_SOFT_SET_H
#define RT_SOFT_SET_H

#include <cstddef>

#include "../../include/rt_api.h"

namespace rtd {

// Passed by value as a kernel argument, next to the LightSet: the light and sample loops'
// indices are wave-uniform, so a radius is read with a scalar load from the argument segment.
// radius[i] belongs to light i of the LightSet; 0 is a point light (one shadow ray).
struct SoftSet {
    float radius[RT_MAX_LIGHTS];
    int samples;  // K, 1..RT_MAX_SHADOW_SAMPLES: the shadow rays of a light with radius > 0
};
static_assert(sizeof(SoftSet) == RT_MAX_LIGHTS * 4 + 4, "SoftSet: 8 radii, a sample count");
static_assert(offsetof(SoftSet, samples) == RT_MAX_LIGHTS * 4, "SoftSet layout");

// The first `count` radii (the rest 0) and K clamped to 1..RT_MAX_SHADOW_SAMPLES.
inline SoftSet make_soft_set(const float* radii, int count, int samples) {
    SoftSet s{};
    const int n = count < 0 ? 0 : count > RT_MAX_LIGHTS ? RT_MAX_LIGHTS : count;
    for (int i = 0; i < n; ++i) s.radius[i] = radii[i];
    s.samples = samples < 1 ? 1 : samples > RT_MAX_SHADOW_SAMPLES ? RT_MAX_SHADOW_SAMPLES : samples;
    return s;
}

}  // namespace rtd

#endif
