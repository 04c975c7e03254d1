// light_set.h — the light set of rt_set_lights as the k_lights kernels take it (host and
// device; rt_device.h, rt_kernels.hip, tests/native/lights_check.cpp). No HIP: plain floats,
// so a CPU test can state the layout the host fills.
#ifndef RT_LIGHT_SET_H
#define RT_LIGHT_SET_H

#include <cstddef>

#include "../../include/rt_api.h"

namespace rtd {

// Passed by value as a kernel argument: the light loop's index is wave-uniform, so a record
// is read with scalar loads from the argument segment. Records past `count` are zero.
struct LightSet {
    float pos[RT_MAX_LIGHTS][3];
    float col[RT_MAX_LIGHTS][3];
    int count;
};
static_assert(sizeof(LightSet) == 2 * RT_MAX_LIGHTS * 12 + 4, "LightSet: 8 positions, 8 colours, a count");
static_assert(offsetof(LightSet, col) == RT_MAX_LIGHTS * 12 && offsetof(LightSet, count) == 2 * RT_MAX_LIGHTS * 12,
              "LightSet layout");

// The first `count` records of `lights` (FlatLight: position at 0, colour at 16; intensity is
// not read by the shader's phong and is not carried).
inline LightSet make_light_set(const FlatLight* lights, int count) {
    LightSet s{};
    s.count = count < 0 ? 0 : count > RT_MAX_LIGHTS ? RT_MAX_LIGHTS : count;
    for (int i = 0; i < s.count; ++i) {
        s.pos[i][0] = lights[i].position.x;
        s.pos[i][1] = lights[i].position.y;
        s.pos[i][2] = lights[i].position.z;
        s.col[i][0] = lights[i].color.x;
        s.col[i][1] = lights[i].color.y;
        s.col[i][2] = lights[i].color.z;
    }
    return s;
}

}  // namespace rtd

#endif
