// lights_check: rt_set_lights' routing rule (csrc/dispatch_plan.h: lights_route, accel_renders,
// and what samples_plan makes of such a frame) against its stated results, and the layout of
// the LightSet kernel argument as the host fills it (csrc/light_set.h). Compiled and run by
// tests/test_lights_cpu.py. Exits non-zero on any mismatch.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../opengl-ray-tracer_amd/csrc/dispatch_plan.h"
#include "../../opengl-ray-tracer_amd/csrc/light_set.h"

using namespace rtp;

static int bad = 0, checks = 0;
#define CHECK(x)                                               \
    do {                                                       \
        ++checks;                                              \
        if (!(x)) {                                            \
            ++bad;                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #x); \
        }                                                      \
    } while (0)

static void check_route() {
    // one light: nothing new, whatever else holds
    for (int accel = 0; accel < 2; ++accel)
        for (int stats = 0; stats < 2; ++stats) {
            CHECK(lights_route(1, stats != 0, accel != 0) == kLightsOff);
            CHECK(lights_route(0, stats != 0, accel != 0) == kLightsOff);
        }
    for (int n = 2; n <= RT_MAX_LIGHTS; ++n) {
        CHECK(lights_route(n, false, true) == kLightsAccel);
        CHECK(lights_route(n, false, false) == kLightsRef);
        // rt_collect_stats* counts the one-light frame
        CHECK(lights_route(n, true, true) == kLightsOff);
        CHECK(lights_route(n, true, false) == kLightsOff);
    }
    // for the samples paths such a frame is one k_accel does not render
    CHECK(accel_renders(true, kLightsOff));
    CHECK(!accel_renders(false, kLightsOff));
    CHECK(!accel_renders(true, kLightsAccel));
    CHECK(!accel_renders(true, kLightsRef));
    CHECK(!accel_renders(false, kLightsRef));
    // rt_set_samples: the general path (scratch surface, then the filter), never fused
    const Samples s = samples_plan(false, 2, accel_renders(true, kLightsAccel), false, false, false, false, false);
    CHECK(s.ss && !s.ss_accel && !s.ss_fused && !s.adaptive && !s.ad_fast && s.filter);
    // rt_set_adaptive: the adaptive filter kernel's path, not the refine passes
    const Samples a = samples_plan(false, 2, accel_renders(true, kLightsAccel), false, false, true, false, true);
    CHECK(a.ss && a.adaptive && !a.ad_fast && !a.ss_fused && a.filter);
    // one sample: no filter pass (but for the convert pass' own setting)
    const Samples o = samples_plan(false, 1, accel_renders(true, kLightsAccel), false, false, false, false, true);
    CHECK(!o.ss && !o.filter && !o.adaptive);
    // one light under rt_set_samples keeps the fused path
    const Samples f = samples_plan(false, 2, accel_renders(true, lights_route(1, false, true)), false, false, false,
                                   false, false);
    CHECK(f.ss_fused && !f.filter);
}

static void check_light_set() {
    using rtd::LightSet;
    CHECK(RT_MAX_LIGHTS == 8);
    CHECK(sizeof(LightSet) == 196);
    CHECK(offsetof(LightSet, pos) == 0 && offsetof(LightSet, col) == 96 && offsetof(LightSet, count) == 192);
    FlatLight in[RT_MAX_LIGHTS];
    std::memset(in, 0xff, sizeof in);  // the paddings are not read
    for (int i = 0; i < RT_MAX_LIGHTS; ++i) {
        in[i].position = rt_vec3{1.0f + i, 2.0f + i, 3.0f + i};
        in[i].color = rt_vec3{0.5f * i, 0.25f * i, 0.125f * i};
    }
    for (int n = 1; n <= RT_MAX_LIGHTS; ++n) {
        const LightSet s = rtd::make_light_set(in, n);
        float raw[49];
        std::memcpy(raw, &s, sizeof s);
        int cnt;
        std::memcpy(&cnt, reinterpret_cast<const char*>(&s) + 192, 4);
        CHECK(cnt == n);
        for (int i = 0; i < RT_MAX_LIGHTS; ++i)
            for (int k = 0; k < 3; ++k) {
                const float p = i < n ? (&in[i].position.x)[k] : 0.0f, c = i < n ? (&in[i].color.x)[k] : 0.0f;
                CHECK(raw[3 * i + k] == p);
                CHECK(raw[24 + 3 * i + k] == c);
            }
    }
    CHECK(rtd::make_light_set(in, 0).count == 0);
    CHECK(rtd::make_light_set(in, 99).count == RT_MAX_LIGHTS);
}

int main() {
    check_route();
    check_light_set();
    std::printf("lights_check %s: %d checks, %d failed\n", bad ? "FAILED" : "ok", checks, bad);
    return bad ? 1 : 0;
}
