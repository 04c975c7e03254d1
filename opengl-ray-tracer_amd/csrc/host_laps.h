// host_laps.h — diagnostics (RT_REBUILD_PROFILE set): wall time of the phases of a host
// step on stderr, each lap since the previous one. No HIP.
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace rta {

struct PhaseLaps {
    const char* step;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseLaps(const char* s) : step(s) {}
    void operator()(const char* what) {
        static const bool on = std::getenv("RT_REBUILD_PROFILE") != nullptr;
        if (!on || !step) return;  // (a null step: this instance reports nothing)
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "%s %-24s %8.3f ms\n", step, what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
};
// a lap of the caller's, if it passed one
inline void lap_of(PhaseLaps* laps, const char* what) {
    if (laps) (*laps)(what);
}

}  // namespace rta
