// plan_check: the dispatch decisions of csrc/dispatch_plan.h against their stated results:
// the 22 k_accel instances and their priority, the heavy-tile split of the frames the
// measurements name, the pixels of a dispatch, the samples paths, the lane_k slots and the
// compaction rule. Exits non-zero on any mismatch.
#include <cstdio>
#include <cstring>

#include "../../opengl-ray-tracer_amd/csrc/dispatch_plan.h"

using namespace rtp;

static int bad = 0, checks = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        ++checks;                                                  \
        if (!(x)) {                                                \
            ++bad;                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);     \
        }                                                          \
    } while (0)

static const bool T = true, F = false;

static bool same(const AccelInstance& a, const AccelInstance& b) {
    return a.timed == b.timed && a.cost == b.cost && a.tail == b.tail && a.mt == b.mt && a.rec == b.rec &&
           a.queue == b.queue && a.ss == b.ss;
}

// <TIMED, COST, TAIL, MT, REC, QUEUE, SS> of RT_ACCEL_INSTANCES (rt_kernels.hip), by case and cost
static const AccelInstance kMt[3] = {{F, F, F, T, F, F, F}, {F, F, F, T, T, F, F}, {F, T, F, T, T, F, F}};
static const AccelInstance kTimes = {T, T, F, F, T, F, F};
static const AccelInstance kTail[3] = {{F, F, T, F, F, T, F}, {F, F, T, F, T, T, F}, {F, T, T, F, T, T, F}};
static const AccelInstance kLatency[3] = {{F, F, T, F, F, F, F}, {F, F, T, F, T, F, F}, {F, T, T, F, T, F, F}};
static const AccelInstance kPlain[3] = {{F, F, F, F, F, F, F}, {F, F, F, F, T, F, F}, {F, T, F, F, T, F, F}};
static const AccelInstance kSsMt[3] = {{F, F, F, T, F, F, T}, {F, F, F, T, T, F, T}, {F, T, F, T, T, F, T}};
static const AccelInstance kSsLatency[3] = {{F, F, T, F, F, F, T}, {F, F, T, F, T, F, T}, {F, T, T, F, T, F, T}};
static const AccelInstance kSsPlain[3] = {{F, F, F, F, F, F, T}, {F, F, F, F, T, F, T}, {F, T, F, F, T, F, T}};

static void check_instances() {
    const Cost costs[3] = {kCostNone, kCostTime, kCostCounters};
    AccelInstance rows[22];
    int n = 0;
    for (int k = 0; k < 3; ++k) {
        const Cost c = costs[k];
        CHECK(same(accel_instance(T, F, F, F, c, F), kMt[k]));
        CHECK(same(accel_instance(F, T, F, F, c, F), kTimes));
        CHECK(same(accel_instance(F, F, T, F, c, F), kTail[k]));
        CHECK(same(accel_instance(F, F, F, T, c, F), kLatency[k]));
        CHECK(same(accel_instance(F, F, F, F, c, F), kPlain[k]));
        CHECK(same(accel_instance(T, F, F, F, c, T), kSsMt[k]));
        CHECK(same(accel_instance(F, F, F, T, c, T), kSsLatency[k]));
        CHECK(same(accel_instance(F, F, F, F, c, T), kSsPlain[k]));
        // the ladder's priority: MT before tile_times before tail before latency
        CHECK(same(accel_instance(T, T, T, T, c, F), kMt[k]));
        CHECK(same(accel_instance(F, T, T, T, c, F), kTimes));
        CHECK(same(accel_instance(F, F, T, T, c, F), kTail[k]));
        // SS over all of them
        CHECK(same(accel_instance(T, T, T, T, c, T), kSsMt[k]));
        CHECK(same(accel_instance(F, T, T, T, c, T), kSsLatency[k]));
        CHECK(same(accel_instance(F, T, T, F, c, T), kSsPlain[k]));
        rows[n++] = kMt[k];
        rows[n++] = kTail[k];
        rows[n++] = kLatency[k];
        rows[n++] = kPlain[k];
        rows[n++] = kSsMt[k];
        rows[n++] = kSsLatency[k];
        rows[n++] = kSsPlain[k];
    }
    rows[n++] = kTimes;
    CHECK(n == 22);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) CHECK(!same(rows[i], rows[j]));
    // every argument combination is one of the 22
    for (int m = 0; m < 32; ++m)
        for (int k = 0; k < 3; ++k) {
            const AccelInstance a = accel_instance(m & 1, m & 2, m & 4, m & 8, costs[k], m & 16);
            bool found = false;
            for (int i = 0; i < n; ++i) found = found || same(a, rows[i]);
            CHECK(found);
        }
}

static HeavyIn heavy_in(int tiles, bool lanes, bool latency) {
    HeavyIn h;
    std::memset(&h, 0, sizeof h);
    h.tiles = tiles;
    h.cu_count = 256;
    h.latency = latency;
    h.lanes = lanes;
    h.heavy_k = -1;  // auto
    h.heavy_parts = 4;
    h.ss = 1;
    return h;
}
static bool split_is(const HeavyIn& h, int k, int parts) {
    const HeavySplit s = heavy_split(h);
    if (s.k != k || s.parts != parts) std::printf("  heavy_split: %d x %d, expected %d x %d\n", s.k, s.parts, k, parts);
    return s.k == k && s.parts == parts;
}

static void check_heavy() {
    CHECK(split_is(heavy_in(7500, F, F), 29, 8));     // 800x600, all packets
    CHECK(split_is(heavy_in(7500, F, T), 58, 32));    // ... waited
    CHECK(split_is(heavy_in(32400, T, T), 162, 2));   // 1920x1080, per-lane walks, waited
    CHECK(split_is(heavy_in(32400, F, T), 162, 4));   // ... all packets
    CHECK(split_is(heavy_in(4080, T, T), 163, 16));   // a 1/8 stripe share of it
    CHECK(split_is(heavy_in(8160, T, T), 326, 8));    // a 1/4 share
    CHECK(split_is(heavy_in(1000, F, F), 16, 8));     // the floor of 16 tiles
    CHECK(split_is(heavy_in(32400, T, F), 0, 1));     // per-lane walks in flight: no split
    HeavyIn h = heavy_in(7500, F, F);                 // the rule gives 29 x 8
    h.ss_fused = true;
    h.ss = 4;                                         // fused 4x4 samples: 8 parts x 4 > 8
    CHECK(split_is(h, 0, 1));
    h.ss = 1;                                         // one lane a block: bands of whole blocks
    CHECK(split_is(h, 29, 8));
    h = heavy_in(7500, F, F);
    h.tile_times = true;
    h.tile_times_cap = 7500 + 29 * 8;                 // a record per tile and per part
    CHECK(split_is(h, 29, 8));
    h.tile_times_cap -= 1;                            // one record short
    CHECK(split_is(h, 0, 1));
    h = heavy_in(32400, T, T);
    h.whole = true;                                   // a wall-time cost frame in latency mode
    CHECK(split_is(h, 0, 1));
    h = heavy_in(100, T, F);                          // rt_debug_heavy: explicit, cut to the frame's tiles
    h.heavy_k = 500;
    h.heavy_parts = 4;
    CHECK(split_is(h, 100, 4));
    h.heavy_parts = 1;                                // one part is no split
    CHECK(split_is(h, 0, 1));
    h.heavy_k = 0;
    h.heavy_parts = 4;
    CHECK(split_is(h, 0, 1));
}

static void check_pixels() {
    // contiguous rows 15..22 of a 20-row frame: 5 of them
    CHECK(dispatch_pixels(Frame{10, 20, 15, 8, 8, 8, 10.f, 20.f}) == 50ull);
    CHECK(dispatch_pixels(Frame{10, 20, 0, 8, 8, 8, 10.f, 20.f}) == 80ull);
    CHECK(dispatch_pixels(Frame{10, 20, 24, 8, 8, 8, 10.f, 20.f}) == 0ull);
    // stripes of 4 rows every 16 from row 4; 10 compact rows: 4 + 4 + 2
    CHECK(dispatch_pixels(Frame{10, 100, 4, 4, 16, 10, 10.f, 100.f}) == 100ull);
    // 12 compact rows of a 38-row frame: the third stripe (rows 36..39) cut to 2
    CHECK(dispatch_pixels(Frame{10, 38, 4, 4, 16, 12, 10.f, 38.f}) == 100ull);
    // ... of a 36-row frame: the third stripe starts past the end
    CHECK(dispatch_pixels(Frame{10, 36, 4, 4, 16, 12, 10.f, 36.f}) == 80ull);
    CHECK(dispatch_pixels(Frame{10, 20, 0, 8, 8, 0, 10.f, 20.f}) == 0ull);
    CHECK(dispatch_pixels(Frame{10, 100, 4, 4, 16, 0, 10.f, 100.f}) == 0ull);
    const Frame o = output_frame(Frame{152, 88, 16, 8, 32, 24, 152.f, 88.f}, 2);
    CHECK(o.width == 76 && o.height == 44 && o.y0 == 8 && o.stripe == 4 && o.period == 16 && o.out_rows == 12);
    CHECK(o.resX == 76.f && o.resY == 44.f);
}

static bool flags_are(const Samples& s, bool ss, bool ss_accel, bool adaptive, bool ad_fast, bool ss_fused, bool filter) {
    return s.ss == ss && s.ss_accel == ss_accel && s.adaptive == adaptive && s.ad_fast == ad_fast &&
           s.ss_fused == ss_fused && s.filter == filter;
}

static void check_samples() {
    for (int accel = 0; accel < 2; ++accel)
        for (int ad = 0; ad < 2; ++ad)
            for (int tt = 0; tt < 2; ++tt)
                for (int gen = 0; gen < 2; ++gen) {
                    // one sample: nothing of it applies
                    CHECK(flags_are(samples_plan(F, 1, accel, tt, gen, ad, F, F), F, F, F, F, F, F));
                    const Samples s = samples_plan(F, 4, accel, tt, gen, ad, F, F);
                    if (accel && !tt && !gen)  // k_accel reduces the samples, or with adaptive refines B
                        CHECK(flags_are(s, T, T, ad, ad, !ad, F));
                    else  // the sample frame, then the filter kernel
                        CHECK(flags_are(s, T, F, ad, F, F, T));
                }
    // rt_stats dispatches take no samples path; rt_debug_convert_pass filters display frames alone
    CHECK(flags_are(samples_plan(T, 4, T, F, F, T, T, T), F, F, F, F, F, F));
    CHECK(flags_are(samples_plan(F, 1, T, F, F, F, T, T), F, F, F, F, F, T));
    CHECK(flags_are(samples_plan(F, 1, T, F, F, F, T, F), F, F, F, F, F, F));
    CHECK(flags_are(samples_plan(F, 2, T, F, F, F, T, T), T, T, F, F, T, F));
}

static void check_rest() {
    // lane_k: auto in frames that walk per lane, the heaviest 1/128 and at least 64
    LaneSlots l = lane_k_slots(-1, 0, T, 32400);
    CHECK(l.k == 253 && l.mode == 2);
    l = lane_k_slots(-1, 0, T, 1000);
    CHECK(l.k == 64 && l.mode == 2);
    l = lane_k_slots(-1, 0, F, 32400);
    CHECK(l.k == 0 && l.mode == 0);
    l = lane_k_slots(40, 1, F, 32400);  // rt_debug_lane_k
    CHECK(l.k == 40 && l.mode == 1);
    l = lane_k_slots(40, 0, T, 32400);
    CHECK(l.k == 0 && l.mode == 0);
    l = lane_k_slots(0, 2, T, 32400);
    CHECK(l.k == 0 && l.mode == 0);
    // compaction: auto from bounce 2 at 8192 items; not below 3 bounces, not fused, not past 2^32 pixels
    TailPlan t = tail_plan(RT_TAIL_AUTO, 8192, 3, F, 76, 44, 10, 60);
    CHECK(t.tail_from == 2 && t.tail && t.rx == 2 && t.regions == 2);
    t = tail_plan(RT_TAIL_AUTO, 8191, 3, F, 76, 44, 10, 60);
    CHECK(t.tail_from == 0 && !t.tail);
    t = tail_plan(RT_TAIL_AUTO, 8192, 2, F, 76, 44, 10, 60);
    CHECK(t.tail_from == 2 && !t.tail);
    t = tail_plan(1, 0, 3, F, 1920, 1080, 240, 32400);
    CHECK(t.tail_from == 1 && t.tail && t.rx == 30 && t.regions == 30 * 17);
    t = tail_plan(1, 0, 3, T, 1920, 1080, 240, 32400);
    CHECK(!t.tail);
    t = tail_plan(0, 100000, 3, F, 1920, 1080, 240, 32400);
    CHECK(t.tail_from == 0 && !t.tail);
    t = tail_plan(1, 0, 3, F, 65536, 65536, 8192, 8192 * 8192);
    CHECK(!t.tail);
    t = tail_plan(1, 0, 3, F, 65536, 65535, 8192, 8192 * 8192);
    CHECK(t.tail);
    // latency mode: frames of at most 12 tiles per wave slot
    CHECK(latency_frame(T, 12 * 256 * 16, 256) && !latency_frame(T, 12 * 256 * 16 + 1, 256));
    CHECK(!latency_frame(F, 100, 256));
    CHECK(many_items(8192) && !many_items(8191));
}

int main() {
    check_instances();
    check_heavy();
    check_pixels();
    check_samples();
    check_rest();
    std::printf("%s: %d checks, %d failed\n", bad ? "plan_check FAILED" : "plan_check ok", checks, bad);
    return bad ? 1 : 0;
}
