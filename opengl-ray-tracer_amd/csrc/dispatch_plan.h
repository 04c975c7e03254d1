// dispatch_plan.h — the per-dispatch decisions of rt_kernels.hip's launch routines that are
// pure arithmetic (host; rt_kernels.hip, tests/native/plan_check.cpp): which samples path a
// frame takes, how many pixels it writes, which of the cost order's heaviest tiles run as
// several waves, which walk their shadows per lane, whether the rays' later bounces are
// compacted, and which k_accel instance renders it. No HIP and no rt_ctx: plain values in,
// plain structs out, so that a CPU test can state every rule's results.
#ifndef RT_DISPATCH_PLAN_H
#define RT_DISPATCH_PLAN_H

#include <algorithm>
#include <cstddef>

#include "../../include/rt_api.h"

namespace rtp {

constexpr size_t kTailAutoItems = 8192;  // RT_TAIL_AUTO threshold
// the heaviest tiles of the cost order as several waves (rt_debug_heavy): the auto rule's frames
constexpr int kHeavyAutoSlots = 2;
// latency mode: frames of at most this many tiles per wave slot (16 per CU). 12: the car's
// 3840x2160 half share (64,800 tiles) waited 0.360 ms with it against 0.318 without, its
// quarter share (32,640) 0.19 against 0.27 (profiles/r05r_share_sweep.json)
constexpr int kLatencyMaxSlots = 12;

// The rows of a frame as a dispatch maps them (KParams' members of the same names).
struct Frame {
    int width, height, y0, stripe, period, out_rows;
    float resX, resY;
};

// The pixels a dispatch of the OUTPUT frame `k` writes: its compact rows below the frame's end.
inline unsigned long long dispatch_pixels(const Frame& k) {
    if (k.period == k.stripe)  // contiguous rows from y0
        return static_cast<unsigned long long>(std::max(0, std::min(k.out_rows, k.height - k.y0))) * k.width;
    unsigned long long rows = 0;
    for (long long s = 0; s * k.stripe < k.out_rows; ++s) {
        const long long base = k.y0 + s * k.period;
        if (base >= k.height) break;
        rows += std::min<long long>({k.stripe, k.out_rows - s * k.stripe, k.height - base});
    }
    return rows * static_cast<unsigned long long>(k.width);
}

// rt_set_lights: which kernels render a frame or a ray list of `lights` lights.
enum LightsRoute {
    kLightsOff,    // one light (or a stats dispatch): the existing kernels, nothing new on the device
    kLightsAccel,  // k_lights over the accelerator (RT_KERNEL_LIGHTS)
    kLightsRef     // k_lights_ref, the literal per-lane loop (RT_KERNEL_LANE)
};

// `accel`: the dispatch would otherwise go to the accelerated kernel (k_accel for a frame --
// RT_KERNEL_AUTO / RT_KERNEL_ACCEL with a usable accelerator, camera within its bound --
// k_shade for a list). rt_collect_stats* counts the reference's one-light frame whatever the set.
inline LightsRoute lights_route(int lights, bool stats, bool accel) {
    if (lights < 2 || stats) return kLightsOff;
    return accel ? kLightsAccel : kLightsRef;
}

// A frame of two or more lights is, for samples_plan, one k_accel does not render: its `accel`.
inline bool accel_renders(bool accel_kind, LightsRoute r) { return accel_kind && r == kLightsOff; }

// rt_set_soft_shadows: which kernels render a frame or a ray list of `lights` lights with the
// radii `radii` (RT_MAX_LIGHTS of them; nullptr: none set). Consulted before lights_route.
enum SoftRoute {
    kSoftOff,    // no light of the set has a radius > 0 (or a stats dispatch): lights_route decides
    kSoftAccel,  // k_soft over the accelerator (RT_KERNEL_SOFT)
    kSoftRef     // k_soft_ref, the literal per-lane loop (RT_KERNEL_LANE)
};

// Soft iff some light i < lights has radii[i] > 0 -- one light included; a radius at an index
// past the set does not count. `stats`, `accel`: as for lights_route.
inline SoftRoute soft_route(int lights, const float* radii, bool stats, bool accel) {
    bool soft = false;
    for (int i = 0; radii && i < lights && i < RT_MAX_LIGHTS; ++i) soft = soft || radii[i] > 0.0f;
    if (!soft || stats) return kSoftOff;
    return accel ? kSoftAccel : kSoftRef;
}

// k_soft's form for the sample rays of bounces >= 1: repacked over the wave (true) or per live
// lane. `form`: rt_debug_soft (1 = repacked, 2 = per lane, 0 = this rule). The repacked instance
// wins where there are later bounces (car 1920x1080, 3 bounces: 6-15 % faster; 100k triangles:
// 3-7 % at K >= 8) but its frame form spills, which costs 6-10 % on a frame of camera rays and
// shadows only (the monkey scene, 1 bounce), where nothing is repacked: so by maxBounces.
inline bool soft_repack(int form, int max_bounces) { return form == 0 ? max_bounces >= 2 : form == 1; }

// A soft frame is, for samples_plan, one k_accel does not render either.
inline bool accel_renders(bool accel_kind, LightsRoute r, SoftRoute s) {
    return accel_renders(accel_kind, r) && s == kSoftOff;
}

struct Samples {
    bool ss, ss_accel, adaptive, ad_fast, ss_fused, filter;
};

// rt_set_samples: k_accel reduces the samples in its store (the SS instances, fused);
// every other frame -- the lane and packet kernels, per-tile records (their instance has
// no SS form), rt_debug_ss_general -- is the one-sample render of the sample frame into
// the context's scratch surface, then k_box_filter (general).
// `n`: the dispatch's samples per axis (KParams::ss); `accel`: k_accel renders the frame;
// `adaptive_on`: rt_set_adaptive's threshold is set; `display`: a display pixel format.
inline Samples samples_plan(bool stats, int n, bool accel, bool tile_times, bool ss_general, bool adaptive_on,
                            bool convert_pass, bool display) {
    Samples s;
    s.ss = !stats && n > 1;
    s.ss_accel = s.ss && accel && !tile_times && !ss_general;
    // rt_set_adaptive: where k_accel would reduce the samples (fast path), it renders the
    // one-sample frame B into the scratch surface instead -- this dispatch from here on, with
    // every setting of a one-sample frame -- and launch_adaptive refines the contrast pixels;
    // every other frame keeps the general path with the adaptive filter kernel.
    s.adaptive = s.ss && adaptive_on;
    s.ad_fast = s.adaptive && s.ss_accel;
    s.ss_fused = s.ss_accel && !s.ad_fast;
    // rt_debug_convert_pass: a one-sample display frame the same way, float frame first, then
    // the filter kernel's conversion (the measurement's baseline, tools/bench_formats.py)
    s.filter = s.ss ? !s.ss_accel : !stats && convert_pass && display;
    return s;
}

// The one-sample output frame of a sample frame `k` of n x n samples per pixel
// (the dispatch scaled it by n: every value is a multiple, the floats exact).
inline Frame output_frame(const Frame& k, int n) {
    return Frame{k.width / n,    k.height / n,   k.y0 / n,
                 k.stripe / n,   k.period / n,   k.out_rows / n,
                 k.resX / static_cast<float>(n), k.resY / static_cast<float>(n)};
}

// rt_set_latency_mode applies to frames of at most kLatencyMaxSlots tiles per wave
// slot: a bigger frame keeps the chip busy on its own, and the split-walk instance's
// throughput cost then outweighs the shorter chains (waited frame, latency mode on
// against off: car 1080p 0.216 against 0.262 ms; car 3840x2160 0.706 against 0.626;
// config 5 3.364 against 3.332; profiles/r04zz2_latency_sweep_*.json)
inline bool latency_frame(bool latency_mode, int tiles, int cu_count) {
    return latency_mode && tiles <= kLatencyMaxSlots * cu_count * 16;
}

// big scenes (the RT_TAIL_AUTO criterion)
inline bool many_items(size_t items) { return items >= kTailAutoItems; }

struct LaneSlots {
    int k, mode;
};

// Of a frame dispatched in the context's cost order:
// the first lane_k dispatch slots (the heaviest tiles): explicit (rt_debug_lane_k)
// or auto -- in frames that walk per lane anyway (LDS stacks allocated), the
// heaviest 1/128 of the tiles walk their camera rays' shadows per lane: shorter
// chains on the slowest tiles (car: serial -5.5 %, 2 in flight equal, r02q)
// `lanes`: some walk is per lane (min(lane_from_depth, shadow_lane_from) < maxBounces).
inline LaneSlots lane_k_slots(int lane_k, int lane_k_mode, bool lanes, int tiles) {
    int lk = lane_k, lm = lane_k_mode;
    if (lk < 0) {
        lk = lanes ? std::max(64, tiles / 128) : 0;
        lm = 2;
    }
    return lk > 0 && lm > 0 ? LaneSlots{lk, lm} : LaneSlots{0, 0};
}

struct HeavyIn {
    int tiles, cu_count;
    bool latency;  // latency_frame
    bool lanes;    // some walk is per lane (min(lane_from_depth, shadow_lane_from) < maxBounces)
    int heavy_k, heavy_parts;  // rt_debug_heavy (heavy_k < 0: auto)
    bool tile_times;           // rt_debug_tile_times, with room for
    size_t tile_times_cap;     // this many records
    // a cost frame by wall time without per-tile records in latency mode, unless the moved
    // camera's frames split (moving && moving_split)
    bool whole;
    bool ss_fused;  // Samples::ss_fused, of
    int ss;         // this many samples per axis
};

struct HeavySplit {
    int k, parts;  // {0, 1}: no tile is split
};

// Of a frame dispatched in the context's cost order:
// heavy tiles: explicit (rt_debug_heavy) or auto. A frame of at most
// kHeavyAutoSlots waves per wave slot whose walks are all packets (config 2:
// 800x600, primary + shadow) is bound by its slowest tiles even with frames
// in flight, and a packet walks the union of its rays' nodes: the heaviest
// 1/256 of its tiles run as 8 waves of 8 rays (measured -20 %, r02n). Where
// per-lane walks dominate the slow tiles (the car's reflections) it loses.
inline HeavySplit heavy_split(const HeavyIn& in) {
    int hk = in.heavy_k, hp = in.heavy_parts;
    if (hk < 0) {
        const bool small = in.tiles <= kHeavyAutoSlots * in.cu_count * 16 && !in.lanes;
        hk = small ? std::max(16, in.tiles / 256) : 0;
        hp = small ? 8 : 1;
        if (small && in.latency) {
            // Waited, such a frame ends on its heaviest packet chains: split into 32
            // waves of 2 rays, a tile's parts walk little more than their own rays'
            // nodes. Config 2 waited (Python loop, tools/latency_sweep.py, r06k-r06m):
            // 29 x 8 (the in-flight rule) 0.0957 ms, 40 x 16 0.0907, 40 x 32 0.0793,
            // 60 / 120 x 32 0.0798, 20 x 32 0.0819, 40 x 64 0.0855. In flight the
            // in-flight rule stays best (4 frames: 0.0314 against 0.0416 with 40 x 32).
            hk = std::max(16, in.tiles / 128);
            hp = 32;
        }
        if (!small && in.latency) {
            // rt_set_latency_mode: the heaviest 1/200 as 4 waves. Car waited frame with the
            // wall-time cost order and whole-tile cost frames (Python loop,
            // profiles/r04z7_latency_sweep.json, r04z8_latency_sweep.json), heaviest k as
            // 4 waves: k = 95 0.2362 ms, 126 0.2161, 159 0.2184, 191 0.2203, 255 0.2260;
            // as 2 waves: 63 0.2371, 127-511 0.224, 1023 0.229; 126 as 8: 0.2275. Some
            // tiles ranked ~96-126 by whole time gain most from the split, so k sits
            // well above that edge (162 of the car's 32,400 tiles).
            // A frame of few tiles per CU (a rank's stripe share of a strong frame) has
            // idle CUs to spread its heaviest chains over: the car's 1/8 share (4,080
            // tiles, 16 per CU) waited 0.175 ms by the whole-frame rule, 0.135-0.144 with
            // its heaviest 1/25 as 16 waves; the 1/4 share (8,160) 0.175-0.192 against
            // 0.156-0.160 with 1/25-1/50 as 8 waves; the 1/2 share mixed (C++ host loop,
            // tools/share_sweep.py, profiles/r05s/r05t_share_sweep*.json)
            // Off the tuned view the 4-wave split lost: four still cameras along
            // bench.py's orbit waited 0.213 / 0.279 / 0.277 / 0.294 ms with it, 0.216 /
            // 0.268 / 0.268 / 0.284 as 2 waves (geometric mean over the views 1.034
            // against 1.011 of each view's best of a 4 x 3 grid; tools/view_sweep.py,
            // profiles/r05za_view_sweep.json): whole frames that walk rays per lane take
            // 2 waves. All-packet frames (the MT car) keep 4: 2.68 ms with 2 against 1.75
            // (r05zl); the heaviest 1/400 as 8, best over two orbit views (geometric mean
            // 1.782 against 1.864 ms, r05zn_view_sweep_mt.json), measured 1.770 against
            // 1.755 at the bench's view and 1.933 against 1.844 animated (r05zo): kept 4
            const int per_cu = in.tiles / std::max(1, in.cu_count);
            hk = std::max(16, in.tiles / (per_cu <= 40 ? 25 : 200));
            hp = per_cu <= 20 ? 16 : per_cu <= 40 ? 8 : in.lanes ? 2 : 4;
        }
    }
    const bool stamps_fit =  // timed frames split only with a record per part
        !in.tile_times ||
        in.tile_times_cap >= static_cast<size_t>(in.tiles) + static_cast<size_t>(std::min(hk, in.tiles)) * hp;
    // In latency mode a dispatch that records wall-time costs runs every tile whole (`whole`):
    // a split tile's parts run side by side, so no sum or maximum of theirs stands for
    // the whole tile's time, and a split set ranked by such an estimate locks in
    // whatever tiles were split first (the car's waited frame settled at 0.222 or
    // 0.237 ms by the split set it started from, r04z5). Recording whole tiles every
    // 16th frame keeps the split set the longest whole tiles. The all-packet frames'
    // own split (8 waves, above) stays on their cost frames: whole, those took 1.5x
    // (config 2, the MT car; r04zz profiles), and in flight the ranking matters less.
    // a supersampled frame's bands hold whole n x n blocks of lanes (8 / hp rows >= n),
    // or the tile is not split: its store reduces each block within one wave
    const bool blocks_whole = !in.ss_fused || hp * in.ss <= 8;
    if (stamps_fit && hp > 1 && hk > 0 && !in.whole && blocks_whole) return HeavySplit{std::min(hk, in.tiles), hp};
    return HeavySplit{0, 1};
}

struct TailPlan {
    int tail_from;  // the first compacted bounce (0: none asked for)
    bool tail;      // this dispatch compacts
    int rx, regions;  // 64x64-pixel regions: per row of them, and in all
};

// compaction: bounces >= tail_from of the rays still alive run in k_accel_tail
// `setting`: rt_set_tail's value; `items`: the scene tree's items.
inline TailPlan tail_plan(int setting, size_t items, int maxBounces, bool ss_fused, int width, int out_rows,
                          int tiles_x, int tiles) {
    TailPlan t;
    // RT_TAIL_AUTO: from bounce 2 on scenes of many scene-tree items (measured: config 5's
    // incoherent bounces -5 %; on the car's 1,302 items the extra kernel costs +18 %)
    t.tail_from = setting != RT_TAIL_AUTO ? setting : (many_items(items) ? 2 : 0);
    // the queue's pixel word is row * width + x in 32 bits (rt_device.h): larger
    // frames render without compaction
    // Supersampled frames render without it too: k_accel_tail finishes pixels one ray
    // at a time and cannot take part in the block reduction (same image either way)
    t.tail = t.tail_from > 0 && t.tail_from < maxBounces && !ss_fused &&
             static_cast<unsigned long long>(width) * out_rows < (1ull << 32);
    t.rx = (tiles_x + 7) / 8;
    t.regions = t.rx * ((tiles / tiles_x + 7) / 8);
    return t;
}

// What a k_accel dispatch records of its tiles for the next frame's order.
enum Cost { kCostNone, kCostTime, kCostCounters };

// k_accel's template arguments <TIMED, COST, TAIL, MT, REC, QUEUE, SS>.
struct AccelInstance {
    bool timed, cost, tail, mt, rec, queue, ss;
};

// The k_accel instance of a dispatch. One that records no tile work runs without the walk
// counters (COST); one that records wall-time costs (cost_time) records them without
// counters (REC alone).
inline AccelInstance accel_instance(bool mt, bool tile_times, bool tail, bool latency, Cost cost, bool ss_fused) {
    const bool rec = cost != kCostNone, cnt = cost == kCostCounters;
    // the supersampling instances (SS): no compaction, no records; Moller-Trumbore, latency
    // mode's split walks, or plain
    if (ss_fused) return AccelInstance{false, cnt, !mt && latency, mt, rec, false, true};
    // Moller-Trumbore accelerator: its own instances; no compaction
    if (mt) return AccelInstance{false, cnt, false, true, rec, false, false};
    // per-tile records (rt_debug_tile_times): counters on, no compaction
    if (tile_times) return AccelInstance{true, true, false, false, true, false, false};
    // the compacting instance, with the split walks of sparse waves (lane_walk_any)
    // that the production instance leaves out for its registers
    if (tail) return AccelInstance{false, cnt, true, false, rec, true, false};
    // latency mode without compaction (tail_from 0): the same split walks, without
    // the queue's code
    if (latency) return AccelInstance{false, cnt, true, false, rec, false, false};
    return AccelInstance{false, cnt, false, false, rec, false, false};  // production
}

}  // namespace rtp

#endif
