// rt_kernels.hip — the MI355X (gfx950) render kernels and the C ABI of
// include/rt_api.h (librtamd.so).
//
// Kernels
//   k_pack_shapes / k_pack_nodes / k_pack_prims : AoS FlatShape/FlatNode (the
//       reference's SSBO records) -> the HBM layouts of rt_device.h and of the
//       accelerator (run once per upload).
//   k_lane<STATS>   : one ray per lane walking the reference's own traversal
//       (stack in LDS, right child first, closest-hit shadow rays). It is the
//       literal restatement of gpu_shader.comp and, with STATS, counts the work
//       that shader performs (node loads, primitive tests, material fetches).
//   k_packet        : a wave64 renders an 8x8 pixel tile as one packet over the
//       reference tree alone: the tree walk order of gpu_shader.comp:384-426 does
//       not depend on the ray, so the wave walks it once with a 64-bit active mask
//       per stack entry (the stack lives in the wave's VGPR lanes: entry j in
//       lane j, readlane/writelane), node and shape records are wave-uniform
//       scalar loads, and each lane keeps exactly the state, order and
//       tie-breaking of its own reference walk. Shadow rays stop per lane at the
//       first occluder closer than the light (equivalent to the reference's
//       closest-hit test). It renders the frames the accelerator
//       cannot (accel_usable).
//   k_accel<TIMED, COST, TAIL, MT, REC, QUEUE, SS> : the production kernel. One 8x8
//       tile (or one band of a split heavy tile) per wave over the exact-result
//       accelerator (accel.h): packet walks (packet_walk) for coherent rays,
//       per-lane walks with LDS stacks (lane_walk) for the rest, same image as
//       the kernels above. rtp::accel_instance (dispatch_plan.h) picks the instance and
//       accel_kernel() finds it; the one without counters,
//       queue or records (k_accel<false, false>) renders the plain frames. The SS
//       instances render supersampled frames (rt_set_samples): the sample frame's
//       tiles, each n x n block of lanes stored as one mean pixel.
//   k_box_filter<N> : rt_set_samples for the frames k_accel does not render: the
//       N x N box filter of a sample frame the kernels above rendered.
//   k_accel_tail    : the remaining bounces of the rays k_accel queued
//       (rt_set_tail), 64 rays from one screen region to a wave.
//   k_adaptive_classify / k_accel_refine<MT, DISP> / k_box_filter_adaptive<N, DISP> :
//       adaptive supersampling (rt_set_adaptive): the pixels of the one-sample frame that
//       contrast with a neighbour are listed and only their n x n samples shaded, or, for
//       the frames k_accel does not render, picked from the whole sample frame.
//   k_trace<MODE, MT> / k_trace_ref<MODE> : ray queries (rt_trace_rays, rt_trace_pixels):
//       the caller's rays, or the camera rays of the caller's pixels, one per lane
//       through lane_walk over the accelerator (k_trace) or through k_lane's literal
//       walk (k_trace_ref); closest hit or occlusion within a limit per ray.
//   k_shade<MT, SPLIT, DISP> / k_shade_ref<DISP> / k_camera_rays : shaded rays (rt_shade_rays,
//       rt_camera_rays): the caller's rays through k_accel_tail's bounce loop from bounce 0,
//       every walk per lane (k_shade), or through k_lane's literal loop (k_shade_ref), one
//       compact pixel per ray; k_camera_rays writes a frame's own camera rays as such a list.
//   k_lights<MT, DISP, FRAME> / k_lights_ref<DISP, FRAME> : frames and shaded rays of two or
//       more point lights (rt_set_lights): the bounce loop with L shadow walks per bounce
//       (bounce_step_lights). FRAME: one 8x8 tile per wave, camera rays and their shadow rays
//       as packets, later bounces per lane; else k_shade's list. k_lights_ref is the literal loop.
//   k_soft<MT, DISP, FRAME> / k_soft_ref<DISP, FRAME> : frames and shaded rays of area lights
//       (rt_set_soft_shadows): k_lights' shapes with K shadow walks per light of radius > 0
//       (bounce_step_soft), the blocked rays counted per light.
//   k_gbuffer<MT, LANE> / k_gbuffer_ref : geometry buffers (rt_dispatch_gbuffer): the closest
//       hit of every pixel's camera ray as planes of shape, depth, normal and position. One
//       8x8 tile per wave through packet_walk (or lane_walk for a camera beyond the
//       accelerator's origin bound); k_gbuffer_ref is k_lane's literal walk.
//   k_ao<MT, LANE, PACK> / k_ao_ref : ambient occlusion (rt_dispatch_ao): k_gbuffer's camera
//       walk, then each hit pixel's K hemisphere rays through the shadow form of lane_walk,
//       per hit lane or (PACK) repacked over the wave's 64 lanes; one byte per pixel out.
//   k_tile_order / k_cost_dilate : the next frame's dispatch order from the tile
//       costs a k_accel dispatch recorded (rt_set_schedule).
//   k_refit / k_inf_slots : boxes and cones of moved shapes (rt_animate,
//       rt_update_shapes / rt_update_nodes).
//
// Launch geometry: k_lane and k_packet run 256-thread blocks = 4 waves side by
// side = 32 x 8 pixels, grid = ceil(W/32) x ceil(rows/8); k_accel and
// k_accel_tail run one wave per block. Every kernel is compiled with
// -ffp-contract=off (Makefile) so its float sequence is the oracle's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <atomic>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include "../../include/rt_api.h"
#include "accel.h"
#include "accel_math.h"
#include "accel_pack.h"
#include "refit_plan.h"
#include "lbvh.h"
#include "rt_device.h"
#include "ao_table.h"
#include "dispatch_plan.h"
#include "group_wait.h"
#include "rt_internal.h"

using namespace rtd;

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 32;  // pixels per block row (4 waves x 8)
constexpr int kTileH = 8;
constexpr int kRing = 1024;    // dispatch timings kept between rt_kernel_times calls
// the device layout's codes, strides and thresholds, shared with the host packer (accel_codes.h)
using rta::kMaxStack, rta::kLeafScan, rta::kLocal, rta::kLeaf, rta::kTopLeaf, rta::kItem, rta::kPair, rta::kRecMask,
    rta::kNoChild, rta::kWideRec, rta::kWideRecMt, rta::kBigList, rta::bits_f, rta::PhaseLaps;

// Stats slots, in rt_stats field order.
enum {
    ST_PIXELS = 0, ST_CLOSEST, ST_SHADOW, ST_NODES,
    ST_BVH0, ST_BVH1, ST_BVH2, ST_BVH3,
    ST_BR0, ST_BR1, ST_BR2, ST_BR3,
    ST_UPD, ST_HITS, ST_COUNT
};

// ---------------------------------------------------------------------------
// Pack kernels

// The ray-independent part of a shape's intersection record (GeoRec).
__device__ GeoRec pack_geo(const FlatShape& s, int si) {
    GeoRec g;
    for (int k = 0; k < 18; ++k) g.f[k] = 0.f;
    g.type = s.type;
    g.idx = si;
    if (s.type == RT_SPHERE) {
        g.f[0] = s.sphereCenter.x; g.f[1] = s.sphereCenter.y; g.f[2] = s.sphereCenter.z;
        g.f[3] = s.sphereRadius;
    } else {
        V n = mk(s.planeNormal.x, s.planeNormal.y, s.planeNormal.z);
        g.f[0] = n.x; g.f[1] = n.y; g.f[2] = n.z; g.f[3] = s.planeD;
        if (s.type == RT_WALL) {
            g.f[4] = s.wallStart.x; g.f[5] = s.wallStart.y; g.f[6] = s.wallStart.z;
            g.f[7] = s.wallWidth; g.f[8] = s.wallHeight;
            // gpu_shader.comp:305-307, a function of the normal only.
            V u = normalize(cross(n, mk(0.f, 1.f, 0.f)));
            if (len(u) < 1e-5f) u = normalize(cross(n, mk(1.f, 0.f, 0.f)));
            V v = normalize(cross(n, u));
            g.f[9] = u.x; g.f[10] = u.y; g.f[11] = u.z;
            g.f[12] = v.x; g.f[13] = v.y; g.f[14] = v.z;
        } else if (s.type == RT_TRIANGLE) {
            V p1 = mk(s.triP1.x, s.triP1.y, s.triP1.z);
            V e1 = mk(s.triP2.x, s.triP2.y, s.triP2.z) - p1;
            V e2 = mk(s.triP3.x, s.triP3.y, s.triP3.z) - p1;
            // gpu_shader.comp:218-229, ray-independent part.
            float d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2);
            g.f[4] = p1.x; g.f[5] = p1.y; g.f[6] = p1.z;
            g.f[7] = e1.x; g.f[8] = e1.y; g.f[9] = e1.z;
            g.f[10] = e2.x; g.f[11] = e2.y; g.f[12] = e2.z;
            g.f[13] = d00; g.f[14] = d01; g.f[15] = d11;
            g.f[16] = d00 * d11 - d01 * d01;
        }
    }
    return g;
}

__device__ __forceinline__ void store_geo(float4* out, const GeoRec& g) {
    const float4* in = reinterpret_cast<const float4*>(&g);
    for (int k = 0; k < 5; ++k) out[k] = in[k];
}

// PrimRec (rt_device.h) of a shape's GeoRec and its rank in the reference walk.
__device__ __forceinline__ PrimRec pack_prim(const GeoRec& g, int seq) {
    PrimRec p;
    for (int k = 0; k < 15; ++k) p.f[k] = g.f[k];
    int type = g.type;
    if (type == 3) {
        p.f[13] = g.f[14];  // d01
        p.f[14] = g.f[16];  // d00 * d11 - d01 * d01
    } else if (type < 0 || type > 3) {  // no INNER hit (get_intersection: NONE)
        type = 1;
        p.f[0] = p.f[1] = p.f[2] = __int_as_float(0x7fc00000);
    }
    p.st = (seq << 2) | type;
    return p;
}

__device__ __forceinline__ void store_prim(float4* prims, int j, const PrimRec& p) {
    const float4* in = reinterpret_cast<const float4*>(&p);
    float4* out = prims + 4 * static_cast<size_t>(j);
    for (int k = 0; k < 4; ++k) out[k] = in[k];
}

__device__ __forceinline__ void store_mat(float4* mat, int j, const FlatMaterial& m) {
    mat[2 * j] = make_float4(m.color.x, m.color.y, m.color.z, m.fresnelStrength);
    mat[2 * j + 1] =
        make_float4(m.ambientStrength, m.diffuseStrength, m.specularStrength, static_cast<float>(m.shininess));
}

__global__ void k_pack_shapes(const FlatShape* __restrict__ src, int S, const int* __restrict__ idx, int I,
                              float4* __restrict__ geo_lin, float4* __restrict__ geo_leaf,
                              float4* __restrict__ mat) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int total = S + I;
    if (j >= total) return;
    const bool leaf_slot = j >= S;
    const int si = leaf_slot ? idx[j - S] : j;
    const FlatShape& s = src[si];
    const GeoRec g = pack_geo(s, si);
    store_geo(leaf_slot ? geo_leaf + 5 * static_cast<size_t>(j - S) : geo_lin + 5 * static_cast<size_t>(j), g);
    if (!leaf_slot) store_mat(mat, j, s.material);
}

__global__ void k_pack_nodes(const FlatNode* __restrict__ src, int N, float4* __restrict__ nodes) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const FlatNode& n = src[k];
    int a, b;
    if (n.leftChild == -1) {
        a = -(n.startShapeIdx + 1);
        b = n.numShapes;
    } else {
        a = n.leftChild;
        b = n.rightChild;
    }
    nodes[2 * k] = make_float4(n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, __int_as_float(a));
    nodes[2 * k + 1] = make_float4(n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, __int_as_float(b));
}

// ---------------------------------------------------------------------------
// Shared per-pixel plumbing

struct PixelCoord {
    int x, r, y;
    bool active;
};

__device__ __forceinline__ PixelCoord pixel_of(const KParams& kp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    PixelCoord pc;
    pc.x = blockIdx.x * kTileW + wave * 8 + (lane & 7);
    pc.r = blockIdx.y * kTileH + (lane >> 3);
    pc.active = pc.x < kp.width && pc.r < kp.out_rows;
    pc.y = pc.active ? image_row(kp, pc.r) : 0;
    pc.active = pc.active && pc.y < kp.height;
    return pc;
}

// Background gradient (gpu_shader.comp:436).
__device__ __forceinline__ V background(const KParams& kp, int y) {
    return mix(mk(0.05f, 0.07f, 0.1f), mk(0.5f, 0.7f, 1.0f), static_cast<float>(y) / kp.resY);
}
// The same gradient at a caller's parameter (rt_view_ray::sky; a frame's is y / resY).
__device__ __forceinline__ V background(const KParams&, float sky) {
    return mix(mk(0.05f, 0.07f, 0.1f), mk(0.5f, 0.7f, 1.0f), sky);
}

__device__ __forceinline__ Ray primary_ray(const KParams& kp, int x, int y) {
    return get_ray(kp, 2.0f * static_cast<float>(x) / kp.resX - 1.0f, 1.0f - 2.0f * static_cast<float>(y) / kp.resY);
}

struct Counters {
    unsigned c[ST_COUNT];
};

// Lighting of one bounce (gpu_shader.comp:482-516): adds to acc/att and
// updates the ray; returns true if the path continues.
__device__ __forceinline__ bool shade_bounce(const KParams& kp, Ray& ray, V hp, V hn, const Mat& m, bool shadow,
                                             V& acc, V& att, float offset_reflect) {
    V pc = phong(hp, hn, ray.d, kp.light_pos, kp.light_color, m);
    if (shadow) pc = pc * 0.3f;
    acc = acc + mulv(att, pc);
    if (m.specular > 0.0f) {
        V rd = reflect(ray.d, hn);
        ray.o = hp + hn * offset_reflect;
        ray.d = rd;
        if (kp.useFresnel) {
            float fr = powf(1.0f - gmax(dot(-ray.d, hn), 0.0f), 5.0f);
            fr = gmin(gmax(fr, 0.0f), 0.8f);
            float rw = m.fresnel * fr;
            float mw = 1.0f - rw;
            att = mulv(att, mix(m.color, mk(1.f, 1.f, 1.f), rw));
            acc = acc + mulv(mw * m.color, pc);
        } else {
            att = att * m.specular;
        }
        return true;
    }
    return false;
}

// ---------------------------------------------------------------------------
// k_lane: the reference walk, one ray per lane.

struct LaneHit {
    bool found;
    float d;
    V p;
    int slot;
};

template <bool STATS>
__device__ LaneHit lane_closest_bvh(const KParams& kp, const float4* __restrict__ nodes,
                                    const float4* __restrict__ geo, Ray r, int* stk, Counters& c) {
    LaneHit res{false, 1e20f, mk(0.f, 0.f, 0.f), -1};
    if (kp.N <= 0) return res;
    const V inv = inv_dir(r.d);
    int sp = 0;
    stk[0] = kp.N - 1;
    sp = 1;
    while (sp > 0) {
        --sp;
        const int k = stk[sp * kBlock];
        const float4 a = nodes[2 * k], b = nodes[2 * k + 1];
        if (STATS) c.c[ST_NODES]++;
        if (!ray_aabb(r.o, inv, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z))) continue;
        const int ia = __float_as_int(a.w), ib = __float_as_int(b.w);
        if (ia < 0) {
            const int start = -ia - 1;
            for (int i = 0; i < ib; ++i) {
                const GeoRec g = load_rec(geo, start + i);
                if (STATS && g.type >= 0 && g.type < 4) c.c[ST_BVH0 + g.type]++;
                const Hit h = intersect(g, r, kp.useMT);
                if (h.type == INNER) {
                    const float d = dist(r.o, h.p);
                    if (d < res.d) {
                        res = LaneHit{true, d, h.p, start + i};
                        if (STATS) c.c[ST_UPD]++;
                    }
                }
            }
        } else {
            if (sp + 2 > kp.max_stack) return LaneHit{false, 1e20f, mk(0.f, 0.f, 0.f), -1};
            stk[sp * kBlock] = ia;
            stk[(sp + 1) * kBlock] = ib;
            sp += 2;
        }
    }
    return res;
}

template <bool STATS>
__device__ LaneHit lane_closest_brute(const KParams& kp, const float4* __restrict__ geo, Ray r, Counters& c) {
    LaneHit res{false, 1e20f, mk(0.f, 0.f, 0.f), -1};
    for (int i = 0; i < kp.S; ++i) {
        const GeoRec g = load_rec(geo, i);
        if (STATS && g.type >= 0 && g.type < 4) c.c[ST_BR0 + g.type]++;
        const Hit h = intersect(g, r, kp.useMT);
        if (h.type == INNER) {
            const float d = dist(r.o, h.p);
            if (d < res.d) {
                res = LaneHit{true, d, h.p, i};
                if (STATS) c.c[ST_UPD]++;
            }
        }
    }
    return res;
}

// Brute-force shadow loop (gpu_shader.comp:569-580): stops at the first
// INNER hit nearer than the light.
template <bool STATS>
__device__ bool lane_shadow_brute(const KParams& kp, const float4* __restrict__ geo, Ray sr, float ld, Counters& c) {
    for (int i = 0; i < kp.S; ++i) {
        const GeoRec g = load_rec(geo, i);
        if (STATS && g.type >= 0 && g.type < 4) c.c[ST_BR0 + g.type]++;
        const Hit h = intersect(g, sr, kp.useMT);
        if (h.type == INNER && dist(sr.o, h.p) < ld) return true;
    }
    return false;
}

template <bool STATS>
__global__ __launch_bounds__(kBlock) void k_lane(const float4* __restrict__ geo_leaf,
                                                 const float4* __restrict__ geo_lin,
                                                 const float4* __restrict__ mat,
                                                 const float4* __restrict__ nodes, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;  // entry s of this lane at stk[s * kBlock]
    const PixelCoord pc = pixel_of(kp);
    Counters c;
    if (STATS)
        for (int i = 0; i < ST_COUNT; ++i) c.c[i] = 0;
    if (pc.active) {
        const V bg = background(kp, pc.y);
        Ray ray = primary_ray(kp, pc.x, pc.y);
        V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
        if (STATS) c.c[ST_PIXELS]++;
        const float shadow_off = kp.useBVH ? 1e-3f : 1e-5f;  // :469 vs :565
        for (int depth = 0; depth < kp.maxBounces; ++depth) {
            if (STATS) c.c[ST_CLOSEST]++;
            LaneHit hit = kp.useBVH ? lane_closest_bvh<STATS>(kp, nodes, geo_leaf, ray, stk, c)
                                    : lane_closest_brute<STATS>(kp, geo_lin, ray, c);
            if (!hit.found) {
                acc = acc + mulv(att, bg);
                break;
            }
            if (STATS) c.c[ST_HITS]++;
            const GeoRec g = load_rec(kp.useBVH ? geo_leaf : geo_lin, hit.slot);
            const V hn = shape_normal(g, hit.p);
            const Mat m = load_mat(mat, g.idx);
            Ray sr{hit.p + hn * shadow_off, normalize(kp.light_pos - hit.p)};
            const float ld = dist(kp.light_pos, hit.p);
            bool shadow;
            if (STATS) c.c[ST_SHADOW]++;
            if (kp.useBVH) {
                // Full closest-hit walk, as gpu_shader.comp:473-480.
                LaneHit sh = lane_closest_bvh<STATS>(kp, nodes, geo_leaf, sr, stk, c);
                shadow = sh.found && sh.d < ld;
            } else {
                shadow = lane_shadow_brute<STATS>(kp, geo_lin, sr, ld, c);
            }
            if (!shade_bounce(kp, ray, hit.p, hn, m, shadow, acc, att, 1e-3f)) break;
        }
        store_px(kp, pc.r, pc.x, make_float4(acc.x, acc.y, acc.z, 1.0f));
    }
    if (STATS) {
        for (int i = 0; i < ST_COUNT; ++i) {
            unsigned long long v = c.c[i];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(kp.stats + i, v);
        }
    }
}

// ---------------------------------------------------------------------------
// k_packet: the wave64 packet walk.

__device__ __forceinline__ int lane_id() { return __lane_id(); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Wave-uniform stack of (node, 64-bit mask) held in three VGPRs: entry j in lane j.
struct WaveStack {
    int node, lo, hi;
    int sp;  // uniform
    __device__ __forceinline__ void push(int k, unsigned long long m) {
        const bool mine = lane_id() == sp;  // v_writelane equivalent
        node = mine ? k : node;
        lo = mine ? static_cast<int>(m & 0xffffffffu) : lo;
        hi = mine ? static_cast<int>(m >> 32) : hi;
        ++sp;
    }
    __device__ __forceinline__ void pop(int& k, unsigned long long& m) {
        --sp;
        k = __builtin_amdgcn_readlane(node, sp);
        const unsigned l = static_cast<unsigned>(__builtin_amdgcn_readlane(lo, sp));
        const unsigned h = static_cast<unsigned>(__builtin_amdgcn_readlane(hi, sp));
        m = (static_cast<unsigned long long>(h) << 32) | l;
    }
};

__device__ __forceinline__ bool lane_in(unsigned long long m) { return (m >> lane_id()) & 1ull; }

// Closest hit for every lane in `active` (reference walk order per lane).
__device__ LaneHit packet_closest_bvh(const KParams& kp, const float4* __restrict__ nodes,
                                      const float4* __restrict__ geo, const Ray& r, bool active) {
    LaneHit res{false, 1e20f, mk(0.f, 0.f, 0.f), -1};
    const unsigned long long m0 = __ballot(active);
    if (kp.N <= 0 || m0 == 0) return res;
    const V inv = inv_dir(r.d);
    WaveStack st{0, 0, 0, 0};
    st.push(kp.N - 1, m0);
    while (st.sp > 0) {
        int k;
        unsigned long long m;
        st.pop(k, m);
        k = uni(k);
        const float4 a = nodes[2 * k], b = nodes[2 * k + 1];
        const bool hb = lane_in(m) && ray_aabb(r.o, inv, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z));
        const unsigned long long mh = __ballot(hb);
        if (mh == 0) continue;
        const int ia = uni(__float_as_int(a.w)), ib = uni(__float_as_int(b.w));
        if (ia < 0) {
            const int start = -ia - 1;
            for (int i = 0; i < ib; ++i) {
                const GeoRec g = load_rec(geo, start + i);
                if (hb) {
                    const Hit h = intersect(g, r, kp.useMT);
                    if (h.type == INNER) {
                        const float d = dist(r.o, h.p);
                        if (d < res.d) res = LaneHit{true, d, h.p, start + i};
                    }
                }
            }
        } else {
            if (st.sp + 2 > kMaxStack) {
                // Unreachable: the host rejects trees deeper than the stack.
                return LaneHit{false, 1e20f, mk(0.f, 0.f, 0.f), -1};
            }
            st.push(ia, mh);
            st.push(ib, mh);
        }
    }
    return res;
}

// Shadow query: true iff the lane's reference closest-hit shadow walk would
// find a hit nearer than `ld` (and than the 1e20 start value). Lanes retire at
// their first such hit.
__device__ bool packet_shadow_bvh(const KParams& kp, const float4* __restrict__ nodes,
                                  const float4* __restrict__ geo, const Ray& r, float ld, bool active) {
    bool shadow = false;
    const unsigned long long m0 = __ballot(active);
    if (kp.N <= 0 || m0 == 0) return false;
    const float lim = gmin(ld, 1e20f);
    const V inv = inv_dir(r.d);
    WaveStack st{0, 0, 0, 0};
    st.push(kp.N - 1, m0);
    unsigned long long done = 0;
    while (st.sp > 0) {
        int k;
        unsigned long long m;
        st.pop(k, m);
        m &= ~done;
        if (m == 0) continue;
        k = uni(k);
        const float4 a = nodes[2 * k], b = nodes[2 * k + 1];
        const bool hb = lane_in(m) && ray_aabb(r.o, inv, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z));
        const unsigned long long mh = __ballot(hb);
        if (mh == 0) continue;
        const int ia = uni(__float_as_int(a.w)), ib = uni(__float_as_int(b.w));
        if (ia < 0) {
            const int start = -ia - 1;
            bool live = hb;
            for (int i = 0; i < ib; ++i) {
                const GeoRec g = load_rec(geo, start + i);
                if (live) {
                    const Hit h = intersect(g, r, kp.useMT);
                    if (h.type == INNER && dist(r.o, h.p) < lim) {
                        shadow = true;
                        live = false;
                    }
                }
                if (__ballot(live) == 0) break;
            }
            done = __ballot(shadow);
            if ((m0 & ~done) == 0) break;
        } else {
            if (st.sp + 2 > kMaxStack) return shadow;
            st.push(ia, mh);
            st.push(ib, mh);
        }
    }
    return shadow;
}

__device__ LaneHit packet_closest_brute(const KParams& kp, const float4* __restrict__ geo, const Ray& r,
                                        bool active) {
    LaneHit res{false, 1e20f, mk(0.f, 0.f, 0.f), -1};
    if (__ballot(active) == 0) return res;
    for (int i = 0; i < kp.S; ++i) {
        const GeoRec g = load_rec(geo, i);
        if (active) {
            const Hit h = intersect(g, r, kp.useMT);
            if (h.type == INNER) {
                const float d = dist(r.o, h.p);
                if (d < res.d) res = LaneHit{true, d, h.p, i};
            }
        }
    }
    return res;
}

__device__ bool packet_shadow_brute(const KParams& kp, const float4* __restrict__ geo, const Ray& r, float ld,
                                    bool active) {
    bool live = active, shadow = false;
    if (__ballot(live) == 0) return false;
    for (int i = 0; i < kp.S; ++i) {
        const GeoRec g = load_rec(geo, i);
        if (live) {
            const Hit h = intersect(g, r, kp.useMT);
            if (h.type == INNER && dist(r.o, h.p) < ld) {
                shadow = true;
                live = false;
            }
        }
        if (__ballot(live) == 0) break;
    }
    return shadow;
}

__global__ __launch_bounds__(kBlock) void k_packet(const float4* __restrict__ geo_leaf,
                                                   const float4* __restrict__ geo_lin,
                                                   const float4* __restrict__ mat,
                                                   const float4* __restrict__ nodes, KParams kp) {
    const PixelCoord pc = pixel_of(kp);
    const V bg = background(kp, pc.y);
    Ray ray = primary_ray(kp, pc.x, pc.y);
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    bool alive = pc.active;
    const float shadow_off = kp.useBVH ? 1e-3f : 1e-5f;
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        if (__ballot(alive) == 0) break;
        LaneHit hit = kp.useBVH ? packet_closest_bvh(kp, nodes, geo_leaf, ray, alive)
                                : packet_closest_brute(kp, geo_lin, ray, alive);
        if (alive && !hit.found) {
            acc = acc + mulv(att, bg);
            alive = false;
        }
        V hn = mk(0.f, 0.f, 0.f);
        Mat m{};
        Ray sr{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
        float ld = 0.f;
        if (alive) {
            const GeoRec g = load_rec(kp.useBVH ? geo_leaf : geo_lin, hit.slot);
            hn = shape_normal(g, hit.p);
            m = load_mat(mat, g.idx);
            sr = Ray{hit.p + hn * shadow_off, normalize(kp.light_pos - hit.p)};
            ld = dist(kp.light_pos, hit.p);
        }
        const bool shadow = kp.useBVH ? packet_shadow_bvh(kp, nodes, geo_leaf, sr, ld, alive)
                                      : packet_shadow_brute(kp, geo_lin, sr, ld, alive);
        if (alive) alive = shade_bounce(kp, ray, hit.p, hn, m, shadow, acc, att, 1e-3f);
    }
    if (pc.active) store_px(kp, pc.r, pc.x, make_float4(acc.x, acc.y, acc.z, 1.0f));
}

// ---------------------------------------------------------------------------
// k_accel: the packet walk over the reference tree plus the exact-result
// accelerator (accel.h). Which reference leaves a lane enters is decided by
// the reference's own box test; inside them, conservative local boxes and a
// distance margin skip shapes that cannot win; every candidate carries its
// rank in the reference walk so that ties resolve exactly as the reference's
// strict "<" in walk order does (lexicographic minimum of (distance, rank)).
// Barycentric triangle test only (the default); Moller-Trumbore frames use
// k_packet.

struct AccelPtrs {
    const float4* __restrict__ anodes;  // 4 float4 per reference node (the root's entry test)
    const float4* __restrict__ prims;   // 4 float4 per prim (PrimRec)
    const float4* __restrict__ lnodes;  // 6 float4 per local inner node: both child boxes + codes, cones
    const float4* __restrict__ wnodes;  // 8 float4 per reference inner node: both children's exact + content boxes
    const int4* __restrict__ tleaf;     // per reference leaf: plain start, plain count, local root code
    const float4* __restrict__ titems;  // 2 float4 per scene-tree item: exact box of its reference leaf + range
    int troot;                          // scene-tree root code (kLocal|w), kNoChild: reference tree only
    int scene_stack;                    // stack entries a scene-tree walk may use (<= the walk's own cap)
    int nfew;                           // > 0: items are gated by a per-ray mask over nfew reference leaves
                                        //      whose exact boxes are titems[0 .. 2*nfew) (few_mask)
    int N;
    float origin_lim;                   // AccelHost::origin_lim
    int boxes_finite;                   // no reference node box holds a NaN (ray_aabb_fast)
    int split_max;                      // lane_walk_any: split walks of waves with <= this many rays (0: off)
    int split_g;                        // ... over groups of at most this many lanes (a power of two)
    const int* __restrict__ prim_shape; // shape index per prim slot (the winner's material)
    float mt_z[3];                      // AccelHost::mt_z (Moller-Trumbore per-ray padding)
};

constexpr bool kWide8 = RT_WIDE8 != 0;

// The closest hit so far: distance, rank in the reference walk, ray parameter and
// record slot. The hit point is o + t d, recomputed from t after the walk: the same
// float operations as where it was found, so the same bits (two registers fewer
// through the walks than keeping the point).
struct Best {
    float d;
    int seq;
    float t;
    int slot;
};

__device__ __forceinline__ V hit_point(const Ray& r, float t) { return r.o + t * r.d; }

__device__ __forceinline__ bool lex_better(float d, int seq, const Best& b) {
    return d < b.d || (d == b.d && seq < b.seq);
}

// gpu_shader.comp:242-328 for one candidate, taking the winner test early:
// the hit point and distance are computed exactly as the reference does, and
// the remaining (wall / barycentric) checks only run when the candidate could
// win. Same result as testing first and comparing after.
// Moller-Trumbore (gpu_shader.comp:170-195) with the same float operations as
// intersect(): t > 0 gives INNER at o + t d, whatever the triangle's facing.
__device__ __forceinline__ bool mt_hit(const float* f, const Ray& r, V& p, float& tt) {
    const V p1 = mk(f[4], f[5], f[6]), e1 = mk(f[7], f[8], f[9]), e2 = mk(f[10], f[11], f[12]);
    const V hh = cross(r.d, e2);
    const float a = dot(e1, hh);
    if (__builtin_fabsf(a) < 1e-5f) return false;
    const float fi = 1.0f / a;
    const V s = r.o - p1;
    const float u = fi * dot(s, hh);
    if (u < 0.0f || u > 1.0f) return false;
    const V q = cross(s, e1);
    const float v = fi * dot(r.d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = fi * dot(e2, q);
    if (!(t > 0.0f)) return false;
    p = hit_point(r, t);
    tt = t;
    return true;
}

// The barycentric terms of a PrimRec triangle (gpu_shader.comp:218-229): d00 and
// d11 recomputed as pack_geo computes them, d01 and the denominator stored.
__device__ __forceinline__ bool tri_inside(const float* f, V p) {
    const V e1 = mk(f[7], f[8], f[9]), e2 = mk(f[10], f[11], f[12]);
    const V tp = p - mk(f[4], f[5], f[6]);
    const float d20 = dot(tp, e1), d21 = dot(tp, e2);
    const float d00 = dot(e1, e1), d11 = dot(e2, e2);
    const float v = (d11 * d20 - f[13] * d21) / f[14];
    const float w = (d00 * d21 - f[13] * d20) / f[14];
    const float u = 1.0f - v - w;
    return !(u < 0.0f || v < 0.0f || w < 0.0f);
}

template <bool MT = false>
__device__ __forceinline__ void try_closest(const PrimRec& g, int slot, const Ray& r, Best& b) {
    const float* f = g.f;
    const int seq = g.st, type = prim_type(g);
    if (MT && type == 3) {
        V p;
        float t;
        if (!mt_hit(f, r, p, t)) return;
        const float d = dist(r.o, p);
        if (lex_better(d, seq, b)) b = Best{d, seq, t, slot};
        return;
    }
    if (type == 0) {
        V c = mk(f[0], f[1], f[2]);
        V oc = r.o - c;
        float aa = dot(r.d, r.d);
        float bb = 2.0f * dot(r.d, oc);
        float cc = dot(oc, oc) - f[3] * f[3];
        float D = bb * bb - 4.0f * aa * cc;
        if (D > 0.0f) {
            float t1 = (-bb - __builtin_sqrtf(D)) / (2.0f * aa);
            if (t1 > 0.0f) {
                V p = hit_point(r, t1);
                float d = dist(r.o, p);
                if (lex_better(d, seq, b)) b = Best{d, seq, t1, slot};
            }
        }
        return;
    }
    V n = mk(f[0], f[1], f[2]);
    const float np = dot(n, r.d);
    // INNER needs np > 0 and t = num / np > 0 (gpu_shader.comp:206-212,276-283):
    // both signs are known before the division, which only the survivors pay.
    if (!(np > 0.0f)) return;
    const float num = -(f[3] + dot(n, r.o));
    if (!(num > 0.0f)) return;
    const float t = num / np;
    if (!(t > 0.0f)) return;
    V p = hit_point(r, t);
    float d = dist(r.o, p);
    if (!lex_better(d, seq, b)) return;
    if (type == 2) {
        V lp = p - mk(f[4], f[5], f[6]);
        float up = dot(lp, mk(f[9], f[10], f[11]));
        float vp = dot(lp, mk(f[12], f[13], f[14]));
        if (up < 0.0f || up > f[7] || vp < 0.0f || vp > f[8]) return;
    } else if (type == 3) {
        if (!tri_inside(f, p)) return;
    }
    b = Best{d, seq, t, slot};
}

// Shadow candidate: an INNER hit nearer than lim (gpu_shader.comp:473-480).
template <bool MT = false>
__device__ __forceinline__ bool try_shadow(const PrimRec& g, const Ray& r, float lim) {
    const float* f = g.f;
    const int type = prim_type(g);
    if (MT && type == 3) {
        V p;
        float t;
        return mt_hit(f, r, p, t) && dist(r.o, p) < lim;
    }
    if (type == 0) {
        V c = mk(f[0], f[1], f[2]);
        V oc = r.o - c;
        float aa = dot(r.d, r.d);
        float bb = 2.0f * dot(r.d, oc);
        float cc = dot(oc, oc) - f[3] * f[3];
        float D = bb * bb - 4.0f * aa * cc;
        if (!(D > 0.0f)) return false;
        float t1 = (-bb - __builtin_sqrtf(D)) / (2.0f * aa);
        return t1 > 0.0f && dist(r.o, r.o + t1 * r.d) < lim;
    }
    V n = mk(f[0], f[1], f[2]);
    const float np = dot(n, r.d);
    if (!(np > 0.0f)) return false;  // signs first, as in try_closest
    const float num = -(f[3] + dot(n, r.o));
    if (!(num > 0.0f)) return false;
    const float t = num / np;
    if (!(t > 0.0f)) return false;
    V p = r.o + t * r.d;
    if (!(dist(r.o, p) < lim)) return false;
    if (type == 2) {
        V lp = p - mk(f[4], f[5], f[6]);
        float up = dot(lp, mk(f[9], f[10], f[11]));
        float vp = dot(lp, mk(f[12], f[13], f[14]));
        return !(up < 0.0f || up > f[7] || vp < 0.0f || vp > f[8]);
    }
    if (type == 3) return tri_inside(f, p);
    return true;
}

// Diagnostics (TIMED k_accel only): per-lane node steps and primitive tests.
struct WalkCount {
    unsigned nodes, tests;
    unsigned wnodes, wtests;  // wave iterations (TIMED diagnostics only): node steps, leaf-loop steps
};

// True in exactly one active lane: counts a wave-level iteration once.
__device__ __forceinline__ bool first_active() {
    return static_cast<int>(__lane_id()) == __builtin_ctzll(__ballot(1));
}

// Codes of the walk: a reference inner node k; kTopLeaf|k a reference leaf;
// kTopLeaf|kItem|i a scene-tree item; kLocal|j a wide node (local or scene
// tree); kLocal|kLeaf|start<<6|count a local leaf (start < 2^22, count < 64:
// bits 28-29 stay clear, so kTopLeaf and kItem are never set in a local code).
__device__ __forceinline__ int top_code(int k, int ia) { return ia < 0 ? static_cast<int>(kTopLeaf | k) : k; }

template <bool MT = false>
__device__ __forceinline__ rta::RayC ray_c(const Ray& r, const AccelPtrs& A) {
    rta::RayC c = rta::ray_consts(r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, A.origin_lim);
    if (MT) rta::mt_ray(c, r.o.x, r.o.y, r.o.z, A.mt_z);
    return c;
}

__device__ __forceinline__ bool box_enter(const rta::RayC& c, float4 lo, float4 hi, float tl, float& te) {
    return rta::box_enter(c, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, tl, te);
}

// Scene-tree item (accel.h, SceneTree): the exact box test of its reference
// leaf (gpu_shader.comp:364-377; NaN-free for the rays that take the scene
// tree), then its prim range.
__device__ __forceinline__ bool enter_item(const AccelPtrs& A, unsigned uc, const Ray& r, const V& inv, int& start,
                                           int& count) {
    const float4* q = A.titems + 2 * static_cast<size_t>(uc & 0x0fffffffu);
    const float4 e0 = q[0], e1 = q[1];
    start = __float_as_int(e0.w);
    count = __float_as_int(e1.w);
    return ray_aabb_fast(r.o, inv, mk(e0.x, e0.y, e0.z), mk(e1.x, e1.y, e1.z));
}

// Few-leaf scenes (<= 8 reference leaves): the exact box tests of all of them
// once per walk; items are then local-leaf codes with kItem set and the leaf's
// index in bits 3-5 (no item record load on the walk).
__device__ __forceinline__ unsigned few_mask(const AccelPtrs& A, const Ray& r, const V& inv) {
    unsigned fm = 0;
    for (int i = 0; i < A.nfew; ++i) {
        const float4 e0 = A.titems[2 * i], e1 = A.titems[2 * i + 1];
        if (ray_aabb_fast(r.o, inv, mk(e0.x, e0.y, e0.z), mk(e1.x, e1.y, e1.z))) fm |= 1u << i;
    }
    return fm;
}

// A ray walks the scene tree when one is built and its slab values cannot be
// NaN (aabb_fast_ok) and the padded tests are in their bounded mode (c.ix != 0).
__device__ __forceinline__ bool use_scene(const AccelPtrs& A, bool fast, const rta::RayC& c) {
    return A.troot != kNoChild && fast && c.ix != 0.0f;
}

// The root has no parent: its own exact box decides entry (gpu_shader.comp:386-395),
// then its content box.
__device__ __forceinline__ bool enter_root(const AccelPtrs& A, const Ray& r, const V& inv, const rta::RayC& c,
                                           float tl, int& code) {
    const float4* q = A.anodes + 4 * static_cast<size_t>(A.N - 1);
    const float4 e0 = q[0], e1 = q[1], c0 = q[2], c1 = q[3];
    float te;
    code = top_code(A.N - 1, __float_as_int(e0.w));
    return ray_aabb(r.o, inv, mk(e0.x, e0.y, e0.z), mk(e1.x, e1.y, e1.z)) &&
           (!(__float_as_int(c0.w) & 8) || box_enter(c, c0, c1, tl, te));
}

// Both children of a node in hand: which the lane enters and at what parameter.
// Reference inner node: the children's exact boxes with the GLSL test (the
// reference's own entry decision, evaluated at the parent), then their content
// boxes. Local inner node: padded child boxes and back-face cones.
struct Kids {
    int ca, cb;
    float ta, tb;
    bool ha, hb;
};

__device__ __forceinline__ Kids ref_kids(const AccelPtrs& A, unsigned uc, const Ray& r, const V& inv,
                                         const rta::RayC& c, float tl, bool in, bool fast) {
    const float4* q = A.wnodes + 8 * static_cast<size_t>(uc);
    const float4 ae0 = q[0], ae1 = q[1], ac0 = q[2], ac1 = q[3];
    const float4 be0 = q[4], be1 = q[5], bc0 = q[6], bc1 = q[7];
    Kids k;
    bool ea, eb;
    if (fast) {
        ea = ray_aabb_fast(r.o, inv, mk(ae0.x, ae0.y, ae0.z), mk(ae1.x, ae1.y, ae1.z));
        eb = ray_aabb_fast(r.o, inv, mk(be0.x, be0.y, be0.z), mk(be1.x, be1.y, be1.z));
    } else {
        ea = ray_aabb(r.o, inv, mk(ae0.x, ae0.y, ae0.z), mk(ae1.x, ae1.y, ae1.z));
        eb = ray_aabb(r.o, inv, mk(be0.x, be0.y, be0.z), mk(be1.x, be1.y, be1.z));
    }
    // content boxes evaluated unconditionally (no branch between the loads and their use)
    float ta, tb;
    const bool pa = box_enter(c, ac0, ac1, tl, ta), pb = box_enter(c, bc0, bc1, tl, tb);
    const bool fa = (__float_as_int(ac0.w) & 8) != 0, fb = (__float_as_int(bc0.w) & 8) != 0;
    k.ha = in & ea & (pa | !fa);
    k.hb = in & eb & (pb | !fb);
    k.ta = fa ? ta : 0.f;
    k.tb = fb ? tb : 0.f;
    k.ca = __float_as_int(ae0.w);
    k.cb = __float_as_int(ae1.w);
    return k;
}

// A wide local node (accel.h, build_wide): up to four children, stored as
// 11 float4 (lo.x[4], lo.y[4], lo.z[4], hi.x[4], hi.y[4], hi.z[4], cone
// axis x[4], y[4], z[4], cone threshold[4], child codes[4]). Returns the
// children sorted by entry parameter, misses last (key = +inf).
struct Kids4 {
    float t[4];
    int code[4];
};

__device__ __forceinline__ void cas(Kids4& k, int i, int j) {
    const bool sw = k.t[j] < k.t[i];
    const float ti = k.t[i], tj = k.t[j];
    const int ci = k.code[i], cj = k.code[j];
    k.t[i] = sw ? tj : ti;
    k.t[j] = sw ? ti : tj;
    k.code[i] = sw ? cj : ci;
    k.code[j] = sw ? ci : cj;
}

// Two children per packed instruction (v_pk_fma_f32, v_pk_mul_f32): the same
// fma / mul per component as rta::box_enter and rta::cone_culls.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// The barycentric accelerator's wide node, 8 float4 = 128 B (one cache line):
// the four children's boxes as six rows (lo.x of the four, lo.y, ... hi.z), one
// quantized back-face cone word per child (accel_math.h, cone_word; kConeNp
// marks a kNoPrune child: entered at parameter 0, no distance limit) and the
// child codes. Same slab operations as rta::box_enter; the cone test is one
// dot4 per child.
__device__ __forceinline__ void wide_pair_q(const rta::RayC& c, float tl, f2 lx, f2 ly, f2 lz, f2 hx, f2 hy, f2 hz,
                                            int w0, int w1, float& t0, float& t1, bool& h0, bool& h1) {
    const f2 ix = {c.ix, c.ix}, iy = {c.iy, c.iy}, iz = {c.iz, c.iz};
    const f2 ox = {-c.ox, -c.ox}, oy = {-c.oy, -c.oy}, oz = {-c.oz, -c.oz};
    const f2 x0 = fma2(lx, ix, ox), x1 = fma2(hx, ix, ox);
    const f2 y0 = fma2(ly, iy, oy), y1 = fma2(hy, iy, oy);
    const f2 z0 = fma2(lz, iz, oz), z1 = fma2(hz, iz, oz);
    const int w[2] = {w0, w1};
    float tn[2], tf[2], te[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool np = w[k] == rta::kConeNp;
        tn[k] = fmaxf(fmaxf(fminf(x0[k], x1[k]), fminf(y0[k], y1[k])), fmaxf(fminf(z0[k], z1[k]), 0.0f));
        const float tz = fmaxf(z0[k], z1[k]);
        tf[k] = fminf(fminf(fmaxf(x0[k], x1[k]), fmaxf(y0[k], y1[k])), np ? fminf(tz, INFINITY) : fminf(tz, tl));
        te[k] = np ? 0.0f : tn[k];
    }
    t0 = te[0];
    t1 = te[1];
    h0 = (tn[0] <= tf[0]) & !rta::cone_culls_q(w0, c.dq);
    h1 = (tn[1] <= tf[1]) & !rta::cone_culls_q(w1, c.dq);
}

#ifndef RT_MT_UNROLL
#define RT_MT_UNROLL 4  // MT wide_kids: children per unrolled step (r03j: 1 -> 4 car MT -15 %)
#endif
constexpr int kMtUnroll = RT_MT_UNROLL;

// Float `comp` of child `sl`'s box (0-2 lo.xyz, 3-5 hi.xyz) in wide record w:
// row comp, lane sl of the SoA records; float comp of the child's 16-float
// block in the MT records (wide_kids).
__host__ __device__ __forceinline__ float* wide_box_f(float4* lnodes, int rec, int w, int sl, int comp) {
    float* base = reinterpret_cast<float*>(lnodes + rec * static_cast<size_t>(w));
    return rec == kWideRecMt ? base + 16 * sl + comp : base + 4 * comp + sl;
}


template <bool MT = false>
__device__ __forceinline__ Kids4 wide_kids(const AccelPtrs& A, unsigned uc, const rta::RayC& c, float tl, bool in) {
    const float4* q = A.lnodes + (MT ? kWideRecMt : kWideRec) * static_cast<size_t>(uc & kRecMask);
    float t[4];
    bool h[4];
    int cc[4];
    if (MT) {
        // per-ray padding (accel_math.h mt_pad / mt_slab; accel_bound.h): each
        // child's static box grown by its pad, the distance limit by lf, then the
        // slab along its cone axis; a child without a finite bound is entered at 0.
        // Record: per child 4 float4 (lo.xyz hi.x | hi.yz axis.xy | axis.z s m0 m1 |
        // m2 m3 m4 m5), then the codes. Results select-written (kMtUnroll < 4 would
        // index them by a loop variable). Pairs of children on packed f32
        // instructions (as wide_pair_q) spilled 40-140 VGPRs in every MT instance (r03).
        const float4 cd = q[16];
        t[0] = t[1] = t[2] = t[3] = 0.0f;
        h[0] = h[1] = h[2] = h[3] = false;
        cc[0] = __float_as_int(cd.x), cc[1] = __float_as_int(cd.y), cc[2] = __float_as_int(cd.z);
        cc[3] = __float_as_int(cd.w);
#pragma unroll kMtUnroll
        for (int s2 = 0; s2 < 4; ++s2) {
            const float4 f0 = q[4 * s2], f1 = q[4 * s2 + 1], f2v = q[4 * s2 + 2], f3 = q[4 * s2 + 3];
            const float k[4] = {f1.z, f1.w, f2v.x, f2v.y};
            const float m[6] = {f2v.z, f2v.w, f3.x, f3.y, f3.z, f3.w};
            float pad, lf, q2, pt, ilf, tt = 0.0f;
            bool hh = true;
            // (r05: a wave-uniform floor case of mt_pad from per-child constants spilled
            // 28 VGPRs in the production MT instance: car MT frame 1.293 -> 1.455 ms in
            // flight, 1.577 without its slab; profiles/r05e_abf_floor*.json. Not kept.)
            const bool ok = rta::mt_pad(c, c.so, k, m, pad, lf, q2, pt, ilf);
            if (ok) {
                float tn, tf;
                hh = rta::box_span(c, f0.x - pad, f0.y - pad, f0.z - pad, f0.w + pad, f1.x + pad, f1.y + pad,
                                   tl * lf, tn, tf);
                if (hh && c.ix != 0.0f && m[5] < 3e38f)
                    hh = rta::mt_slab(c.mox, c.moy, c.moz, c.on, c, k, m, q2, pt, tn, tf);
                // the stack's prune compares with tl, not tl * lf: scaled by mt_pad's bound
                // ilf <= 1 / lf, not by a reciprocal (car MT -2.0 %, r04zz9)
                tt = tn * ilf;
            }
            // select-written (a lane-varying index would put t / h in scratch)
            t[0] = s2 == 0 ? tt : t[0], t[1] = s2 == 1 ? tt : t[1], t[2] = s2 == 2 ? tt : t[2];
            t[3] = s2 == 3 ? tt : t[3];
            h[0] = s2 == 0 ? hh : h[0], h[1] = s2 == 1 ? hh : h[1], h[2] = s2 == 2 ? hh : h[2];
            h[3] = s2 == 3 ? hh : h[3];
        }
    } else {
        const float4 lx = q[0], ly = q[1], lz = q[2], hx = q[3], hy = q[4], hz = q[5];
        const float4 cw = q[6], cd = q[7];
        cc[0] = __float_as_int(cd.x), cc[1] = __float_as_int(cd.y), cc[2] = __float_as_int(cd.z);
        cc[3] = __float_as_int(cd.w);
        wide_pair_q(c, tl, (f2){lx.x, lx.y}, (f2){ly.x, ly.y}, (f2){lz.x, lz.y}, (f2){hx.x, hx.y}, (f2){hy.x, hy.y},
                    (f2){hz.x, hz.y}, __float_as_int(cw.x), __float_as_int(cw.y), t[0], t[1], h[0], h[1]);
        wide_pair_q(c, tl, (f2){lx.z, lx.w}, (f2){ly.z, ly.w}, (f2){lz.z, lz.w}, (f2){hx.z, hx.w}, (f2){hy.z, hy.w},
                    (f2){hz.z, hz.w}, __float_as_int(cw.z), __float_as_int(cw.w), t[2], t[3], h[2], h[3]);
    }
    Kids4 k;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
        k.t[s2] = (h[s2] & (cc[s2] != kNoChild) & in) ? t[s2] : INFINITY;
        k.code[s2] = cc[s2];
    }
    return k;
}

__device__ __forceinline__ void sort4(Kids4& k) {
    cas(k, 0, 1);
    cas(k, 2, 3);
    cas(k, 0, 2);
    cas(k, 1, 3);
    cas(k, 1, 2);
}

// The second record of a kPair node (its children 4-7), or none: every child a miss.
template <bool MT = false>
__device__ __forceinline__ Kids4 wide_kids_hi(const AccelPtrs& A, unsigned uc, const rta::RayC& c, float tl, bool in) {
    Kids4 k;
    if (!MT && kWide8 && (uc & kPair)) return wide_kids<MT>(A, uc + 1u, c, tl, in);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
        k.t[s2] = INFINITY;
        k.code[s2] = kNoChild;
    }
    return k;
}

// Both records' children as one list sorted by entry parameter (19-comparator
// network), for the split walk's shared prologue.
struct Kids8 {
    float t[8];
    int code[8];
};
__device__ __forceinline__ Kids8 sort8(const Kids4& a, const Kids4& b) {
    Kids8 k;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
        k.t[s2] = a.t[s2], k.code[s2] = a.code[s2];
        k.t[4 + s2] = b.t[s2], k.code[4 + s2] = b.code[s2];
    }
    auto cx = [&](int i, int j) {
        const bool sw = k.t[j] < k.t[i];
        const float ti = k.t[i], tj = k.t[j];
        const int ci = k.code[i], cj = k.code[j];
        k.t[i] = sw ? tj : ti, k.t[j] = sw ? ti : tj;
        k.code[i] = sw ? cj : ci, k.code[j] = sw ? ci : cj;
    };
    cx(0, 1), cx(2, 3), cx(4, 5), cx(6, 7), cx(0, 2), cx(1, 3), cx(4, 6), cx(5, 7), cx(1, 2), cx(5, 6);
    cx(0, 4), cx(1, 5), cx(2, 6), cx(3, 7), cx(2, 4), cx(3, 5), cx(1, 2), cx(3, 4), cx(5, 6);
    return k;
}
__device__ __forceinline__ int pick_code8(const Kids8& k, int i) {
    int r = k.code[0];
#pragma unroll
    for (int s2 = 1; s2 < 8; ++s2) r = i == s2 ? k.code[s2] : r;
    return r;
}
__device__ __forceinline__ float pick_t8(const Kids8& k, int i) {
    float r = k.t[0];
#pragma unroll
    for (int s2 = 1; s2 < 8; ++s2) r = i == s2 ? k.t[s2] : r;
    return r;
}

// k.code[i] / k.t[i] for a lane-varying i (selects, no indexed registers)
__device__ __forceinline__ int pick_code(const Kids4& k, int i) {
    return i == 0 ? k.code[0] : i == 1 ? k.code[1] : i == 2 ? k.code[2] : k.code[3];
}
__device__ __forceinline__ float pick_t(const Kids4& k, int i) {
    return i == 0 ? k.t[0] : i == 1 ? k.t[1] : i == 2 ? k.t[2] : k.t[3];
}

// Stacked entry parameters are kept as bf16 rounded toward zero: never above
// the true value (te >= 0), so the pop-time prune only ever drops less.
__device__ __forceinline__ unsigned short f_bf16_down(float t) {
    return static_cast<unsigned short>(__float_as_uint(t) >> 16);
}
__device__ __forceinline__ float bf16_f(unsigned short b) { return __uint_as_float(static_cast<unsigned>(b) << 16); }

// Per-lane walk ("while-while"): each lane walks its own stack in LDS (code +
// entry parameter per entry). A lane descends until it holds a leaf, keeping
// the nearer child in registers and stacking the farther one; the wave then
// tests all lanes' leaves together. A stacked entry is dropped on pop when a
// nearer hit has been found since it was pushed.
//
// Split walks (sg > 1, lane_walk_any): the sg lanes of an aligned group walk one
// ray. From the root (a prologue before the main loop, so the loop's registers
// are not raised) they share a path (ss lanes, this lane the si-th) and test
// its nodes with a fixed limit (tl0), so every lane of the share sees
// the same children; a node with h hit children hands child p to the lanes
// si * h / ss == p (h < ss) or lane si the children si, si + ss, ... (h >= ss,
// its own from then on). Every child is walked by some lane, leaves of the
// shared part by all of them. The lanes' best distances are pooled after every
// round of leaf tests (and a shadow hit ends the group's walks); the result is
// the (distance, rank) minimum over the group, which does not depend on which
// lane tested which leaf.
// FLAT_SHADOW: a shadow hit sets the lane's flags and ends its leaf loop through the loop
// test, instead of returning from inside the loop (r03: car -1.7 % in flight and serially;
// config 5 +0.5 %, so the big-scene instances, which split walks, keep the return).
template <bool SHADOW, bool COUNT = false, bool WSTAT = false, bool MT = false, bool FLAT_SHADOW = false>
__device__ void lane_walk(const AccelPtrs& A, const Ray& r, bool active, float lim_shadow, Best& b, bool& shadow,
                          int* stk, unsigned short* stt, int stride, int cap, WalkCount& wc, int sg = 1,
                          int si = 0) {
    if (A.N <= 0 || !active) return;
    const V inv = inv_dir(r.d);
    const bool fast = A.boxes_finite && aabb_fast_ok(r.o, inv);
    const rta::RayC c = ray_c<MT>(r, A);
    float tl = rta::t_limit(SHADOW ? lim_shadow : b.d, c.rdl);
    // sp: the stack top as an element offset (entries x stride), so a push or pop
    // adds or subtracts stride instead of multiplying (v_mul_lo_u32 is quarter rate)
    int sp = 0, cur = A.troot;
    const int capo = cap * stride;
    bool have = true;
    // The scene tree has no static stack bound: a lane whose push would not fit
    // drops it and marks `ovf`; when its walk ends it walks the reference tree
    // from the root (with the best hit so far), whose bound the builder checked.
    bool ovf = false;
    int pcap = min(cap, A.scene_stack) * stride;  // push bound of the tree being walked (offset)
    unsigned fm = 0;
    if (!use_scene(A, fast, c)) {
        have = enter_root(A, r, inv, c, tl, cur);
        pcap = capo;
    } else if (A.nfew > 0) {
        fm = few_mask(A, r, inv);
    }
    int start = 0, count = 0;  // the leaf range this lane holds (reset after each round's tests)
    if (sg > 1) {
        // Split: the shared top of the tree, out of the main loop (whose registers it
        // does not add to). Shared nodes are tested with a fixed limit (tl0), so every
        // lane of a share (ss lanes, this the si-th) sees the same children.
        const float tl0 = SHADOW ? tl : INFINITY;
        int ss = sg;
        while (have && ss > 1) {
            const unsigned uc = static_cast<unsigned>(cur);
            if (uc & (kLeaf | kItem)) break;  // a leaf: the share tests it (and walks on) together
            if (COUNT) wc.nodes++;
            if (uc & kTopLeaf) {  // plain range + local root: hold the range, enter the root
                if (count > 0) break;
                const int4 lf = A.tleaf[uc & 0x0fffffffu];
                start = lf.x;
                count = lf.y;
                have = lf.z != kNoChild;
                cur = lf.z;
            } else if (uc & kLocal) {
                if constexpr (!MT && kWide8) {
                    // a kPair node: both records' children, sorted as one list of up to 8
                    const Kids8 w = sort8(wide_kids<MT>(A, uc, c, tl0, true), wide_kids_hi<MT>(A, uc, c, tl0, true));
                    int h = 0;
#pragma unroll
                    for (int s2 = 0; s2 < 8; ++s2) h += w.t[s2] < INFINITY;
                    if (h == 0) {
                        have = false;
                    } else if (h >= ss) {  // positions si, si + ss, ... (ss >= 2, h <= 8) are this lane's
                        for (int q = si + ss; q < h; q += ss) {
                            if (sp < pcap) {
                                stk[sp] = pick_code8(w, q);
                                stt[sp] = f_bf16_down(pick_t8(w, q));
                                sp += stride;
                            } else {
                                ovf = true;
                            }
                        }
                        cur = pick_code8(w, si);
                        ss = 1;
                    } else {  // child p, shared by the lanes [lo, hi) of this share
                        const int p = si * h / ss, lo = (p * ss + h - 1) / h, hi = ((p + 1) * ss + h - 1) / h;
                        cur = pick_code8(w, p);
                        si -= lo;
                        ss = hi - lo;
                    }
                } else {
                    Kids4 w = wide_kids<MT>(A, uc, c, tl0, true);
                    sort4(w);
                    const int h = (w.t[0] < INFINITY) + (w.t[1] < INFINITY) + (w.t[2] < INFINITY) + (w.t[3] < INFINITY);
                    if (h == 0) {
                        have = false;
                    } else if (h >= ss) {  // positions si and si + ss (ss >= 2, h <= 4) are this lane's
                        if (si + ss < h) {
                            if (sp < pcap) {
                                stk[sp] = pick_code(w, si + ss);
                                stt[sp] = f_bf16_down(pick_t(w, si + ss));
                                sp += stride;
                            } else {
                                ovf = true;
                            }
                        }
                        cur = pick_code(w, si);
                        ss = 1;
                    } else {  // child p, shared by the lanes [lo, hi) of this share
                        const int p = si * h / ss, lo = (p * ss + h - 1) / h, hi = ((p + 1) * ss + h - 1) / h;
                        cur = pick_code(w, p);
                        si -= lo;
                        ss = hi - lo;
                    }
                }
            } else {
                const Kids k = ref_kids(A, uc, r, inv, c, tl0, true, fast);
                if (k.ha && k.hb) {  // two children over ss >= 2 lanes
                    const bool a_first = !(k.tb < k.ta);
                    const int p = si * 2 / ss, lo = (p * ss + 1) / 2, hi = ((p + 1) * ss + 1) / 2;
                    cur = (p == 0) == a_first ? k.ca : k.cb;
                    si -= lo;
                    ss = hi - lo;
                } else if (k.ha || k.hb) {
                    cur = k.ha ? k.ca : k.cb;
                } else {
                    have = false;
                }
            }
        }
    }
    // From here `cur == kNoChild` means the lane holds no node (no separate flag: one
    // lane mask fewer to merge at every join of the descent)
    if (!have) cur = kNoChild;
    bool ended = false;
    for (;;) {
        // While-while, speculative: a lane descends until it holds a leaf, then keeps
        // walking inner nodes while any other lane is still looking for one; a lane
        // that meets a second leaf parks on it (kept for the next round), and the
        // round ends when every walking lane holds a leaf (measured: config 3 -4 %,
        // config 5 -14 %).
        // One-exit form: a lane that finishes, parks or ends its walk sets `stop`
        // instead of leaving the loop, and the round ends on the wave-uniform test alone
        // (fewer lane-mask merges per step; r03: config 5 -3 %). Ended lanes are
        // stopped: no exec test around the loop (config 5: -2 %).
        bool stop = ended;
        for (;;) {
            if (__ballot(!stop && count == 0) == 0) break;
            if (!stop && cur == kNoChild) {
                if (sp == 0) {
                    if (ovf) {  // a scene-tree push was dropped: the reference tree, from its root
                        ovf = false;
                        pcap = capo;
                        if (!enter_root(A, r, inv, c, tl, cur)) cur = kNoChild;
                    }
                    if (cur == kNoChild) {
                        ended = count == 0;  // walk finished (a held leaf is still tested)
                        stop = true;
                    }
                } else {
                    sp -= stride;
                    const int pc = stk[sp];
                    cur = bf16_f(stt[sp]) > tl ? kNoChild : pc;  // dropped if a nearer hit was found since the push
                }
            }
            const unsigned uc = static_cast<unsigned>(cur);
            stop = stop || (cur != kNoChild && count > 0 && (uc & (kTopLeaf | kLeaf)));  // park on a leaf
            if (stop || cur == kNoChild) continue;
            if (COUNT) wc.nodes++;
            if (WSTAT && first_active()) wc.wnodes++;
            cur = kNoChild;  // the branches below set the next node, if any
            // kLocal codes (wide nodes and local leaves, including few-leaf items) first,
            // as one region: a round in which no lane holds a reference-tree code skips
            // the rest with one exec test instead of three
            if (uc & kLocal) {
                if (uc & kLeaf) {
                    start = static_cast<int>((uc >> 6) & 0x3fffffu);
                    count = static_cast<int>(uc & 0x3fu);
                    if (uc & kItem) count = ((fm >> (count >> 3)) & 1u) ? (count & 7) : 0;  // few-leaf item
                } else {
                    auto push = [&](float t, int code) {
                        if (t < INFINITY) {
                            if (sp < pcap) {
                                stk[sp] = code;
                                stt[sp] = f_bf16_down(t);
                                sp += stride;
                            } else {
                                ovf = true;  // scene tree only: local trees fit their bound
                            }
                        }
                    };
                    // a node of two records (kPair): the second record's children first,
                    // sorted, its 2nd-4th stacked; then the first record's; the nearer of
                    // the two records' nearest is walked, the other stacked last. One
                    // record's values live at a time (the walk is at the VGPR cap).
                    const bool pair = !MT && kWide8 && (uc & kPair);
                    float vt = INFINITY;
                    int vc = kNoChild;
                    if (pair) {
                        Kids4 v = wide_kids<MT>(A, uc + 1u, c, tl, true);
                        sort4(v);
#pragma unroll
                        for (int s2 = 3; s2 >= 1; --s2) push(v.t[s2], v.code[s2]);
                        vt = v.t[0];
                        vc = v.code[0];
                    }
                    Kids4 w = wide_kids<MT>(A, uc, c, tl, true);
                    sort4(w);
#pragma unroll
                    for (int s2 = 3; s2 >= 1; --s2) push(w.t[s2], w.code[s2]);
                    if (pair) {
                        const bool vf = vt < w.t[0];
                        push(vf ? w.t[0] : vt, vf ? w.code[0] : vc);
                        w.t[0] = vf ? vt : w.t[0];
                        w.code[0] = vf ? vc : w.code[0];
                    }
                    if (w.t[0] < INFINITY) cur = w.code[0];
                }
            } else if ((uc & (kTopLeaf | kItem)) == (kTopLeaf | kItem)) {
                int s0, n0;
                if (enter_item(A, uc, r, inv, s0, n0)) {
                    start = s0;
                    count = n0;
                }
            } else if (uc & kTopLeaf) {
                const int4 lf = A.tleaf[uc & 0x0fffffffu];
                start = lf.x;
                count = lf.y;
                cur = lf.z;  // the local root (kNoChild: none) is entered with the leaf
            } else {
                const Kids k = ref_kids(A, uc, r, inv, c, tl, true, fast);
                if (k.ha && k.hb) {
                    const bool a_first = !(k.tb < k.ta);  // nearer entry first
                    if (sp < capo) {
                        stk[sp] = a_first ? k.cb : k.ca;
                        stt[sp] = f_bf16_down(a_first ? k.tb : k.ta);
                        sp += stride;
                    }
                    cur = a_first ? k.ca : k.cb;
                } else if (k.ha || k.hb) {
                    cur = k.ha ? k.ca : k.cb;
                }
            }
        }
        if (__ballot(count > 0) == 0) return;  // every lane's walk finished
        for (int i = 0; i < count; ++i) {
            const PrimRec g = load_prim(A.prims, start + i);
            if (COUNT) wc.tests++;
            if (WSTAT && first_active()) wc.wtests++;
            if (SHADOW && FLAT_SHADOW) {
                // an occluder ends this lane's walk at the next round's test (no exit
                // from inside the loop)
                if (try_shadow<MT>(g, r, lim_shadow)) {
                    shadow = true;
                    ended = true;
                    count = i + 1;
                }
            } else if (SHADOW) {
                if (try_shadow<MT>(g, r, lim_shadow)) {
                    shadow = true;
                    if (sg == 1) return;
                    ended = true;  // split: the group learns it below
                    break;
                }
            } else {
                try_closest<MT>(g, start + i, r, b);
            }
        }
        count = 0;
        if (sg > 1) {  // every lane of the wave's groups is here (the returns above are wave-uniform)
            if (SHADOW) {
                int any = shadow ? 1 : 0;
                for (int o = 1; o < sg; o <<= 1) any |= __shfl_xor(any, o);
                if (any) {
                    shadow = true;
                    ended = true;
                }
            } else {
                float d = b.d;
                for (int o = 1; o < sg; o <<= 1) d = fminf(d, __shfl_xor(d, o));
                tl = rta::t_limit(d, c.rdl);
            }
        } else if (!SHADOW) {
            tl = rta::t_limit(b.d, c.rdl);
        }
    }
}

// lane_walk for a wave's rays. A wave with few rays (at most A.split_max, e.g. the
// reflections of a tile where little is a mirror) gives each ray a group of idle
// lanes that split its walk (lane_walk, sg > 1): the longest walk of the wave gets
// shorter, and the wave issues fewer rounds. The group's result is the lexicographic
// (distance, rank) minimum of its lanes' -- the same hit as one lane's whole walk.
// One lane_walk either way (one copy of the walk in the kernel). b must hold the
// same value in every lane (bounce_step's fresh best); on return it holds each
// active lane's result and r each active lane's own ray (both are rebuilt from the
// group, so neither is live across the walk).
// SPLIT = false compiles the plain walk alone: the split's registers spill in the
// car's production kernel (+8 % per frame there, r02m), so only the kernels of
// big scenes (the compacting k_accel instance and k_accel_tail) carry it.
template <bool SHADOW, bool COUNT = false, bool WSTAT = false, bool MT = false, bool SPLIT = true>
__device__ __forceinline__ void lane_walk_any(const AccelPtrs& A, Ray& r, bool active, float lim_shadow, Best& b,
                                              bool& shadow, int* stk, unsigned short* stt, int stride, int cap,
                                              WalkCount& wc) {
    if (!SPLIT) {  // the plain walk, without the split's registers
        lane_walk<SHADOW, COUNT, WSTAT, MT, true>(A, r, active, lim_shadow, b, shadow, stk, stt, stride, cap, wc);
        return;
    }
    const unsigned long long m = __ballot(active);
    const int n = __popcll(m);
    int G = 1;
    while (G < A.split_g && 2 * G * n <= 64) G *= 2;
    if (n == 0 || n > A.split_max) G = 1;  // wave-uniform
    const int lane = lane_id();
    int src = lane;  // the ray this lane walks
    bool walk = active;
    if (G > 1) {
        const int j = lane / G;
        int q = 0;  // the j-th ray of the wave (wave-uniform loop over m's bits)
        for (unsigned long long mm = m; mm; mm &= mm - 1ull, ++q)
            if (q == j) src = __builtin_ctzll(mm);
        walk = j < n;
    }
    Ray rr{mk(__shfl(r.o.x, src), __shfl(r.o.y, src), __shfl(r.o.z, src)),
           mk(__shfl(r.d.x, src), __shfl(r.d.y, src), __shfl(r.d.z, src))};
    const float ls = __shfl(lim_shadow, src);
    bool sh = false;
    lane_walk<SHADOW, COUNT, WSTAT, MT>(A, rr, walk, ls, b, sh, stk, stt, stride, cap, wc, G, lane % G);
    // the group lane holding this lane's result (recomputed here: nothing extra live through the walk)
    const int from = G > 1 ? G * __popcll(__ballot(active) & ((1ull << lane) - 1ull)) : lane;
    if (SHADOW) {
        int any = sh ? 1 : 0;
        for (int o = 1; o < G; o <<= 1) any |= __shfl_xor(any, o);
        any = __shfl(any, from);
        if (active && any) shadow = true;
    } else {
        for (int o = 1; o < G; o <<= 1) {
            const float d = __shfl_xor(b.d, o);
            const int sq = __shfl_xor(b.seq, o), sl = __shfl_xor(b.slot, o);
            const float tt = __shfl_xor(b.t, o);
            if (lex_better(d, sq, b)) b = Best{d, sq, tt, sl};
        }
        b = Best{__shfl(b.d, from), __shfl(b.seq, from), __shfl(b.t, from), __shfl(b.slot, from)};
        r = Ray{mk(__shfl(rr.o.x, from), __shfl(rr.o.y, from), __shfl(rr.o.z, from)),
                mk(__shfl(rr.d.x, from), __shfl(rr.d.y, from), __shfl(rr.d.z, from))};
    }
}

// Packet walk: one wave-uniform walk with a 64-bit lane mask per stack entry
// (VGPR-resident stack, scalar node loads). The reference's walk order does
// not depend on the ray, so one walk with masks reproduces every lane's own;
// the order among children follows the first lane that enters both.
template <bool SHADOW, bool COUNT = false, bool WSTAT = false, bool MT = false>
__device__ void packet_walk(const AccelPtrs& A, const Ray& r, bool active, float lim_shadow, Best& b,
                            bool& shadow, WalkCount& wc) {
    unsigned long long m = __ballot(active);
    if (A.N <= 0 || m == 0) return;
    const V inv = inv_dir(r.d);
    const bool fast = A.boxes_finite && aabb_fast_ok(r.o, inv);
    const rta::RayC c = ray_c<MT>(r, A);
    float tl = rta::t_limit(SHADOW ? lim_shadow : b.d, c.rdl);
    WaveStack st{0, 0, 0, 0};
    int cur = 0;
    unsigned long long ovf = 0;  // lanes whose scene-tree pushes were dropped (see lane_walk)
    unsigned fm = 0;             // few-leaf mask (few_mask)
    int pcap = kMaxStack;        // push bound of the tree being walked (uniform)
    {
        int code = 0;
        const bool scene = use_scene(A, fast, c);
        const bool hr = enter_root(A, r, inv, c, tl, code);  // code is the same in every lane
        const unsigned long long mr = __ballot(active && !scene && hr), ms = __ballot(active && scene);
        if (ms && A.nfew > 0) fm = few_mask(A, r, inv);
        cur = uni(code);
        m = mr;
        if (ms) {  // scene-tree lanes first; reference-tree lanes (if any) follow as if overflowed
            ovf = mr;
            cur = A.troot;
            m = ms;
            pcap = min(kMaxStack, A.scene_stack);
        }
    }
    unsigned long long done = 0;
    for (;;) {
        if (m == 0) {
            if (st.sp == 0) {
                if (!ovf) return;
                // scene-tree pushes were dropped for the lanes in ovf: they walk the
                // reference tree from its root (with their best hits so far)
                int code = 0;
                const bool hr = enter_root(A, r, inv, c, tl, code);
                m = __ballot(lane_in(ovf) && hr) & ~done;
                ovf = 0;
                pcap = kMaxStack;
                cur = uni(code);
                continue;
            }
            st.pop(cur, m);
            cur = uni(cur);
            if (SHADOW) m &= ~done;
            continue;
        }
        if (COUNT && lane_in(m)) wc.nodes++;
        if (WSTAT) wc.wnodes += lane_id() == 0 ? 1u : 0u;
        const unsigned uc = static_cast<unsigned>(cur);
        Kids k{0, 0, 0.f, 0.f, false, false};
        int start = 0, count = 0;
        bool item_in = true;
        if ((uc & (kTopLeaf | kItem)) == (kTopLeaf | kItem)) {
            item_in = enter_item(A, uc, r, inv, start, count);
            start = uni(start);
            count = uni(count);
        } else if (uc & kTopLeaf) {
            const int4 lf = A.tleaf[uc & 0x0fffffffu];
            start = uni(lf.x);
            count = uni(lf.y);
            k.ca = uni(lf.z);
            k.ha = (k.ca != kNoChild) && lane_in(m);  // local root: entered with the leaf
        } else if (uc & kLeaf) {
            start = static_cast<int>((uc >> 6) & 0x3fffffu);
            count = static_cast<int>(uc & 0x3fu);
            if (uc & kItem) {  // few-leaf item
                item_in = (fm >> (count >> 3)) & 1u;
                count &= 7;
            }
        } else if (uc & kLocal) {
            // wide node: children ordered by the entry parameters of the first lane
            // that enters any of them; the rest pushed far to near
            // a kPair node (uniform): both records' children, up to 8
            constexpr int NK = !MT && kWide8 ? 8 : 4;
            Kids4 wk[2];
            wk[0] = wide_kids<MT>(A, uc, c, tl, lane_in(m));
            if (NK == 8) wk[1] = wide_kids_hi<MT>(A, uc, c, tl, lane_in(m));
            unsigned long long wm[NK];
            float key[NK];
            int code[NK];
            unsigned long long any = 0;
#pragma unroll
            for (int s2 = 0; s2 < NK; ++s2) {
                wm[s2] = __ballot(wk[s2 >> 2].t[s2 & 3] < INFINITY);
                any |= wm[s2];
            }
            const int rep = any ? __builtin_ctzll(any) : 0;
#pragma unroll
            for (int s2 = 0; s2 < NK; ++s2) {
                const Kids4& w = wk[s2 >> 2];
                key[s2] = wm[s2] ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.t[s2 & 3]), rep)) : INFINITY;
                code[s2] = uni(w.code[s2 & 3]);
                if (wm[s2] && !(key[s2] < INFINITY)) key[s2] = 3.0e38f;  // the representative lane misses it
            }
#define RT_CAS3(i, j)                                                                   \
    if (key[j] < key[i]) {                                                              \
        const float t_ = key[i]; key[i] = key[j]; key[j] = t_;                          \
        const int c_ = code[i]; code[i] = code[j]; code[j] = c_;                        \
        const unsigned long long m_ = wm[i]; wm[i] = wm[j]; wm[j] = m_;                 \
    }
            if (NK == 8) {
                RT_CAS3(0, 1) RT_CAS3(2, 3) RT_CAS3(4, 5) RT_CAS3(6, 7) RT_CAS3(0, 2) RT_CAS3(1, 3) RT_CAS3(4, 6)
                RT_CAS3(5, 7) RT_CAS3(1, 2) RT_CAS3(5, 6) RT_CAS3(0, 4) RT_CAS3(1, 5) RT_CAS3(2, 6) RT_CAS3(3, 7)
                RT_CAS3(2, 4) RT_CAS3(3, 5) RT_CAS3(1, 2) RT_CAS3(3, 4) RT_CAS3(5, 6)
            } else {
                RT_CAS3(0, 1) RT_CAS3(2, 3) RT_CAS3(0, 2) RT_CAS3(1, 3) RT_CAS3(1, 2)
            }
#undef RT_CAS3
#pragma unroll
            for (int s2 = NK - 1; s2 >= 1; --s2)
                if (wm[s2]) {
                    if (st.sp < pcap) st.push(code[s2], wm[s2]);
                    else ovf |= wm[s2];  // scene tree only: local trees fit their bound
                }
            cur = code[0];
            m = wm[0];
            continue;
        } else {
            k = ref_kids(A, uc, r, inv, c, tl, lane_in(m), fast);
            k.ca = uni(k.ca);
            k.cb = uni(k.cb);
        }
        if (count > 0) {
            bool live = lane_in(m) && item_in;
            for (int i = 0; i < count; ++i) {
                const PrimRec g = load_prim(A.prims, start + i);
                if (WSTAT) wc.wtests += lane_id() == 0 ? 1u : 0u;
                if (live) {
                    if (COUNT) wc.tests++;
                    if (SHADOW) {
                        if (try_shadow<MT>(g, r, lim_shadow)) {
                            shadow = true;
                            live = false;
                        }
                    } else {
                        try_closest<MT>(g, start + i, r, b);
                    }
                }
                if (SHADOW && __ballot(live) == 0) break;
            }
            if (SHADOW) {
                done = __ballot(shadow);
                if (k.ha && shadow) k.ha = false;
            } else {
                tl = rta::t_limit(b.d, c.rdl);
            }
        }
        const unsigned long long ma = __ballot(k.ha), mb = __ballot(k.hb);
        if (ma && mb) {
            // near first for the wave: the child the first lane of both masks enters sooner
            const int rep = __builtin_ctzll(ma & mb ? (ma & mb) : ma);
            const float ra = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k.ta), rep));
            const float rb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k.tb), rep));
            const bool a_first = !(rb < ra);
            if (st.sp < kMaxStack) st.push(a_first ? k.cb : k.ca, a_first ? mb : ma);
            cur = a_first ? k.ca : k.cb;
            m = a_first ? ma : mb;
        } else if (ma) {
            cur = k.ca;
            m = ma;
        } else if (mb) {
            cur = k.cb;
            m = mb;
        } else {
            m = 0;
        }
    }
}

// One 8x8 tile per wave (lane l: pixel (l&7, l>>3) of the tile).
__device__ __forceinline__ PixelCoord tile_pixel(const KParams& kp, int tile) {
    const int lane = threadIdx.x & 63;
    PixelCoord pc;
    pc.x = (tile % kp.tiles_x) * 8 + (lane & 7);
    pc.r = (tile / kp.tiles_x) * 8 + (lane >> 3);
    pc.active = pc.x < kp.width && pc.r < kp.out_rows;
    pc.y = pc.active ? image_row(kp, pc.r) : 0;
    pc.active = pc.active && pc.y < kp.height;
    return pc;
}

// Diagnostics (TIMED k_accel): one record of kTileRec u64 per tile:
//   [0] start, [1] end (100 MHz wall clock), [2] node steps and [3] tests
//   summed over the wave's lanes, [4], [5] their per-lane maxima,
//   [6 + s] wave clock ticks and [14 + s] node steps summed over lanes of walk
//   slot s = 2 * bounce + (0 closest, 1 shadow), bounce < 4, [22] leaf-loop and
//   [23] node-step iterations of the wave (all walks).
constexpr int kTileRec = 24;

// Ray compaction (rt_set_tail): queue entries per 64x64-pixel region.
constexpr int kTailRegion = 64 * 64;

// Cost-ordered dispatch (rt_set_schedule, k_tile_order): 32 half-octave
// buckets of a tile's work; the render kernel counts them per group of
// kOrderThreads tiles (one k_tile_order workgroup each).
constexpr int kOrderBuckets = 32, kOrderThreads = 256;
// lane_walk_any defaults (rt_debug_split)
constexpr int kSplitMax = 16, kSplitGroup = 8;
constexpr int kMtWalkFrom = 1 << 16;      // auto walk policy of Moller-Trumbore frames: all packets
constexpr int kMtPacketMaxNodes = 1024;  // ... over reference trees of fewer nodes (walk_from)
// the heaviest tiles of the cost order as several waves (rt_debug_heavy)
constexpr int kHeavyTiles = -1, kHeavyParts = 4;  // -1: auto (dispatch_plan.h, heavy_split)
constexpr unsigned kXcds = 8;  // MI355X: 8 XCDs, workgroups dealt round-robin

__device__ __forceinline__ int work_bucket(unsigned c) {
    if (c < 2u) return 0;
    const int l = 31 - __builtin_clz(c);  // >= 1
    return min(kOrderBuckets - 1, 2 * l - 1 + static_cast<int>((c >> (l - 1)) & 1u));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ void walk_rec(unsigned long long* rec, int slot, const WalkCount& before,
                                         const WalkCount& after, unsigned long long ticks) {
    if (!rec || slot >= 8) return;
    const unsigned long long n = wave_sum(after.nodes - before.nodes);
    if ((threadIdx.x & 63) == 0) {
        rec[6 + slot] = ticks;
        rec[14 + slot] = n;
    }
}

// One bounce of gpu_shader.comp:450-517 for a wave's rays: closest hit, background
// on a miss, the shadow ray, then Phong and the mirror ray (shade_bounce).
// bg_y() gives the lane's image row (recomputed, not kept live through the walks).
template <bool COUNT, bool COST, bool MT, bool SPLIT, class BgY>
__device__ __forceinline__ void bounce_step(const AccelPtrs& A, const float4* __restrict__ mat, const KParams& kp,
                                            int depth, Ray& ray, bool& alive, V& acc, V& att, BgY bg_y, int* stk,
                                            unsigned short* stt, int cap, WalkCount& wc, unsigned long long* rec,
                                            int lane_from, int shadow_from) {
    Best best{1e20f, 0x7fffffff, 0.f, -1};
    bool unused = false;
    const bool lane_mode = depth >= lane_from;  // wave-uniform
    WalkCount w0 = wc;
    unsigned long long c0 = COUNT ? clock64() : 0;
    if (lane_mode)
        lane_walk_any<false, COST || COUNT, COUNT, MT, SPLIT>(A, ray, alive, 0.f, best, unused, stk, stt, blockDim.x,
                                                              cap, wc);
    else
        packet_walk<false, COST || COUNT, COUNT, MT>(A, ray, alive, 0.f, best, unused, wc);
    if (COUNT) walk_rec(rec, 2 * depth, w0, wc, clock64() - c0);
    if (alive && best.slot < 0) {
        acc = acc + mulv(att, background(kp, bg_y()));
        alive = false;
    }
    // The shadow ray; the hit's normal and material are fetched again after the
    // shadow walk rather than kept live through it (register pressure).
    Ray sr{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
    float ld = 0.f;
    if (alive) {
        const V hp = hit_point(ray, best.t);
        const V hn = shape_normal(load_prim(A.prims, best.slot), hp);
        sr = Ray{hp + hn * kp.shadow_off, normalize(kp.light_pos - hp)};
        ld = dist(kp.light_pos, hp);
    }
    bool shadow = false;
    Best dummy{0.f, 0, 0.f, -1};
    w0 = wc;
    c0 = COUNT ? clock64() : 0;
    if (depth >= shadow_from)
        lane_walk_any<true, COST || COUNT, COUNT, MT, SPLIT>(A, sr, alive, gmin(ld, 1e20f), dummy, shadow, stk, stt,
                                                             blockDim.x, cap, wc);
    else
        packet_walk<true, COST || COUNT, COUNT, MT>(A, sr, alive, gmin(ld, 1e20f), dummy, shadow, wc);
    if (COUNT) walk_rec(rec, 2 * depth + 1, w0, wc, clock64() - c0);
    if (alive) {
        const PrimRec g = load_prim(A.prims, best.slot);
        const V hp = hit_point(ray, best.t);
        alive = shade_bounce(kp, ray, hp, shape_normal(g, hp), load_mat(mat, A.prim_shape[best.slot]), shadow, acc,
                             att, 1e-3f);
    }
}

// Walk counts (node steps, tests) are kept when COST: they are the cost that
// orders a later dispatch (rt_set_schedule). COUNT adds the per-walk records.
// SS: a supersampled frame (rt_set_samples): kp describes the sample frame, and the store
// writes the mean of each kp.ss x kp.ss block of lanes (store_px_ss) instead of every lane.
template <bool COUNT, bool COST = true, bool TAIL = false, bool MT = false, bool QUEUE = TAIL, bool SS = false,
          bool DISP = false>
__device__ void accel_tile(const AccelPtrs& A, const float4* __restrict__ mat, const KParams& kp, int tile,
                           int part, int* stk, unsigned short* stt, int cap, WalkCount& wc,
                           unsigned long long* rec, bool heavy) {
    // the heaviest slots (lane_k) may walk their camera rays / shadows per lane (lane_k_mode)
    const int lane_from = heavy && (kp.lane_k_mode & 1) ? 0 : kp.lane_from_depth;
    const int shadow_from = heavy && (kp.lane_k_mode & 2) ? 0 : kp.shadow_lane_from;
    // part > 0: this wave renders band part - 1 of the tile (64 / heavy_parts lanes)
    const bool mine = part == 0 || ((threadIdx.x & 63) * kp.heavy_parts >> 6) == part - 1;
    // Pixel coordinates and the background are recomputed where needed rather than
    // kept live through the walks (register pressure: they would be spilled).
    Ray ray;
    bool alive;
    {
        const PixelCoord pc = tile_pixel(kp, tile);
        ray = primary_ray(kp, pc.x, pc.y);
        alive = pc.active && mine;
    }
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    bool deferred = false;  // the lane's remaining bounces run in k_accel_tail
    if (kp.root_ok) {
        // The root's exact test (gpu_shader.comp:386-395) from the kernel arguments: a camera
        // ray that misses it hits nothing in any walk (every leaf box lies inside the root's
        // for the scene tree; the reference walk starts there), so it takes the background
        // without the walk's dependent loads -- the sky tiles of a frame. root_ok 2: the
        // boxes were grown on the device (rt_animate), read the root's from anodes.
        V rlo = mk(kp.root_lo[0], kp.root_lo[1], kp.root_lo[2]), rhi = mk(kp.root_hi[0], kp.root_hi[1], kp.root_hi[2]);
        if (kp.root_ok == 2) {
            const float4 a = A.anodes[4 * static_cast<size_t>(A.N - 1)], b = A.anodes[4 * static_cast<size_t>(A.N - 1) + 1];
            rlo = mk(a.x, a.y, a.z);
            rhi = mk(b.x, b.y, b.z);
        }
        const bool in = ray_aabb(ray.o, inv_dir(ray.d), rlo, rhi);
        if (alive && !in) {
            acc = background(kp, tile_pixel(kp, tile).y);
            alive = false;
        }
    }
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        if (__ballot(alive) == 0) break;
        bounce_step<COUNT, COST, MT, TAIL>(A, mat, kp, depth, ray, alive, acc, att,
                                           [&]() { return tile_pixel(kp, tile).y; }, stk, stt, cap, wc, rec,
                                           lane_from, shadow_from);
        if (TAIL && QUEUE && depth + 1 == kp.tail_from && __popcll(__ballot(alive)) <= kp.tail_max_lanes) {
            // Compaction: the rays still alive go to the tail queue (one atomic per wave)
            // per 64x64-pixel region (8x8 tiles), so a tail wave's rays come from one area
            const unsigned long long m = __ballot(alive);
            if (m) {
                const int rid = (tile / kp.tiles_x / 8) * kp.tail_rx + (tile % kp.tiles_x) / 8;
                int base = 0;
                if ((threadIdx.x & 63) == 0) base = rid * kTailRegion + atomicAdd(kp.tail_count + rid, __popcll(m));
                base = __shfl(base, 0);
                if (alive) {
                    const int lane = threadIdx.x & 63;
                    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                    const PixelCoord pc = tile_pixel(kp, tile);
                    float4* q = kp.tail_queue + 3 * static_cast<size_t>(pos);
                    q[0] = make_float4(ray.o.x, ray.o.y, ray.o.z, acc.x);
                    q[1] = make_float4(ray.d.x, ray.d.y, ray.d.z, acc.y);
                    q[2] = make_float4(att.x, att.y, att.z, acc.z);
                    // unsigned, as k_accel_tail decodes it (launch() keeps width * rows < 2^32)
                    kp.tail_px[pos] = static_cast<int>(static_cast<unsigned>(pc.r) * static_cast<unsigned>(kp.width) +
                                                       static_cast<unsigned>(pc.x));
                }
            }
            deferred = alive;
            break;
        }
    }
    const PixelCoord pc = tile_pixel(kp, tile);
    if (SS) {
        // The box filter of rt_set_samples (include/rt_api.h), in its fixed order: an xor
        // butterfly over the lane bits of x (0..2), then of y (3..5), log2 n rounds each, so
        // every lane of an n x n block ends with the block's sum (addition commutes: the same
        // bits in each). Lanes outside the frame or not of this band hold zeros, and a block
        // lies wholly inside or outside both (launch() splits only into bands of whole blocks).
        for (int b = 1; b < kp.ss; b <<= 1)
            acc = acc + mk(__shfl_xor(acc.x, b), __shfl_xor(acc.y, b), __shfl_xor(acc.z, b));
        for (int b = 8; b < 8 * kp.ss; b <<= 1)
            acc = acc + mk(__shfl_xor(acc.x, b), __shfl_xor(acc.y, b), __shfl_xor(acc.z, b));
        const int lane = threadIdx.x & 63;
        const float w = 1.0f / static_cast<float>(kp.ss * kp.ss);  // a power of two: exact
        if (pc.active && mine && ((lane | lane >> 3) & (kp.ss - 1)) == 0)
            store_px_ss<DISP ? kStoreDisplay : kStoreFloat>(kp, pc.r, pc.x,
                                                            make_float4(acc.x * w, acc.y * w, acc.z * w, 1.0f));
        return;
    }
    if (pc.active && mine && !deferred)
        store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, pc.r, pc.x, make_float4(acc.x, acc.y, acc.z, 1.0f));
}

// One dispatch slot per wave. TIMED writes each tile's start/end wall clock and
// walk counts (diagnostics only). At most 128 VGPRs: four waves per SIMD, which
// the LDS stacks also fit (accel.h, kLaneStack).
#ifndef RT_ACCEL_ATTR
#define RT_ACCEL_ATTR __attribute__((amdgpu_waves_per_eu(4)))
#endif
// COST = false: no walk counters (their registers: 12 -> 3 spilled VGPRs). REC: the
// dispatch records each tile's cost for the next order (rt_set_schedule); without COST
// it can only record the wall-time cost (kp.cost_time), which needs no counters.
// TAIL: queue the rays alive after bounce tail_from - 1 for k_accel_tail (rt_set_tail).
// SS: the supersampling instances (rt_set_samples): the same tiles over the sample frame,
// each n x n block of lanes stored as one mean pixel (accel_tile).
// DISP: the instance's twin for the display formats (RT_FORMAT_RGBA8, SRGBA8, RGBA16F: StoreKind
// in rt_device.h); accel_kernel() takes it from kAccelTable.
template <bool TIMED, bool COST = true, bool TAIL = false, bool MT = false, bool REC = COST, bool QUEUE = TAIL,
          bool SS = false, bool DISP = false>
__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_accel(AccelPtrs A, const float4* __restrict__ mat, KParams kp) {
    extern __shared__ int lds_stack[];
    // per-lane stacks, entry j of lane i at [j * blockDim.x + i]: codes, then bf16 entry parameters
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    // dispatch slots: the heavy_k heaviest tiles (the head of the cost order) as heavy_parts
    // waves each, then the rest of the order one wave per tile
    const int hs = kp.heavy_k * kp.heavy_parts;
    if (tile < kp.tiles + hs - kp.heavy_k) {
        unsigned long long t0 = 0;
        if (TIMED || (REC && kp.cost_time)) t0 = wall_clock64();
        int part = 0;
        const int slot = REC ? __builtin_amdgcn_readfirstlane(tile) : tile;
        if (kp.tile_order) {  // dispatch order -> image tile (a permutation)
            if (tile < hs) {
                part = tile % kp.heavy_parts + 1;
                tile = kp.tile_order[tile / kp.heavy_parts];
            } else {
                tile = kp.tile_order[tile - hs + kp.heavy_k];
            }
        }
        if (REC) {  // wave-uniform: kept in SGPRs through the walks
            tile = __builtin_amdgcn_readfirstlane(tile);
            part = __builtin_amdgcn_readfirstlane(part);
        }
        WalkCount wc{0u, 0u, 0u, 0u};
        // a split tile's parts stamp records tiles + slot (rt_debug_tile_times with room for them)
        unsigned long long* rec =
            TIMED ? kp.tile_times + kTileRec * static_cast<size_t>(part > 0 ? kp.tiles + slot : tile) : nullptr;
        accel_tile<TIMED, COST, TAIL, MT, QUEUE, SS, DISP>(A, mat, kp, tile, part, stk, stt, kp.lane_stack, wc, rec,
                                                           slot < kp.lane_k);
        if (TIMED) {
            const unsigned long long t1 = wall_clock64();
            unsigned long long sn = wc.nodes, st = wc.tests, mn = wc.nodes, mt = wc.tests;
            for (int off = 32; off > 0; off >>= 1) {
                sn += __shfl_xor(sn, off);
                st += __shfl_xor(st, off);
                mn = max(mn, __shfl_xor(mn, off));
                mt = max(mt, __shfl_xor(mt, off));
            }
            const unsigned long long wn = wave_sum(wc.wnodes), wt = wave_sum(wc.wtests);
            if (lane == 0) {
                unsigned long long* o = rec;
                o[22] = wt;
                o[23] = wn;
                o[0] = t0;
                o[1] = t1;
                o[2] = sn;
                o[3] = st;
                o[4] = mn;
                o[5] = mt;
            }
        }
        if (REC && kp.tile_cost) {
            // the tile's cost: its wave's wall time in 40 ns units (cost_time) -- the length
            // of its dependent chain, which a packet walk's union of nodes stretches beyond
            // what its lanes' own steps count -- or those lanes' node steps + tests. Ranking by
            // time: car waited frame 0.2504 -> 0.2247 ms with the latency mode's split below,
            // in flight -1 % (r04v, profiles/r04v_*)
            const unsigned long long work = !COST || kp.cost_time
                                                ? (wall_clock64() - t0) >> 2
                                                : wave_sum(static_cast<unsigned long long>(wc.nodes) + wc.tests);
            unsigned wk = static_cast<unsigned>(work < 0xffffffffull ? work : 0xffffffffull);
            bool rec = part == 0;
            if (part > 0 && lane == 0) {
                // a split tile's cost is the sum of its parts' (one record per tile, by the
                // part that finishes last). Round 3 took the first band's times the bands: a
                // heavy tile whose first band is sky then ranked low, ran whole and late,
                // ranked high again, and so on (the latency-mode car waited frame 0.25 or
                // 0.287 ms by the phase of that cycle, r04l)
                // One 64-bit atomic carries both the count and the sum, so the last part reads
                // the total from its own return value: no agent-scope fences (each writes back
                // or invalidates the XCD's L2, the cost that sank the in-kernel dilation).
                const int hk = slot / kp.heavy_parts;
                const unsigned long long old =
                    atomicAdd(&kp.heavy_acc[hk], (1ull << 56) | static_cast<unsigned long long>(wk));
                if (static_cast<int>(old >> 56) == kp.heavy_parts - 1) {
                    const unsigned long long sum = (old & ((1ull << 56) - 1)) + wk;
                    wk = static_cast<unsigned>(sum < 0xffffffffull ? sum : 0xffffffffull);
                    rec = true;
                }
            }
            if (lane == 0 && rec) {
                kp.tile_cost[tile] = wk;
                atomicAdd(&kp.sched_hist[(tile / kOrderThreads) * kOrderBuckets + work_bucket(wk)], 1u);
            }
        }
    }
}

// Every k_accel instance rtp::accel_instance (dispatch_plan.h) can choose, <TIMED, COST, TAIL, MT, REC, QUEUE, SS>, with
// its twin for the display formats (DISP).
#define RT_ACCEL_INSTANCES(X)                                                                    \
    X(false, false, false, false, false, false, false) X(false, false, false, false, false, false, true) \
    X(false, false, false, false, true, false, false) X(false, false, false, false, true, false, true)   \
    X(false, false, false, true, false, false, false) X(false, false, false, true, false, false, true)   \
    X(false, false, false, true, true, false, false) X(false, false, false, true, true, false, true)     \
    X(false, false, true, false, false, false, false) X(false, false, true, false, false, false, true)   \
    X(false, false, true, false, false, true, false) X(false, false, true, false, true, false, false)    \
    X(false, false, true, false, true, false, true) X(false, false, true, false, true, true, false)      \
    X(false, true, false, false, true, false, false) X(false, true, false, false, true, false, true)     \
    X(false, true, false, true, true, false, false) X(false, true, false, true, true, false, true)       \
    X(false, true, true, false, true, false, false) X(false, true, true, false, true, false, true)       \
    X(false, true, true, false, true, true, false) X(true, true, false, false, true, false, false)
using AccelFn = void (*)(AccelPtrs, const float4*, KParams);
struct AccelEntry {
    rtp::AccelInstance args;
    AccelFn plain, display;
};
#define RT_ACCEL_ENTRY(...) {{__VA_ARGS__}, k_accel<__VA_ARGS__>, k_accel<__VA_ARGS__, true>},
const AccelEntry kAccelTable[] = {RT_ACCEL_INSTANCES(RT_ACCEL_ENTRY)};
#undef RT_ACCEL_ENTRY

// The instance rtp::accel_instance chose, or its twin compiled with the display formats'
// conversion; nullptr for arguments without an entry (RT_ACCEL_INSTANCES is out of date).
AccelFn accel_kernel(const rtp::AccelInstance& a, bool display) {
    for (const AccelEntry& e : kAccelTable) {
        const rtp::AccelInstance& b = e.args;
        if (a.timed == b.timed && a.cost == b.cost && a.tail == b.tail && a.mt == b.mt && a.rec == b.rec &&
            a.queue == b.queue && a.ss == b.ss)
            return display ? e.display : e.plain;
    }
    return nullptr;
}

// The queued rays' remaining bounces (rt_set_tail): one wave per possible chunk
// of 64 rays (kTailRegion / 64 per region), each taking one. The same bounce arithmetic as
// k_accel; a ray's walk does not depend on the other lanes, so compacting rays
// from different tiles into one wave leaves every pixel's value unchanged.
__device__ __forceinline__ int wave_sum_int(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_accel_tail(AccelPtrs A, const float4* __restrict__ mat,
                                                                      KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    // chunks of 64 queued rays, region after region: total chunk count first
    int total = 0;
    for (int b = 0; b < kp.tail_regions; b += 64) {
        const int cnt = b + lane < kp.tail_regions ? kp.tail_count[b + lane] : 0;
        total += wave_sum_int((cnt + 63) >> 6);
    }
    // (r05: the chunks in XCD-contiguous eighths, each XCD's L2 on one band of regions,
    // measured slower on config 5: 2.734 against 2.689 ms in flight, 3.419 against 3.292
    // solo; profiles/r05zs_abf_tail_xcd_negative_*.json)
    const int chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (chunk < total) {
        // the region holding chunk: running prefix of the regions' chunk counts
        int rid = 0, first = 0, n = 0, acc0 = 0;
        for (int b = 0; b < kp.tail_regions; b += 64) {
            const int cnt = b + lane < kp.tail_regions ? kp.tail_count[b + lane] : 0;
            const int ch = (cnt + 63) >> 6;
            int incl = ch;  // inclusive prefix over the 64 lanes
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(incl, off);
                if (lane >= off) incl += y;
            }
            const unsigned long long hit = __ballot(acc0 + incl > chunk && acc0 + incl - ch <= chunk && ch > 0);
            if (hit) {
                const int l = __builtin_ctzll(hit);
                rid = b + l;
                first = __shfl(acc0 + incl - ch, l);
                n = __shfl(cnt, l);
                break;
            }
            acc0 += __shfl(incl, 63);
        }
        const int k = (chunk - first) * 64 + lane;  // index within the region
        bool alive = k < n;
        const int i = rid * kTailRegion + k;
        Ray ray{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
        V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
        int r = 0, x = 0;
        if (alive) {
            const float4* q = kp.tail_queue + 3 * static_cast<size_t>(i);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2];
            const unsigned px = static_cast<unsigned>(kp.tail_px[i]);
            ray = Ray{mk(q0.x, q0.y, q0.z), mk(q1.x, q1.y, q1.z)};
            acc = mk(q0.w, q1.w, q2.w);
            att = mk(q2.x, q2.y, q2.z);
            r = static_cast<int>(px / static_cast<unsigned>(kp.width));
            x = static_cast<int>(px - static_cast<unsigned>(r) * static_cast<unsigned>(kp.width));
        }
        const bool have = alive;
        WalkCount wc{0u, 0u, 0u, 0u};
        for (int depth = kp.tail_from; depth < kp.maxBounces; ++depth) {
            if (__ballot(alive) == 0) break;
            bounce_step<false, false, false, true>(A, mat, kp, depth, ray, alive, acc, att,
                                                   [&]() { return image_row(kp, r); }, stk, stt, kp.lane_stack, wc,
                                                   nullptr, kp.lane_from_depth, kp.shadow_lane_from);
        }
        if (have) store_px(kp, r, x, make_float4(acc.x, acc.y, acc.z, 1.0f));
    }
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < kp.tail_counters; b += blockDim.x) kp.tail_count_next[b] = 0;
}

// ---------------------------------------------------------------------------
// Ray queries (rt_trace_rays / rt_trace_rays_host / rt_trace_pixels): the walks above for
// rays the caller gives, one ray per lane in the order given, answered as rt_hit records.

struct TraceArgs {
    const float4* __restrict__ rays;  // rt_ray: origin | limit, dir | reserved (unused with xy)
    const int2* __restrict__ xy;      // rt_trace_pixels: the pixels whose camera rays are traced, else null
    float4* __restrict__ hits;        // rt_hit, one 16-byte store per ray
    int n;
};

// Ray i and its occlusion limit: two 16-byte loads, or the kernels' own camera ray of
// pixel xy[i] with an infinite limit.
__device__ __forceinline__ Ray trace_ray(const TraceArgs& q, const KParams& kp, int i, float& lim) {
    if (q.xy) {
        const int2 p = q.xy[i];
        lim = INFINITY;
        return primary_ray(kp, p.x, p.y);
    }
    const float4 a = q.rays[2 * static_cast<size_t>(i)], b = q.rays[2 * static_cast<size_t>(i) + 1];
    lim = a.w;
    return Ray{mk(a.x, a.y, a.z), mk(b.x, b.y, b.z)};
}

__device__ __forceinline__ void store_hit(const TraceArgs& q, int i, int shape, float d, bool occluded) {
    q.hits[i] = make_float4(__int_as_float(shape), d, __int_as_float(occluded ? 1 : 0), 0.0f);
}

// MODE: rt_trace_mode. One wave per block over the accelerator, with k_accel_tail's LDS
// stacks and the plain (non-split) lane_walk: closest form, or shadow form with the ray's
// own limit. The winner's distance is the walk's Best::d, its shape AccelPtrs::prim_shape.
template <int MODE, bool MT>
__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_trace(AccelPtrs A, TraceArgs q, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < q.n;
    Ray r{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
    float lim = 0.f;
    if (active) r = trace_ray(q, kp, i, lim);
    WalkCount wc{0u, 0u, 0u, 0u};
    Best b{1e20f, 0x7fffffff, 0.f, -1};
    bool shadow = false;
    if (MODE == RT_TRACE_ANY) {
        lane_walk<true, false, false, MT, true>(A, r, active, gmin(lim, 1e20f), b, shadow, stk, stt, blockDim.x,
                                                kp.lane_stack, wc);
        if (active) store_hit(q, i, -1, 1e20f, shadow);
    } else {
        lane_walk<false, false, false, MT, true>(A, r, active, 0.f, b, shadow, stk, stt, blockDim.x, kp.lane_stack,
                                                 wc);
        if (active) store_hit(q, i, b.slot >= 0 ? A.prim_shape[b.slot] : -1, b.d, b.slot >= 0 && b.d < lim);
    }
}

// The shadow counterpart of lane_closest_bvh: the same walk and intersection, ended by the
// first INNER hit nearer than ld (the reference's closest hit is nearer than ld exactly
// when some hit is).
__device__ bool lane_any_bvh(const KParams& kp, const float4* __restrict__ nodes, const float4* __restrict__ geo,
                             Ray r, float ld, int* stk) {
    if (kp.N <= 0) return false;
    const V inv = inv_dir(r.d);
    int sp = 1;
    stk[0] = kp.N - 1;
    while (sp > 0) {
        --sp;
        const int k = stk[sp * kBlock];
        const float4 a = nodes[2 * k], b = nodes[2 * k + 1];
        if (!ray_aabb(r.o, inv, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z))) continue;
        const int ia = __float_as_int(a.w), ib = __float_as_int(b.w);
        if (ia < 0) {
            const int start = -ia - 1;
            for (int i = 0; i < ib; ++i) {
                const Hit h = intersect(load_rec(geo, start + i), r, kp.useMT);
                if (h.type == INNER && dist(r.o, h.p) < ld) return true;
            }
        } else {
            if (sp + 2 > kp.max_stack) return false;
            stk[sp * kBlock] = ia;
            stk[(sp + 1) * kBlock] = ib;
            sp += 2;
        }
    }
    return false;
}

// The same queries over the reference tree alone, k_lane's literal walk (contexts without a
// usable accelerator, RT_KERNEL_LANE / RT_KERNEL_PACKET): 256-thread blocks, k_lane's stacks.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_trace_ref(TraceArgs q, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= q.n) return;
    float lim;
    const Ray r = trace_ray(q, kp, i, lim);
    if (MODE == RT_TRACE_ANY) {
        store_hit(q, i, -1, 1e20f, lane_any_bvh(kp, kp.nodes, kp.geo_leaf, r, gmin(lim, 1e20f), stk));
    } else {
        Counters c;
        const LaneHit h = lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, r, stk, c);
        const int shape = h.found ? __float_as_int(kp.geo_leaf[5 * static_cast<size_t>(h.slot)].y) : -1;
        store_hit(q, i, shape, h.d, h.found && h.d < lim);
    }
}

// ---------------------------------------------------------------------------
// Shaded rays (rt_shade_rays / rt_shade_rays_host / rt_camera_rays): the frame's bounce loop
// for rays the caller gives, one ray per lane in the order given, one pixel per ray.

struct ShadeArgs {
    const float4* __restrict__ rays;  // rt_view_ray: origin | sky, dir | reserved
    int n;
};

// Pixel i of the compact list as (row, column) of a surface 65,536 pixels wide (shade_launch
// sets kp.pitch to match), so store_px's int column arithmetic holds for any n < 2^31.
constexpr int kShadeRowShift = 16;
__device__ __forceinline__ int shade_row(unsigned i) { return static_cast<int>(i >> kShadeRowShift); }
__device__ __forceinline__ int shade_col(unsigned i) { return static_cast<int>(i & ((1u << kShadeRowShift) - 1u)); }

// One wave per block over the accelerator, with k_trace's LDS stacks: k_accel_tail's loop around
// bounce_step from depth 0, every walk a lane walk (lane_from = shadow_from = 0), so a ray's
// origin and direction are its own (ray_consts decides per ray). The background parameter is
// read again from the ray record on a miss, not kept live through the walks.
template <bool MT, bool SPLIT, bool DISP>
__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_shade(AccelPtrs A, const float4* __restrict__ mat,
                                                                 ShadeArgs q, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    bool alive = i < static_cast<unsigned>(q.n);
    Ray ray{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
    if (alive) {
        const float4 a = q.rays[2 * static_cast<size_t>(i)], b = q.rays[2 * static_cast<size_t>(i) + 1];
        ray = Ray{mk(a.x, a.y, a.z), mk(b.x, b.y, b.z)};
    }
    const bool have = alive;
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    WalkCount wc{0u, 0u, 0u, 0u};
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        if (__ballot(alive) == 0) break;
        bounce_step<false, false, MT, SPLIT>(A, mat, kp, depth, ray, alive, acc, att,
                                             [&]() { return q.rays[2 * static_cast<size_t>(i)].w; }, stk, stt,
                                             kp.lane_stack, wc, nullptr, 0, 0);
    }
    if (have)
        store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, shade_row(i), shade_col(i),
                                                     make_float4(acc.x, acc.y, acc.z, 1.0f));
}

// The same pixels from k_lane's literal per-pixel loop (gpu_shader.comp:450-517), both useBVH
// branches, with the ray and the background from the record (contexts without a usable
// accelerator, RT_KERNEL_LANE / RT_KERNEL_PACKET): 256-thread blocks, k_lane's stacks.
template <bool DISP>
__global__ __launch_bounds__(kBlock) void k_shade_ref(ShadeArgs q, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= static_cast<unsigned>(q.n)) return;
    const float4 ra = q.rays[2 * static_cast<size_t>(i)], rb = q.rays[2 * static_cast<size_t>(i) + 1];
    const V bg = background(kp, ra.w);
    Ray ray{mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z)};
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    Counters c;
    const float shadow_off = kp.useBVH ? 1e-3f : 1e-5f;  // :469 vs :565
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        const LaneHit hit = kp.useBVH ? lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, ray, stk, c)
                                      : lane_closest_brute<false>(kp, kp.geo_lin, ray, c);
        if (!hit.found) {
            acc = acc + mulv(att, bg);
            break;
        }
        const GeoRec g = load_rec(kp.useBVH ? kp.geo_leaf : kp.geo_lin, hit.slot);
        const V hn = shape_normal(g, hit.p);
        const Mat m = load_mat(kp.mat, g.idx);
        const Ray sr{hit.p + hn * shadow_off, normalize(kp.light_pos - hit.p)};
        const float ld = dist(kp.light_pos, hit.p);
        bool shadow;
        if (kp.useBVH) {
            // Full closest-hit walk, as gpu_shader.comp:473-480.
            const LaneHit sh = lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, sr, stk, c);
            shadow = sh.found && sh.d < ld;
        } else {
            shadow = lane_shadow_brute<false>(kp, kp.geo_lin, sr, ld, c);
        }
        if (!shade_bounce(kp, ray, hit.p, hn, m, shadow, acc, att, 1e-3f)) break;
    }
    store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, shade_row(i), shade_col(i), make_float4(acc.x, acc.y, acc.z, 1.0f));
}

// rt_camera_rays: record (y - y0) * width + x holds primary_ray of pixel (x, y) and the
// background parameter a frame uses for row y; one thread per record.
__global__ __launch_bounds__(kBlock) void k_camera_rays(KParams kp, float4* __restrict__ out, unsigned n) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned r = i / static_cast<unsigned>(kp.width);
    const int x = static_cast<int>(i - r * static_cast<unsigned>(kp.width)), y = kp.y0 + static_cast<int>(r);
    const Ray ray = primary_ray(kp, x, y);
    out[2 * static_cast<size_t>(i)] = make_float4(ray.o.x, ray.o.y, ray.o.z, static_cast<float>(y) / kp.resY);
    out[2 * static_cast<size_t>(i) + 1] = make_float4(ray.d.x, ray.d.y, ray.d.z, __int_as_float(0));
}

// ---------------------------------------------------------------------------
// Two or more point lights (rt_set_lights; the definition is include/rt_api.h's). Kernels of
// their own: one-light frames and lists never reach this code, and nothing above is changed.

__device__ __forceinline__ V light_pos(const LightSet& L, int i) { return mk(L.pos[i][0], L.pos[i][1], L.pos[i][2]); }
__device__ __forceinline__ V light_col(const LightSet& L, int i) { return mk(L.col[i][0], L.col[i][1], L.col[i][2]); }

// The light term of a bounce: term_0 + term_1 + ..., left to right, term_i = phong with light
// i, times 0.3 where bit i of `blocked` is set. i is wave-uniform: scalar loads of the records.
__device__ __forceinline__ V lights_term(const LightSet& L, V hp, V hn, V view, const Mat& m, unsigned blocked) {
    V pc = mk(0.f, 0.f, 0.f);
#pragma unroll 1
    for (int i = 0; i < L.count; ++i) {
        V t = phong(hp, hn, view, light_pos(L, i), light_col(L, i), m);
        if ((blocked >> i) & 1u) t = t * 0.3f;
        pc = i == 0 ? t : pc + t;
    }
    return pc;
}

// shade_bounce (gpu_shader.comp:482-516) from a light term already summed.
__device__ __forceinline__ bool shade_bounce_pc(const KParams& kp, Ray& ray, V hp, V hn, const Mat& m, V pc, V& acc,
                                                V& att, float offset_reflect) {
    acc = acc + mulv(att, pc);
    if (m.specular > 0.0f) {
        V rd = reflect(ray.d, hn);
        ray.o = hp + hn * offset_reflect;
        ray.d = rd;
        if (kp.useFresnel) {
            float fr = powf(1.0f - gmax(dot(-ray.d, hn), 0.0f), 5.0f);
            fr = gmin(gmax(fr, 0.0f), 0.8f);
            float rw = m.fresnel * fr;
            float mw = 1.0f - rw;
            att = mulv(att, mix(m.color, mk(1.f, 1.f, 1.f), rw));
            acc = acc + mulv(mw * m.color, pc);
        } else {
            att = att * m.specular;
        }
        return true;
    }
    return false;
}

// bounce_step with the light loop: the closest walk, then L shadow walks from the one shadow
// origin, each lane's answers collected in `blocked`; only after the last walk are the normal
// and the material fetched, once, and the Phong loop run. So what is live through the walks
// is what bounce_step keeps live through its single shadow walk, plus one register. The
// shadow ray is formed again from the hit record before each walk for the same reason.
template <bool MT, class BgY>
__device__ __forceinline__ void bounce_step_lights(const AccelPtrs& A, const float4* __restrict__ mat,
                                                   const KParams& kp, const LightSet& L, int depth, Ray& ray,
                                                   bool& alive, V& acc, V& att, BgY bg_y, int* stk, unsigned short* stt,
                                                   int cap, WalkCount& wc, int lane_from, int shadow_from) {
    Best best{1e20f, 0x7fffffff, 0.f, -1};
    bool unused = false;
    if (depth >= lane_from)  // wave-uniform
        lane_walk_any<false, false, false, MT, false>(A, ray, alive, 0.f, best, unused, stk, stt, blockDim.x, cap, wc);
    else
        packet_walk<false, false, false, MT>(A, ray, alive, 0.f, best, unused, wc);
    if (alive && best.slot < 0) {
        acc = acc + mulv(att, background(kp, bg_y()));
        alive = false;
    }
    unsigned blocked = 0;
#pragma unroll 1
    for (int i = 0; i < L.count; ++i) {
        Ray sr{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
        float ld = 0.f;
        if (alive) {
            const V hp = hit_point(ray, best.t);
            const V hn = shape_normal(load_prim(A.prims, best.slot), hp);
            const V lp = light_pos(L, i);
            sr = Ray{hp + hn * kp.shadow_off, normalize(lp - hp)};
            ld = dist(lp, hp);
        }
        bool shadow = false;
        Best dummy{0.f, 0, 0.f, -1};
        if (depth >= shadow_from)
            lane_walk_any<true, false, false, MT, false>(A, sr, alive, gmin(ld, 1e20f), dummy, shadow, stk, stt,
                                                         blockDim.x, cap, wc);
        else
            packet_walk<true, false, false, MT>(A, sr, alive, gmin(ld, 1e20f), dummy, shadow, wc);
        if (shadow) blocked |= 1u << i;
    }
    if (alive) {
        const PrimRec g = load_prim(A.prims, best.slot);
        const V hp = hit_point(ray, best.t);
        const V hn = shape_normal(g, hp);
        const Mat m = load_mat(mat, A.prim_shape[best.slot]);
        alive = shade_bounce_pc(kp, ray, hp, hn, m, lights_term(L, hp, hn, ray.d, m, blocked), acc, att, 1e-3f);
    }
}

// Over the accelerator, one wave per block with the lane stacks in LDS, as k_shade.
// FRAME = false: k_shade's shape -- ray i of the list per lane, every walk per lane, compact
// pixels. FRAME = true: tile blockIdx.x of the frame in row-major tile order (tile_pixel,
// primary_ray), camera rays and their L shadow rays as wave64 packets -- the L shadow packets
// of a tile converge on one point each -- and later bounces per lane; the sky from the image
// row, the pixel through store_px in the dispatch's row mapping and format. No cost order, no
// split tiles, no compaction: launch_lights.
template <bool MT, bool DISP, bool FRAME>
__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_lights(AccelPtrs A, const float4* __restrict__ mat,
                                                                  ShadeArgs q, LightSet L, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;  // the list's ray
    const int tile = static_cast<int>(blockIdx.x);             // the frame's tile
    bool alive;
    Ray ray{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
    if constexpr (FRAME) {
        const PixelCoord pc = tile_pixel(kp, tile);
        ray = primary_ray(kp, pc.x, pc.y);
        alive = pc.active;
    } else {
        alive = i < static_cast<unsigned>(q.n);
        if (alive) {
            const float4 a = q.rays[2 * static_cast<size_t>(i)], b = q.rays[2 * static_cast<size_t>(i) + 1];
            ray = Ray{mk(a.x, a.y, a.z), mk(b.x, b.y, b.z)};
        }
    }
    const bool have = alive;
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    if (FRAME && kp.root_ok) {
        // accel_tile's root test: a camera ray that misses the root's box takes the background
        V rlo = mk(kp.root_lo[0], kp.root_lo[1], kp.root_lo[2]), rhi = mk(kp.root_hi[0], kp.root_hi[1], kp.root_hi[2]);
        if (kp.root_ok == 2) {
            const float4 a = A.anodes[4 * static_cast<size_t>(A.N - 1)], b = A.anodes[4 * static_cast<size_t>(A.N - 1) + 1];
            rlo = mk(a.x, a.y, a.z);
            rhi = mk(b.x, b.y, b.z);
        }
        if (alive && !ray_aabb(ray.o, inv_dir(ray.d), rlo, rhi)) {
            acc = background(kp, tile_pixel(kp, tile).y);
            alive = false;
        }
    }
    WalkCount wc{0u, 0u, 0u, 0u};
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        if (__ballot(alive) == 0) break;
        if constexpr (FRAME)
            bounce_step_lights<MT>(A, mat, kp, L, depth, ray, alive, acc, att,
                                   [&]() { return tile_pixel(kp, tile).y; }, stk, stt, kp.lane_stack, wc, 1, 1);
        else
            bounce_step_lights<MT>(A, mat, kp, L, depth, ray, alive, acc, att,
                                   [&]() { return q.rays[2 * static_cast<size_t>(i)].w; }, stk, stt, kp.lane_stack,
                                   wc, 0, 0);
    }
    if (!have) return;
    const float4 px = make_float4(acc.x, acc.y, acc.z, 1.0f);
    if constexpr (FRAME) {
        const PixelCoord pc = tile_pixel(kp, tile);
        store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, pc.r, pc.x, px);
    } else {
        store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, shade_row(i), shade_col(i), px);
    }
}

// The literal per-lane loop of k_lane (FRAME: its pixels and blocks) / k_shade_ref (the list)
// with the light loop, both useBVH branches: RT_KERNEL_LANE / RT_KERNEL_PACKET, contexts
// without a usable accelerator, far cameras. The BVH branch's shadow is the full closest-hit
// walk with found && d < ld, per light (gpu_shader.comp:473-480).
template <bool DISP, bool FRAME>
__global__ __launch_bounds__(kBlock) void k_lights_ref(ShadeArgs q, LightSet L, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    int r, x;  // the output pixel
    V bg;
    Ray ray;
    if constexpr (FRAME) {
        const PixelCoord pc = pixel_of(kp);
        if (!pc.active) return;
        r = pc.r;
        x = pc.x;
        bg = background(kp, pc.y);
        ray = primary_ray(kp, pc.x, pc.y);
    } else {
        if (i >= static_cast<unsigned>(q.n)) return;
        const float4 ra = q.rays[2 * static_cast<size_t>(i)], rb = q.rays[2 * static_cast<size_t>(i) + 1];
        r = shade_row(i);
        x = shade_col(i);
        bg = background(kp, ra.w);
        ray = Ray{mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z)};
    }
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    Counters c;
    const float shadow_off = kp.useBVH ? 1e-3f : 1e-5f;  // :469 vs :565
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        const LaneHit hit = kp.useBVH ? lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, ray, stk, c)
                                      : lane_closest_brute<false>(kp, kp.geo_lin, ray, c);
        if (!hit.found) {
            acc = acc + mulv(att, bg);
            break;
        }
        const GeoRec g = load_rec(kp.useBVH ? kp.geo_leaf : kp.geo_lin, hit.slot);
        const V hn = shape_normal(g, hit.p);
        const Mat m = load_mat(kp.mat, g.idx);
        const V so = hit.p + hn * shadow_off;
        unsigned blocked = 0;
#pragma unroll 1
        for (int k = 0; k < L.count; ++k) {
            const V lp = light_pos(L, k);
            const Ray sr{so, normalize(lp - hit.p)};
            const float ld = dist(lp, hit.p);
            bool shadow;
            if (kp.useBVH) {
                const LaneHit sh = lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, sr, stk, c);
                shadow = sh.found && sh.d < ld;
            } else {
                shadow = lane_shadow_brute<false>(kp, kp.geo_lin, sr, ld, c);
            }
            if (shadow) blocked |= 1u << k;
        }
        if (!shade_bounce_pc(kp, ray, hit.p, hn, m, lights_term(L, hit.p, hn, ray.d, m, blocked), acc, att, 1e-3f))
            break;
    }
    store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, r, x, make_float4(acc.x, acc.y, acc.z, 1.0f));
}

// ---------------------------------------------------------------------------
// Geometry buffers (rt_dispatch_gbuffer / rt_gbuffer_host): the closest hit of every pixel's
// camera ray as up to four planes (include/rt_api.h: shape, depth, normal, position).

// One pixel of every plane the caller gave (a wave-uniform choice), compact row r, column x.
// Streaming stores, one per plane: the kernels never read the planes back.
typedef float rt_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_gbuffer(const rt_gbuffer& g, int r, int x, int shape, float depth, V n, V p,
                                              float w) {
    const size_t row = static_cast<size_t>(r);
    if (g.shape)
        __builtin_nontemporal_store(shape,
                                    reinterpret_cast<int*>(reinterpret_cast<char*>(g.shape) + row * g.shape_pitch) + x);
    if (g.depth)
        __builtin_nontemporal_store(
            depth, reinterpret_cast<float*>(reinterpret_cast<char*>(g.depth) + row * g.depth_pitch) + x);
    if (g.normal)
        __builtin_nontemporal_store(
            rt_f32x4{n.x, n.y, n.z, 0.0f},
            reinterpret_cast<rt_f32x4*>(reinterpret_cast<char*>(g.normal) + row * g.normal_pitch) + x);
    if (g.position)
        __builtin_nontemporal_store(
            rt_f32x4{p.x, p.y, p.z, w},
            reinterpret_cast<rt_f32x4*>(reinterpret_cast<char*>(g.position) + row * g.position_pitch) + x);
}

// One 8x8 tile per wave in row-major tile order (tile_pixel), any number of waves to a block,
// over the accelerator: the tile's camera rays as one packet (packet_walk: the stack in VGPRs,
// no LDS), or, LANE, one ray per lane with k_trace's LDS stacks -- the frames whose camera lies
// beyond the accelerator's origin bound, and the A/B of tools/bench_gbuffer.py. Rays that miss
// the root's box (accel_tile's test, from the kernel arguments) skip the walk: the sky tiles.
// No shading state is carried, so k_accel's register cap does not apply.
template <bool MT, bool LANE>
__global__ __launch_bounds__(kBlock) void k_gbuffer(AccelPtrs A, rt_gbuffer g, KParams kp) {
    extern __shared__ int lds_stack[];
    const int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tile >= kp.tiles) return;  // wave-uniform
    const PixelCoord pc = tile_pixel(kp, tile);
    const Ray ray = primary_ray(kp, pc.x, pc.y);
    bool alive = pc.active;
    if (kp.root_ok) {
        V rlo = mk(kp.root_lo[0], kp.root_lo[1], kp.root_lo[2]), rhi = mk(kp.root_hi[0], kp.root_hi[1], kp.root_hi[2]);
        if (kp.root_ok == 2) {
            const float4 a = A.anodes[4 * static_cast<size_t>(A.N - 1)], b = A.anodes[4 * static_cast<size_t>(A.N - 1) + 1];
            rlo = mk(a.x, a.y, a.z);
            rhi = mk(b.x, b.y, b.z);
        }
        alive = alive && ray_aabb(ray.o, inv_dir(ray.d), rlo, rhi);
    }
    Best best{1e20f, 0x7fffffff, 0.f, -1};
    bool unused = false;
    WalkCount wc{0u, 0u, 0u, 0u};
    if (LANE) {
        int* stk = lds_stack + threadIdx.x;
        unsigned short* stt =
            reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) +
            threadIdx.x;
        lane_walk<false, false, false, MT, true>(A, ray, alive, 0.f, best, unused, stk, stt, blockDim.x,
                                                 kp.lane_stack, wc);
    } else {
        packet_walk<false, false, false, MT>(A, ray, alive, 0.f, best, unused, wc);
    }
    if (!pc.active) return;
    if (best.slot < 0) {
        store_gbuffer(g, pc.r, pc.x, -1, 1e20f, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), 0.0f);
        return;
    }
    const V p = hit_point(ray, best.t);
    store_gbuffer(g, pc.r, pc.x, A.prim_shape[best.slot], best.d, shape_normal(load_prim(A.prims, best.slot), p), p,
                  1.0f);
}

// The same planes from k_lane's literal walk over the reference tree alone (contexts without
// a usable accelerator, RT_KERNEL_LANE / RT_KERNEL_PACKET): k_lane's blocks, pixels and stacks.
__global__ __launch_bounds__(kBlock) void k_gbuffer_ref(rt_gbuffer g, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    const PixelCoord pc = pixel_of(kp);
    if (!pc.active) return;
    const Ray r = primary_ray(kp, pc.x, pc.y);
    Counters c;
    const LaneHit h = lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, r, stk, c);
    if (!h.found) {
        store_gbuffer(g, pc.r, pc.x, -1, 1e20f, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), 0.0f);
        return;
    }
    const GeoRec rec = load_rec(kp.geo_leaf, h.slot);
    store_gbuffer(g, pc.r, pc.x, rec.idx, h.d, shape_normal(rec, h.p), h.p, 1.0f);
}

// ---------------------------------------------------------------------------
// Ambient occlusion (rt_dispatch_ao / rt_ao_host): per pixel the number of the K fixed
// hemisphere rays about the visible surface's facing normal that are occluded within a radius
// (include/rt_api.h, "Definition of a pixel": every operation below is in that order).

__device__ const float kAoDir[64 * 3] = {RT_AO_DIRS};
__device__ const float kAoRot[16 * 2] = {RT_AO_ROT};

struct AoArgs {
    rt_ao out;
    int rays;
    float radius, bias;
};

// Steps 1, 2 and 5's origin: the facing normal, the tangent frame about it, the rays' origin.
struct AoFrame {
    V o, t, u, nf;
};

__device__ __forceinline__ AoFrame ao_frame(V p, V n, V d, float bias) {
    const float s = (n.x * d.x + n.y * d.y) + n.z * d.z;
    const V nf = s > 0.0f ? -n : n;
    const float sg = copysignf(1.0f, nf.z);
    const float a = -1.0f / (sg + nf.z);
    const float b = (nf.x * nf.y) * a;
    AoFrame f;
    f.t = mk(1.0f + sg * ((nf.x * nf.x) * a), sg * b, -(sg * nf.x));
    f.u = mk(b, sg + (nf.y * nf.y) * a, -nf.y);
    f.nf = nf;
    f.o = p + nf * bias;
    return f;
}

// Steps 4 and 5: ray k of a pixel whose rotation is (c, sn).
__device__ __forceinline__ Ray ao_ray(const AoFrame& f, float c, float sn, int k) {
    const float dx = kAoDir[3 * k], dy = kAoDir[3 * k + 1], lz = kAoDir[3 * k + 2];
    const float lx = c * dx - sn * dy, ly = sn * dx + c * dy;
    return Ray{f.o, mk((f.t.x * lx + f.u.x * ly) + f.nf.x * lz, (f.t.y * lx + f.u.y * ly) + f.nf.y * lz,
                       (f.t.z * lx + f.u.z * ly) + f.nf.z * lz)};
}

// One pixel of the planes the caller gave: a byte store, and a streaming dword store.
__device__ __forceinline__ void store_ao(const AoArgs& q, int r, int x, int count) {
    const size_t row = static_cast<size_t>(r);
    if (q.out.count) (q.out.count + row * q.out.count_pitch)[x] = static_cast<uint8_t>(count);
    if (q.out.visibility)
        __builtin_nontemporal_store(
            static_cast<float>(q.rays - count) / static_cast<float>(q.rays),
            reinterpret_cast<float*>(reinterpret_cast<char*>(q.out.visibility) + row * q.out.visibility_pitch) + x);
}

constexpr int kAoSlot = 15;  // dwords a hit lane leaves in LDS (PACK): o, t, u, nf, (c, sn), its counter

// One 8x8 tile per wave, any number of waves to a block. The camera rays go exactly as in
// k_gbuffer (the root-box skip, then packet_walk, or LANE: lane_walk). The occlusion rays go
// through the shadow form of lane_walk with k_trace's LDS stacks.
//   PACK = false (the default, kAoPack): each hit lane walks its own K rays, one after the
//     other. A tile on a silhouette keeps its miss lanes idle for K walks.
//   PACK = true: the h hit lanes (a ballot) leave their frame in LDS, slot = rank among the hit
//     lanes; the wave walks the h * K work items 64 at a time (item i: ray i / h of slot i % h,
//     so the lanes of a round walk the same or neighbouring k of neighbouring pixels) and adds
//     each occluded ray to its owner's LDS counter. ceil(h * K / 64) rounds, none for a tile
//     without a hit.
// Dynamic LDS: lane_stack x 6 B per lane, then, PACK, kAoSlot x 256 B per wave. Waves do not
// share LDS, so nothing here waits on a block barrier.
template <bool MT, bool LANE, bool PACK>
__global__ __launch_bounds__(kBlock) void k_ao(AccelPtrs A, AoArgs q, KParams kp) {
    extern __shared__ int lds_stack[];
    const int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tile >= kp.tiles) return;  // wave-uniform
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const PixelCoord pc = tile_pixel(kp, tile);
    const Ray ray = primary_ray(kp, pc.x, pc.y);
    bool alive = pc.active;
    if (kp.root_ok) {
        V rlo = mk(kp.root_lo[0], kp.root_lo[1], kp.root_lo[2]), rhi = mk(kp.root_hi[0], kp.root_hi[1], kp.root_hi[2]);
        if (kp.root_ok == 2) {
            const float4 a = A.anodes[4 * static_cast<size_t>(A.N - 1)], b = A.anodes[4 * static_cast<size_t>(A.N - 1) + 1];
            rlo = mk(a.x, a.y, a.z);
            rhi = mk(b.x, b.y, b.z);
        }
        alive = alive && ray_aabb(ray.o, inv_dir(ray.d), rlo, rhi);
    }
    Best best{1e20f, 0x7fffffff, 0.f, -1};
    bool unused = false;
    WalkCount wc{0u, 0u, 0u, 0u};
    if (LANE) {
        lane_walk<false, false, false, MT, true>(A, ray, alive, 0.f, best, unused, stk, stt, blockDim.x,
                                                 kp.lane_stack, wc);
    } else {
        packet_walk<false, false, false, MT>(A, ray, alive, 0.f, best, unused, wc);
    }
    const bool hit = pc.active && best.slot >= 0;
    const unsigned long long hm = __ballot(hit);
    if (hm == 0) {  // wave-uniform: a tile of misses costs the camera walk only
        if (pc.active) store_ao(q, pc.r, pc.x, 0);
        return;
    }
    AoFrame f{};
    float c = 1.0f, sn = 0.0f;
    if (hit) {
        const V p = hit_point(ray, best.t);
        f = ao_frame(p, shape_normal(load_prim(A.prims, best.slot), p), ray.d, q.bias);
        const int j = (pc.x & 3) + 4 * (pc.y & 3);
        c = kAoRot[2 * j];
        sn = kAoRot[2 * j + 1];
    }
    const float lim = gmin(q.radius, 1e20f);
    int count = 0;
    if (!PACK) {
        for (int k = 0; k < q.rays; ++k) {  // wave-uniform trip count
            bool occluded = false;
            Best b{1e20f, 0x7fffffff, 0.f, -1};
            lane_walk<true, false, false, MT, true>(A, ao_ray(f, c, sn, k), hit, lim, b, occluded, stk, stt,
                                                    blockDim.x, kp.lane_stack, wc);
            count += occluded ? 1 : 0;
        }
    } else {
        const int lane = threadIdx.x & 63;
        float* fr = reinterpret_cast<float*>(lds_stack) + (static_cast<size_t>(kp.lane_stack) * blockDim.x * 6) / 4 +
                    static_cast<size_t>(threadIdx.x >> 6) * (kAoSlot * 64);
        int* cnt = reinterpret_cast<int*>(fr) + 14 * 64;
        const int h = __popcll(hm);
        const int slot = __popcll(hm & ((1ull << lane) - 1ull));
        if (hit) {
            const float v[14] = {f.o.x, f.o.y, f.o.z, f.t.x, f.t.y, f.t.z, f.u.x, f.u.y, f.u.z, f.nf.x, f.nf.y, f.nf.z, c, sn};
#pragma unroll
            for (int e = 0; e < 14; ++e) fr[e * 64 + slot] = v[e];
            cnt[slot] = 0;
        }
        // the wave's own LDS writes, read by its other lanes: program order, no block barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const unsigned items = static_cast<unsigned>(h) * static_cast<unsigned>(q.rays);  // at most 4096
        for (unsigned base = 0; base < items; base += 64) {  // wave-uniform
            const unsigned i = base + static_cast<unsigned>(lane);
            const bool on = i < items;
            const unsigned k = on ? i / static_cast<unsigned>(h) : 0u;
            const int j = on ? static_cast<int>(i - k * static_cast<unsigned>(h)) : 0;
            AoFrame g;
            g.o = mk(fr[0 * 64 + j], fr[1 * 64 + j], fr[2 * 64 + j]);
            g.t = mk(fr[3 * 64 + j], fr[4 * 64 + j], fr[5 * 64 + j]);
            g.u = mk(fr[6 * 64 + j], fr[7 * 64 + j], fr[8 * 64 + j]);
            g.nf = mk(fr[9 * 64 + j], fr[10 * 64 + j], fr[11 * 64 + j]);
            bool occluded = false;
            Best b{1e20f, 0x7fffffff, 0.f, -1};
            lane_walk<true, false, false, MT, true>(A, ao_ray(g, fr[12 * 64 + j], fr[13 * 64 + j], static_cast<int>(k)),
                                                    on, lim, b, occluded, stk, stt, blockDim.x, kp.lane_stack, wc);
            if (on && occluded) atomicAdd(&cnt[j], 1);  // LDS atomic
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (hit) count = cnt[slot];
    }
    if (pc.active) store_ao(q, pc.r, pc.x, count);
}

// The same planes from k_lane's literal walks over the reference tree alone (contexts without
// a usable accelerator, RT_KERNEL_LANE / RT_KERNEL_PACKET): k_lane's blocks, pixels and stacks;
// lane_closest_bvh for the camera ray, then lane_any_bvh for each of the K rays.
__global__ __launch_bounds__(kBlock) void k_ao_ref(AoArgs q, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    const PixelCoord pc = pixel_of(kp);
    if (!pc.active) return;
    const Ray r = primary_ray(kp, pc.x, pc.y);
    Counters cn;
    const LaneHit h = lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, r, stk, cn);
    int count = 0;
    if (h.found) {
        const AoFrame f = ao_frame(h.p, shape_normal(load_rec(kp.geo_leaf, h.slot), h.p), r.d, q.bias);
        const int j = (pc.x & 3) + 4 * (pc.y & 3);
        const float c = kAoRot[2 * j], sn = kAoRot[2 * j + 1], lim = gmin(q.radius, 1e20f);
        for (int k = 0; k < q.rays; ++k)
            count += lane_any_bvh(kp, kp.nodes, kp.geo_leaf, ao_ray(f, c, sn, k), lim, stk) ? 1 : 0;
    }
    store_ao(q, pc.r, pc.x, count);
}

// ---------------------------------------------------------------------------
// Area lights (rt_set_soft_shadows; the definition is include/rt_api.h's, every operation below
// in that order). Kernels of their own, in the shape of k_lights / k_lights_ref: frames and
// lists without a radius > 0 never reach this code, and nothing above is changed.

// Steps 1-5: sample point k of a light at lp with radius R > 0, seen from the hit point hp. The
// frame is ao_frame's about w without the facing flip; the rotation is per lane (a hash of hp,
// a gather from kAoRot), k is wave-uniform (scalar loads from kAoDir).
__device__ __forceinline__ V soft_point(V hp, V lp, float R, int k) {
    const V w = normalize(lp - hp);
    const float sg = copysignf(1.0f, w.z);
    const float a = -1.0f / (sg + w.z);
    const float b = (w.x * w.y) * a;
    const V t = mk(1.0f + sg * ((w.x * w.x) * a), sg * b, -(sg * w.x));
    const V u = mk(b, sg + (w.y * w.y) * a, -w.y);
    const unsigned j =
        ((__float_as_uint(hp.x) ^ __float_as_uint(hp.y) ^ __float_as_uint(hp.z)) * 0x9E3779B1u) >> 28;
    const float c = kAoRot[2 * j], sn = kAoRot[2 * j + 1];
    const float dx = kAoDir[3 * k], dy = kAoDir[3 * k + 1];
    const float lx = c * dx - sn * dy, ly = sn * dx + c * dy;
    const float rx = R * lx, ry = R * ly;
    return mk(lp.x + ((t.x * rx) + (u.x * ry)), lp.y + ((t.y * rx) + (u.y * ry)), lp.z + ((t.z * rx) + (u.z * ry)));
}

// Shadow ray k of light i from the hit (hp, hn): towards the sample point, or the light itself
// for radius 0 -- then exactly k_lights' ray. `ld`: its limit before min(.., 1e20f).
__device__ __forceinline__ Ray soft_ray(const LightSet& L, const SoftSet& S, int i, int k, V hp, V hn, float off,
                                        float& ld) {
    const V lp = light_pos(L, i);
    const float R = S.radius[i];
    const V s = R > 0.0f ? soft_point(hp, lp, R, k) : lp;
    ld = dist(s, hp);
    return Ray{hp + hn * off, normalize(s - hp)};
}

// The rays of light i: K for an area light, one for a point.
__device__ __forceinline__ int soft_rays(const SoftSet& S, int i) { return S.radius[i] > 0.0f ? S.samples : 1; }

// The light term of a bounce: term_0 + term_1 + ..., left to right; term_i = phong with light
// i's centre, times 1 - 0.7 b_i / K_i where b_i > 0. `blocked`: eight 7-bit counts b_i.
__device__ __forceinline__ V soft_term(const LightSet& L, const SoftSet& S, V hp, V hn, V view, const Mat& m,
                                       unsigned long long blocked) {
    V pc = mk(0.f, 0.f, 0.f);
#pragma unroll 1
    for (int i = 0; i < L.count; ++i) {
        V t = phong(hp, hn, view, light_pos(L, i), light_col(L, i), m);
        const unsigned b = static_cast<unsigned>(blocked >> (7 * i)) & 127u;
        if (b > 0) t = t * (1.0f - 0.7f * (static_cast<float>(b) / static_cast<float>(soft_rays(S, i))));
        pc = i == 0 ? t : pc + t;
    }
    return pc;
}

// bounce_step_lights with the sample loop: the closest walk, then K_i shadow walks per light
// from the one shadow origin, each lane's blocked rays counted in `blocked` (two registers);
// the normal and the material are fetched once, after the last walk, and each sample ray is
// formed again from the hit record before its walk, so the walks keep live what
// bounce_step_lights keeps. Both loops are wave-uniform. A wave whose lanes all left (sky)
// walks no shadow ray.
//   PACK (bounces >= 1, where a mirror leaves few lanes alive and each would walk its L K rays
//   while the rest idle; k_ao's PACK form): the h live lanes leave hit point and normal in LDS
//   (`pk`, slot = rank among the live lanes); per light the wave walks the h * K_i items 64 at
//   a time (item: ray item / h of slot item % h), each sample ray formed from the slot by the
//   same soft_ray, and adds each blocked ray to its owner's LDS counter, between wave-level
//   fences. Same counts, so the same bytes.
constexpr int kSoftSlot = 7;  // dwords a live lane leaves in LDS (PACK): hp, hn, its counter
template <bool MT, bool PACK, class BgY>
__device__ __forceinline__ void bounce_step_soft(const AccelPtrs& A, const float4* __restrict__ mat, const KParams& kp,
                                                 const LightSet& L, const SoftSet& S, int depth, Ray& ray, bool& alive,
                                                 V& acc, V& att, BgY bg_y, int* stk, unsigned short* stt, int cap,
                                                 WalkCount& wc, int lane_from, int shadow_from, float* pk) {
    Best best{1e20f, 0x7fffffff, 0.f, -1};
    bool unused = false;
    if (depth >= lane_from)  // wave-uniform
        lane_walk_any<false, false, false, MT, false>(A, ray, alive, 0.f, best, unused, stk, stt, blockDim.x, cap, wc);
    else
        packet_walk<false, false, false, MT>(A, ray, alive, 0.f, best, unused, wc);
    if (alive && best.slot < 0) {
        acc = acc + mulv(att, background(kp, bg_y()));
        alive = false;
    }
    const unsigned long long hm = __ballot(alive);
    if (hm == 0) return;
    unsigned long long blocked = 0;
    if (PACK && depth >= 1) {  // wave-uniform: the live lanes' sample rays over all 64 lanes
        const int lane = threadIdx.x & 63;
        int* cnt = reinterpret_cast<int*>(pk) + 6 * 64;
        const int h = __popcll(hm);
        const int slot = __popcll(hm & ((1ull << lane) - 1ull));
        if (alive) {
            const V hp = hit_point(ray, best.t);
            const V hn = shape_normal(load_prim(A.prims, best.slot), hp);
            const float v[6] = {hp.x, hp.y, hp.z, hn.x, hn.y, hn.z};
#pragma unroll
            for (int e = 0; e < 6; ++e) pk[e * 64 + slot] = v[e];
            cnt[slot] = 0;
        }
#pragma unroll 1
        for (int i = 0; i < L.count; ++i) {
            // the wave's own LDS writes, read by its other lanes: program order, no block barrier
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const unsigned items = static_cast<unsigned>(h) * static_cast<unsigned>(soft_rays(S, i));  // at most 4096
#pragma unroll 1
            for (unsigned base = 0; base < items; base += 64) {
                const unsigned it = base + static_cast<unsigned>(lane);
                const bool on = it < items;
                const unsigned k = on ? it / static_cast<unsigned>(h) : 0u;
                const int j = on ? static_cast<int>(it - k * static_cast<unsigned>(h)) : 0;
                const V hp = mk(pk[0 * 64 + j], pk[1 * 64 + j], pk[2 * 64 + j]);
                const V hn = mk(pk[3 * 64 + j], pk[4 * 64 + j], pk[5 * 64 + j]);
                float ld;
                Ray sr = soft_ray(L, S, i, static_cast<int>(k), hp, hn, kp.shadow_off, ld);
                bool shadow = false;
                Best dummy{0.f, 0, 0.f, -1};
                lane_walk_any<true, false, false, MT, false>(A, sr, on, gmin(ld, 1e20f), dummy, shadow, stk, stt,
                                                             blockDim.x, cap, wc);
                if (on && shadow) atomicAdd(&cnt[j], 1);  // LDS atomic
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (alive) {
                blocked += static_cast<unsigned long long>(cnt[slot]) << (7 * i);
                cnt[slot] = 0;
            }
        }
    }
    const bool packed = PACK && depth >= 1;  // else the plain form: each live lane walks its own rays
#pragma unroll 1
    for (int i = 0; !packed && i < L.count; ++i) {
        const int rays = soft_rays(S, i);
#pragma unroll 1
        for (int k = 0; k < rays; ++k) {
            Ray sr{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
            float ld = 0.f;
            if (alive) {
                const V hp = hit_point(ray, best.t);
                sr = soft_ray(L, S, i, k, hp, shape_normal(load_prim(A.prims, best.slot), hp), kp.shadow_off, ld);
            }
            bool shadow = false;
            Best dummy{0.f, 0, 0.f, -1};
            if (depth >= shadow_from)
                lane_walk_any<true, false, false, MT, false>(A, sr, alive, gmin(ld, 1e20f), dummy, shadow, stk, stt,
                                                             blockDim.x, cap, wc);
            else
                packet_walk<true, false, false, MT>(A, sr, alive, gmin(ld, 1e20f), dummy, shadow, wc);
            if (shadow) blocked += 1ull << (7 * i);
        }
    }
    if (alive) {
        const PrimRec g = load_prim(A.prims, best.slot);
        const V hp = hit_point(ray, best.t);
        const V hn = shape_normal(g, hp);
        const Mat m = load_mat(mat, A.prim_shape[best.slot]);
        alive = shade_bounce_pc(kp, ray, hp, hn, m, soft_term(L, S, hp, hn, ray.d, m, blocked), acc, att, 1e-3f);
    }
}

// k_lights with the SoftSet: one wave per block, the lane stacks in LDS. FRAME = false: the
// list, every walk per lane. FRAME = true: tile blockIdx.x in row-major tile order, camera rays
// and all their sample rays as wave64 packets -- the K packets of a light converge on one small
// disc -- later bounces per lane. No cost order, no split tiles, no compaction: launch_soft.
template <bool MT, bool DISP, bool FRAME, bool PACK>
__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_soft(AccelPtrs A, const float4* __restrict__ mat, ShadeArgs q,
                                                                LightSet L, SoftSet S, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;  // the list's ray
    const int tile = static_cast<int>(blockIdx.x);             // the frame's tile
    bool alive;
    Ray ray{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
    if constexpr (FRAME) {
        const PixelCoord pc = tile_pixel(kp, tile);
        ray = primary_ray(kp, pc.x, pc.y);
        alive = pc.active;
    } else {
        alive = i < static_cast<unsigned>(q.n);
        if (alive) {
            const float4 a = q.rays[2 * static_cast<size_t>(i)], b = q.rays[2 * static_cast<size_t>(i) + 1];
            ray = Ray{mk(a.x, a.y, a.z), mk(b.x, b.y, b.z)};
        }
    }
    const bool have = alive;
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    if (FRAME && kp.root_ok) {
        // accel_tile's root test: a camera ray that misses the root's box takes the background
        V rlo = mk(kp.root_lo[0], kp.root_lo[1], kp.root_lo[2]), rhi = mk(kp.root_hi[0], kp.root_hi[1], kp.root_hi[2]);
        if (kp.root_ok == 2) {
            const float4 a = A.anodes[4 * static_cast<size_t>(A.N - 1)], b = A.anodes[4 * static_cast<size_t>(A.N - 1) + 1];
            rlo = mk(a.x, a.y, a.z);
            rhi = mk(b.x, b.y, b.z);
        }
        if (alive && !ray_aabb(ray.o, inv_dir(ray.d), rlo, rhi)) {
            acc = background(kp, tile_pixel(kp, tile).y);
            alive = false;
        }
    }
    WalkCount wc{0u, 0u, 0u, 0u};
    // PACK: kSoftSlot dwords per lane after the lane stacks (launch_soft's LDS size)
    float* pk = reinterpret_cast<float*>(lds_stack) + (static_cast<size_t>(kp.lane_stack) * blockDim.x * 6) / 4;
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        if (__ballot(alive) == 0) break;
        if constexpr (FRAME)
            bounce_step_soft<MT, PACK>(A, mat, kp, L, S, depth, ray, alive, acc, att,
                                       [&]() { return tile_pixel(kp, tile).y; }, stk, stt, kp.lane_stack, wc, 1, 1, pk);
        else
            bounce_step_soft<MT, PACK>(A, mat, kp, L, S, depth, ray, alive, acc, att,
                                       [&]() { return q.rays[2 * static_cast<size_t>(i)].w; }, stk, stt,
                                       kp.lane_stack, wc, 0, 0, pk);
    }
    if (!have) return;
    const float4 px = make_float4(acc.x, acc.y, acc.z, 1.0f);
    if constexpr (FRAME) {
        const PixelCoord pc = tile_pixel(kp, tile);
        store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, pc.r, pc.x, px);
    } else {
        store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, shade_row(i), shade_col(i), px);
    }
}

// k_lights_ref with the sample loop: the literal per-lane loop on both useBVH branches
// (RT_KERNEL_LANE / RT_KERNEL_PACKET, contexts without a usable accelerator, far cameras).
template <bool DISP, bool FRAME>
__global__ __launch_bounds__(kBlock) void k_soft_ref(ShadeArgs q, LightSet L, SoftSet S, KParams kp) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    int r, x;  // the output pixel
    V bg;
    Ray ray;
    if constexpr (FRAME) {
        const PixelCoord pc = pixel_of(kp);
        if (!pc.active) return;
        r = pc.r;
        x = pc.x;
        bg = background(kp, pc.y);
        ray = primary_ray(kp, pc.x, pc.y);
    } else {
        if (i >= static_cast<unsigned>(q.n)) return;
        const float4 ra = q.rays[2 * static_cast<size_t>(i)], rb = q.rays[2 * static_cast<size_t>(i) + 1];
        r = shade_row(i);
        x = shade_col(i);
        bg = background(kp, ra.w);
        ray = Ray{mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z)};
    }
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    Counters c;
    const float shadow_off = kp.useBVH ? 1e-3f : 1e-5f;  // :469 vs :565
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        const LaneHit hit = kp.useBVH ? lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, ray, stk, c)
                                      : lane_closest_brute<false>(kp, kp.geo_lin, ray, c);
        if (!hit.found) {
            acc = acc + mulv(att, bg);
            break;
        }
        const GeoRec g = load_rec(kp.useBVH ? kp.geo_leaf : kp.geo_lin, hit.slot);
        const V hn = shape_normal(g, hit.p);
        const Mat m = load_mat(kp.mat, g.idx);
        unsigned long long blocked = 0;
#pragma unroll 1
        for (int l = 0; l < L.count; ++l) {
            const int rays = soft_rays(S, l);
#pragma unroll 1
            for (int k = 0; k < rays; ++k) {
                float ld;
                const Ray sr = soft_ray(L, S, l, k, hit.p, hn, shadow_off, ld);
                bool shadow;
                if (kp.useBVH) {
                    const LaneHit sh = lane_closest_bvh<false>(kp, kp.nodes, kp.geo_leaf, sr, stk, c);
                    shadow = sh.found && sh.d < ld;
                } else {
                    shadow = lane_shadow_brute<false>(kp, kp.geo_lin, sr, ld, c);
                }
                if (shadow) blocked += 1ull << (7 * l);
            }
        }
        if (!shade_bounce_pc(kp, ray, hit.p, hn, m, soft_term(L, S, hit.p, hn, ray.d, m, blocked), acc, att, 1e-3f))
            break;
    }
    store_px<DISP ? kStoreDisplay : kStoreFloat>(kp, r, x, make_float4(acc.x, acc.y, acc.z, 1.0f));
}

// The general path of rt_set_samples: the sample frame was rendered by any kernel into a
// scratch surface (compact rows, RGBA32F); one thread per output pixel applies the box
// filter in the order rt_api.h fixes -- log2 N pairwise rounds along x, then along y,
// i.e. balanced trees over contiguous halves, then one multiply -- per channel, alpha
// included, and writes the output in the requested format and row mapping.
template <int N>
__device__ __forceinline__ float4 box_x(const float4* __restrict__ p) {
    if constexpr (N == 1) {
        return p[0];
    } else {
        const float4 a = box_x<N / 2>(p), b = box_x<N / 2>(p + N / 2);
        return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}
template <int N, int M>
__device__ __forceinline__ float4 box_y(const char* __restrict__ p, size_t pitch) {
    if constexpr (M == 1) {
        return box_x<N>(reinterpret_cast<const float4*>(p));
    } else {
        const float4 a = box_y<N, M / 2>(p, pitch), b = box_y<N, M / 2>(p + (M / 2) * pitch, pitch);
        return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}
// width, height, y0, stripe, period, out_rows: the OUTPUT frame's (rt_dispatch_rows_ex).
// DISP: the instance for the display formats (kept apart: with both stores in one kernel
// k_box_filter<8> went from 76 to 256 VGPRs).
template <int N, bool DISP = false>
__global__ __launch_bounds__(256) void k_box_filter(const char* __restrict__ src, size_t src_pitch,
                                                    char* __restrict__ dst, size_t pitch, int width, int height,
                                                    int y0, int stripe, int period, int out_rows, int format) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || r >= out_rows) return;
    const int y = y0 + r + (r / stripe) * (period - stripe);
    if (y >= height) return;  // not rendered: left untouched, as the one-sample dispatch leaves it
    float4 v = box_y<N, N>(src + static_cast<size_t>(r) * N * src_pitch + static_cast<size_t>(x) * N * sizeof(float4),
                           src_pitch);
    const float w = 1.0f / static_cast<float>(N * N);
    v = make_float4(v.x * w, v.y * w, v.z * w, v.w * w);
    if (DISP) {  // display formats: the conversion of the filtered float32 value
        store_display(dst + static_cast<size_t>(r) * pitch + static_cast<size_t>(x) * display_bytes(format), format, v);
        return;
    }
    if (format == RT_FORMAT_RGB32F) {
        float* p = reinterpret_cast<float*>(dst + static_cast<size_t>(r) * pitch) + 3 * x;
        p[0] = v.x;
        p[1] = v.y;
        p[2] = v.z;
        return;
    }
    const int row = format == RT_FORMAT_RGBA32F_IMAGE ? y : r;
    reinterpret_cast<float4*>(dst + static_cast<size_t>(row) * pitch)[x] = v;
}

// ---------------------------------------------------------------------------
// Adaptive supersampling (rt_set_adaptive, include/rt_api.h): B is the dispatch's one-sample
// frame, S its n x n frame; a pixel takes S where B contrasts with a 4-neighbour and B
// elsewhere. Frames k_accel renders (launch(), fast path): B into the context's scratch
// surface by the ordinary one-sample dispatch, then
//   k_adaptive_classify : one thread per output pixel writes the unrefined pixels and lists
//                         the refined ones (one atomic per wave);
//   k_accel_refine      : one wave per 64 / n^2 listed pixels shades their samples, per-lane
//                         walks with k_accel_tail's LDS stacks, and stores the block means.
// Every other frame (general path): the whole sample frame as for rt_set_samples, then
// k_box_filter_adaptive picks the corner sample or the box mean per pixel -- exact for every
// kernel variant, and no faster than full supersampling.

// The rule on one pair of pixels: one float32 subtraction per channel; a NaN refines.
__device__ __forceinline__ bool ad_contrast(float4 a, float4 b, float t) {
    return !(fabsf(a.x - b.x) <= t) || !(fabsf(a.y - b.y) <= t) || !(fabsf(a.z - b.z) <= t);
}

// The OUTPUT frame's row mapping (rt_dispatch_rows_ex).
struct AdRows {
    int height, y0, stripe, period, out_rows;
};
__device__ __forceinline__ int ad_image_row(const AdRows& m, int r) {
    return m.y0 + r + (r / m.stripe) * (m.period - m.stripe);
}
// Compact row r2 is one of the dispatch's own pixels' and lies at image row y.
__device__ __forceinline__ bool ad_own_row(const AdRows& m, int r2, int y) {
    return r2 >= 0 && r2 < m.out_rows && y < m.height && ad_image_row(m, r2) == y;
}

// Whether pixel (r, x) at image row y, of value p, is refined; px(r, x) reads B. Rows are
// read only where ad_own_row holds, so nothing outside the dispatch's own pixels is touched.
template <class Px>
__device__ __forceinline__ bool ad_refines(const AdRows& m, int width, int r, int x, int y, float thr, float4 p,
                                           Px px) {
    bool ref = false;
    if (x > 0) ref = ref || ad_contrast(p, px(r, x - 1), thr);
    if (x + 1 < width) ref = ref || ad_contrast(p, px(r, x + 1), thr);
    if (ad_own_row(m, r - 1, y - 1)) ref = ref || ad_contrast(p, px(r - 1, x), thr);
    if (ad_own_row(m, r + 1, y + 1)) ref = ref || ad_contrast(p, px(r + 1, x), thr);
    return ref;
}

// Adds the wave's refined pixels (ballot m, non-zero) to *count with one atomic; returns
// this lane's position among them.
__device__ __forceinline__ unsigned ad_append(unsigned* count, unsigned long long m) {
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == __builtin_ctzll(m)) base = atomicAdd(count, static_cast<unsigned>(__popcll(m)));
    base = static_cast<unsigned>(__shfl(static_cast<int>(base), __builtin_ctzll(m)));
    return base + static_cast<unsigned>(__popcll(m & ((1ull << lane) - 1ull)));
}

// kp: the one-sample OUTPUT frame with the dispatch's dst, pitch and format; k_lane's grid,
// so a wave is an 8x8 tile and the list stays coherent tile by tile. bsrc: B, compact rows
// of RGBA32F. list: r * width + x per refined pixel (unsigned: launch() keeps it below
// 2^32), capacity out_rows * width; *count: zeroed in stream order before this kernel.
__global__ __launch_bounds__(kBlock) void k_adaptive_classify(KParams kp, const char* __restrict__ bsrc,
                                                              size_t bpitch, float thr,
                                                              unsigned* __restrict__ list,
                                                              unsigned* __restrict__ count) {
    const PixelCoord pc = pixel_of(kp);
    bool refine = false;
    if (pc.active) {
        auto px = [&](int r, int x) {
            return reinterpret_cast<const float4*>(bsrc + static_cast<size_t>(r) * bpitch)[x];
        };
        const float4 p = px(pc.r, pc.x);
        refine = ad_refines(AdRows{kp.height, kp.y0, kp.stripe, kp.period, kp.out_rows}, kp.width, pc.r, pc.x, pc.y,
                            thr, p, px);
        if (!refine) store_px(kp, pc.r, pc.x, p);
    }
    const unsigned long long m = __ballot(refine);
    if (m) {  // wave-uniform
        const unsigned pos = ad_append(count, m);
        if (refine)
            list[pos] = static_cast<unsigned>(pc.r) * static_cast<unsigned>(kp.width) + static_cast<unsigned>(pc.x);
    }
}

// kp: the SAMPLE frame (fill_kparams with ss = n), dst / pitch / rgb the output's. One wave
// per possible chunk of 64 / n^2 listed pixels (waves past the list's end exit at once, as
// k_accel_tail's): lane l holds sample (l & (n-1), (l >> log2 n) & (n-1)) of the chunk's
// pixel l >> 2 log2 n. Every bounce walks per lane -- a wave's rays come from several
// pixels -- and a ray's value does not depend on the walk's form, so each sample has the
// bits the supersampling k_accel instance gives it; the filter is that instance's xor
// butterfly over this layout, x rounds then y rounds, then the exact 1 / n^2.
// (With the frame's own walk policy instead -- packets for camera rays and their shadows --
// the passes behind B cost the same: car 1080p n = 2, threshold 1/16, 0.418 ms against
// 0.413 all per lane; DESIGN.md "Adaptive supersampling".)
template <bool MT, bool DISP>
__global__ __launch_bounds__(kBlock) RT_ACCEL_ATTR void k_accel_refine(AccelPtrs A, const float4* __restrict__ mat,
                                                                        KParams kp,
                                                                        const unsigned* __restrict__ list,
                                                                        const unsigned* __restrict__ count) {
    extern __shared__ int lds_stack[];
    int* stk = lds_stack + threadIdx.x;
    unsigned short* stt =
        reinterpret_cast<unsigned short*>(lds_stack + static_cast<size_t>(kp.lane_stack) * blockDim.x) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int sh = 31 - __builtin_clz(kp.ss);  // log2 n
    const unsigned total = *count;
    const unsigned long long chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned long long k = (chunk << (6 - 2 * sh)) + static_cast<unsigned>(lane >> (2 * sh));
    if ((chunk << (6 - 2 * sh)) >= total) return;  // wave-uniform
    const unsigned ow = static_cast<unsigned>(kp.width >> sh);  // the output's width
    bool alive = k < total;
    int r = 0, x = 0;  // the output pixel
    Ray ray{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 1.f)};
    // the sample's image row: image_row of the sample frame at n * r is n times the output's
    auto sample_y = [&]() { return image_row(kp, r << sh) + ((lane >> sh) & (kp.ss - 1)); };
    if (alive) {
        const unsigned px = list[k];
        r = static_cast<int>(px / ow);
        x = static_cast<int>(px - static_cast<unsigned>(r) * ow);
        ray = primary_ray(kp, (x << sh) + (lane & (kp.ss - 1)), sample_y());
    }
    const bool have = alive;
    V acc = mk(0.f, 0.f, 0.f), att = mk(1.f, 1.f, 1.f);
    WalkCount wc{0u, 0u, 0u, 0u};
    for (int depth = 0; depth < kp.maxBounces; ++depth) {
        if (__ballot(alive) == 0) break;
        bounce_step<false, false, MT, !MT>(A, mat, kp, depth, ray, alive, acc, att, sample_y, stk, stt,
                                           kp.lane_stack, wc, nullptr, 0, 0);
    }
    // lanes past the list's end hold zeros; a pixel's n^2 lanes are all in or all out
    for (int b = 1; b < kp.ss * kp.ss; b <<= 1)
        acc = acc + mk(__shfl_xor(acc.x, b), __shfl_xor(acc.y, b), __shfl_xor(acc.z, b));
    const float w = 1.0f / static_cast<float>(kp.ss * kp.ss);  // a power of two: exact
    if (have && (lane & (kp.ss * kp.ss - 1)) == 0) {
        KParams ko = kp;  // the output frame's row mapping, for RT_FORMAT_RGBA32F_IMAGE
        ko.y0 = kp.y0 >> sh;
        ko.stripe = kp.stripe >> sh;
        ko.period = kp.period >> sh;
        store_px<DISP ? kStoreDisplay : kStoreFloat>(ko, r, x, make_float4(acc.x * w, acc.y * w, acc.z * w, 1.0f));
    }
}

// The general path's filter: k_box_filter with the rule applied to the corner samples
// (B(p) is sample (0, 0) of p's block: 2 (n x) / (n resX) and (n y) / (n resY) are the
// float32 values 2 x / resX and y / resY). *count: the refined pixels (rt_adaptive_stats).
template <int N, bool DISP = false>
__global__ __launch_bounds__(256) void k_box_filter_adaptive(const char* __restrict__ src, size_t src_pitch,
                                                             char* __restrict__ dst, size_t pitch, int width,
                                                             int height, int y0, int stripe, int period,
                                                             int out_rows, int format, float thr,
                                                             unsigned* __restrict__ count) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    const AdRows m{height, y0, stripe, period, out_rows};
    const int y = r < out_rows ? ad_image_row(m, r) : 0;
    const bool active = x < width && r < out_rows && y < height;
    bool refine = false;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        auto px = [&](int rr, int xx) {
            return *reinterpret_cast<const float4*>(src + static_cast<size_t>(rr) * N * src_pitch +
                                                    static_cast<size_t>(xx) * N * sizeof(float4));
        };
        v = px(r, x);
        refine = ad_refines(m, width, r, x, y, thr, v, px);
        if (refine) {
            v = box_y<N, N>(src + static_cast<size_t>(r) * N * src_pitch + static_cast<size_t>(x) * N * sizeof(float4),
                            src_pitch);
            const float w = 1.0f / static_cast<float>(N * N);
            v = make_float4(v.x * w, v.y * w, v.z * w, v.w * w);
        }
    }
    const unsigned long long rm = __ballot(refine);
    if (rm) ad_append(count, rm);
    if (!active) return;
    if (DISP) {
        store_display(dst + static_cast<size_t>(r) * pitch + static_cast<size_t>(x) * display_bytes(format), format, v);
        return;
    }
    if (format == RT_FORMAT_RGB32F) {
        float* p = reinterpret_cast<float*>(dst + static_cast<size_t>(r) * pitch) + 3 * x;
        p[0] = v.x;
        p[1] = v.y;
        p[2] = v.z;
        return;
    }
    const int row = format == RT_FORMAT_RGBA32F_IMAGE ? y : r;
    reinterpret_cast<float4*>(dst + static_cast<size_t>(row) * pitch)[x] = v;
}

__global__ void k_pack_prims(const float4* __restrict__ geo_lin, const int* __restrict__ prim_shape,
                             const int* __restrict__ prim_seq, int P, float4* __restrict__ prims) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    store_prim(prims, j, pack_prim(load_rec(geo_lin, prim_shape[j]), prim_seq[j]));
}

// Dispatch order for the next frame (rt_set_schedule): tiles sorted by the
// work their waves did in the last dispatch (node steps + primitive tests over
// the 64 lanes; unlike a duration it does not depend on what ran beside the
// tile), most first, as a counting sort over 32 half-octave buckets. The render
// kernel counts each group of kOrderThreads tiles' buckets (hist rows); group
// j's workgroup here places its tiles after every tile of a heavier bucket and
// after the tiles of the same bucket in groups < j (ranks inside a group by
// LDS atomics: order inside a bucket is arbitrary). Two histogram sets
// alternate by frame; this kernel zeroes the rows the next frame counts into.
__global__ __launch_bounds__(kOrderThreads) void k_tile_order(const unsigned* __restrict__ cost, int n,
                                                              const unsigned* __restrict__ hist,
                                                              unsigned* __restrict__ next, int next_words,
                                                              int* __restrict__ order, int xcd) {
    constexpr int kPart = kOrderThreads / kOrderBuckets;  // threads per bucket for the row sums
    __shared__ unsigned tot[kPart][kOrderBuckets], pre[kPart][kOrderBuckets];
    __shared__ unsigned start[kOrderBuckets], rank[kOrderBuckets], base[kOrderBuckets], count[kOrderBuckets];
    const int t = threadIdx.x, j = blockIdx.x, groups = gridDim.x;
    {
        const int b = t % kOrderBuckets, part = t / kOrderBuckets;
        unsigned a = 0, p = 0;
#pragma unroll 8
        for (int r = part; r < groups; r += kPart) {
            const unsigned h = hist[r * kOrderBuckets + b];
            a += h;
            p += r < j ? h : 0u;
        }
        tot[part][b] = a;
        pre[part][b] = p;
    }
    for (int w = j * kOrderThreads + t; w < next_words; w += groups * kOrderThreads) next[w] = 0u;
    __syncthreads();
    if (t < 64) {  // one wave: bucket sums, then a suffix scan (buckets from the most work down)
        unsigned a = 0, p = 0;
        if (t < kOrderBuckets) {
#pragma unroll
            for (int k = 0; k < kPart; ++k) {
                a += tot[k][t];
                p += pre[k][t];
            }
            rank[t] = 0u;
        }
        unsigned x = a;  // inclusive sum over buckets >= t
        for (int off = 1; off < kOrderBuckets; off <<= 1) {
            const unsigned y = __shfl_down(x, off);
            if (t + off < kOrderBuckets) x += y;
        }
        if (t < kOrderBuckets) {
            start[t] = x - a + p;
            base[t] = x - a;
            count[t] = a;
        }
    }
    __syncthreads();
    const int i = j * kOrderThreads + t;
    if (i < n) {
        const int b = work_bucket(cost[i]);
        const unsigned pos = start[b] + atomicAdd(&rank[b], 1u);
        if (!xcd) {
            order[pos] = i;
        } else {
            // Workgroups go to the 8 XCDs round-robin (slot s on XCD s mod 8), and each
            // XCD has its own L2. Deal the bucket's tiles (in group order, i.e. screen
            // bands) as 8 contiguous chunks, chunk c to the slots base + c, base + 8 + c,
            // ...: each XCD walks one band of the bucket at a time, and every XCD still
            // gets an eighth of every bucket (same longest-first balance).
            const unsigned cnt = count[b], q = cnt / kXcds, rem = cnt % kXcds, pb = pos - base[b];
            unsigned c, k;
            if (pb < rem * (q + 1)) {
                c = pb / (q + 1);
                k = pb % (q + 1);
            } else {
                c = rem + (pb - rem * (q + 1)) / q;
                k = (pb - rem * (q + 1)) % q;
            }
            order[base[b] + kXcds * k + c] = i;
        }
    }
}

// The cost order's input dilated (rt_debug_cost_dilate): each tile's cost replaced by
// the largest within r tiles in x and y, and the per-group bucket rows k_tile_order
// reads recounted from those. A camera that moved since the costs were recorded sees
// its heavy tiles a few tiles away from where they were; ranking their neighbourhood
// high too puts them early anyway. (r05: dilating in the render kernel instead -- each
// tile's cost raised into its 3 x 3 neighbourhood by atomic max, the last recorder of a
// neighbour counting its bucket -- took the moving car frame from 0.296 to 2.77 ms: the
// agent-scope fences between the two phases, per tile, across 8 XCDs; r05zu.)
__global__ __launch_bounds__(kOrderThreads) void k_cost_dilate(const unsigned* __restrict__ cost, int n, int tiles_x,
                                                               int r, unsigned* __restrict__ out,
                                                               unsigned* __restrict__ hist) {
    __shared__ unsigned cnt[kOrderBuckets];
    const int t = threadIdx.x, i = blockIdx.x * kOrderThreads + t;
    if (t < kOrderBuckets) cnt[t] = 0u;
    __syncthreads();
    if (i < n) {
        const int x = i % tiles_x, y = i / tiles_x, rows = (n + tiles_x - 1) / tiles_x;
        unsigned m = 0u;
        for (int yy = max(0, y - r); yy <= min(rows - 1, y + r); ++yy)
            for (int xx = max(0, x - r); xx <= min(tiles_x - 1, x + r); ++xx) {
                const int j = yy * tiles_x + xx;
                if (j < n) m = max(m, cost[j]);
            }
        out[i] = m;
        atomicAdd(&cnt[work_bucket(m)], 1u);
    }
    __syncthreads();
    if (t < kOrderBuckets) hist[blockIdx.x * kOrderBuckets + t] = cnt[t];
}

// ---------------------------------------------------------------------------
// Device animation (rt_animate): updateScene + updateBVH on the device.

// Wall::end (src/shapes/wall.hpp:16-31), host glm operation order.
__host__ __device__ V wall_end(const FlatShape& s) {
    const V n = mk(s.planeNormal.x, s.planeNormal.y, s.planeNormal.z);
    const V t1 = fabsf(n.x) > fabsf(n.y) ? normalize(mk(-n.z, 0.f, n.x)) : normalize(mk(0.f, -n.z, n.y));
    const V t2 = normalize(cross(n, t1));
    return (mk(s.wallStart.x, s.wallStart.y, s.wallStart.z) + t1 * s.wallWidth) + t2 * s.wallHeight;
}

// BoundingBox::growToInclude(shape) (BoundingBox.hpp:50-95) from an empty box:
// the points it adds, as a (lo, hi) pair; a shape that adds nothing leaves
// lo = +inf, hi = -inf.
__host__ __device__ void reference_box(const FlatShape& s, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = INFINITY;
        hi[a] = -INFINITY;
    }
    auto add = [&](V p) {
        const float v[3] = {p.x, p.y, p.z};
        for (int a = 0; a < 3; ++a) {
            lo[a] = v[a] < lo[a] ? v[a] : lo[a];
            hi[a] = hi[a] < v[a] ? v[a] : hi[a];
        }
    };
    if (s.type == RT_SPHERE) {
        const float r = s.sphereRadius;
        add(mk(s.sphereCenter.x + r, s.sphereCenter.y + r, s.sphereCenter.z + r));
        add(mk(s.sphereCenter.x - r, s.sphereCenter.y - r, s.sphereCenter.z - r));
    } else if (s.type == RT_WALL) {
        add(mk(s.wallStart.x, s.wallStart.y, s.wallStart.z));
        add(wall_end(s));
    } else if (s.type == RT_TRIANGLE) {
        if (isfinite(s.triP1.x) && isfinite(s.triP2.x) && isfinite(s.triP3.x)) {  // :52
            add(mk(s.triP1.x, s.triP1.y, s.triP1.z));
            add(mk(s.triP2.x, s.triP2.y, s.triP2.z));
            add(mk(s.triP3.x, s.triP3.y, s.triP3.z));
        }
    }
}

// CSR lists built on the host (refit_plan.h plan_refit, RefitOffsets). Per animated shape i:
//   slots  : its geo_leaf slots (bvhIndices positions)
//   prims  : its accelerator prim slots
//   wpos   : wide-record slots (4*w + s) of the local nodes above those prims
// Per reference node j that lists an animated shape (node_ids[j]):
//   node   : the animated shapes it lists (updateBVH's set, leaves + ancestors)
//   wn     : the wnodes child slots (2 * parent + side) that hold its box
//   item   : the scene-tree items (titems records) whose exact box is its box
struct AnimMaps {
    const int *ids, *slot_off, *slot_list, *prim_off, *prim_list, *wpos_off, *wpos_list;
    const int *node_ids, *node_off, *node_list;
    const int *wn_off, *wn_list, *item_off, *item_list;
    const int* ecls;       // per entry: its class when the accelerator was built (accel_bound.h)
    const int* prim_entry; // per accelerator prim: its shape's refit entry, -1 if none
    int count, nodes;
};
// the per-frame flag of a refit entry: the nodes listing it grow to hold it
// (rt_animate: updateBVH on the device; rt_update_shapes leaves the node boxes to
// rt_update_nodes, as a glBufferSubData of the shape records does)
// AF_BOX (with AF_GROW): the growth is the box the host passed for the entry (the union of
// several frames' growToInclude boxes: rtx::animate_deferred), not its current record's
enum { AF_GROW = 4, AF_BOX = 8 };

struct AnimOut {
    FlatShape* shapes;  // staging copy of the full shape array
    FlatNode* nodes;    // staging copy of the node array (authoritative boxes)
    float4 *geo_lin, *geo_leaf, *mat;
    float4* packed;                   // the packed node copies (k_pack_nodes layout)
    float4 *anodes, *lnodes, *prims;  // accelerator (null when off)
    float4 *wnodes, *titems;          // accelerator: per-parent child boxes, scene-tree items' exact boxes
    float4* pbox;                     // conservative box per prim (lo, hi), for the slot refit
    const int* prim_seq;
    float4* sbox;                     // per entry: reference box, conservative box (4 float4)
    float origin_lim;
    int mt;                           // the accelerator's wide nodes: kWideRecMt float cones, else kWideRec
    float mt_z[3];                    // MT accelerators: AccelHost::mt_z (the per-ray padding's centre Z)
    const int* prim_shape;            // accelerator: shape index per prim (AccelPtrs::prim_shape)
    int cone_cull;                    // rt_debug_cone_cull: 0 keeps every cone full
};

// One refit launch (k_refit) of flush_updates: what it reads from the pinned ring
// and how its workgroups split the work.
struct RefitArgs {
    const FlatShape* fresh;    // per entry: its current record (pinned, mapped)
    const int* flags;          // per entry: AF_GROW, AF_BOX (pinned)
    const float4* gbox;        // per entry with AF_BOX: its growth box (lo, hi; pinned), or null
    const FlatNode* nsrc;      // rt_update_nodes: the host's node records (pinned), or null
    int* report;               // pinned: set to 1 when an entry's bound changed kind
    int na, nd, nb;            // workgroups of the record, node-set and node roles
    const int4* dirty;         // slot refit work list (n_dirty entries after the nb node waves, + 1 end)
    int n_big;                 // its first n_big slots take a workgroup each, the rest a wave each
    const float4* dstatic;     // per dirty slot: the box of its prims outside the refit set (lo, hi)
    const int* dlist;          // the refit set's prims of each dirty slot (dirty[j].w ..)
    int n_dirty, rec;          // its length; the wide record size (kWideRec / kWideRecMt)
    const int* titem_ref;      // per scene-tree item: its reference leaf
    int n_items, N;
    int direct;                // node / slot roles derive the entries' boxes from `fresh` themselves
};

// A lane-strided loop over [b, e) in steps of 4 x 64 whose four loads are issued
// before any is used: a long range (a slot near a local root spans thousands of
// prims) then costs a memory latency per step, not per prim.
// nt threads (a wave or a workgroup), this one tid.
template <class Load, class Use>
__device__ __forceinline__ void range4(int b, int e, int tid, int nt, Load load, Use use) {
    for (int p0 = b + tid; p0 < e; p0 += 4 * nt) {
        decltype(load(0)) v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (p0 + nt * u < e) v[u] = load(p0 + nt * u);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (p0 + nt * u < e) use(v[u]);
    }
}
template <class Load, class Use>
__device__ __forceinline__ void range4(int b, int e, int lane, Load load, Use use) {
    range4(b, e, lane, 64, load, use);
}

struct Box4 {
    float4 a, b;
};

__device__ __forceinline__ void wave_minmax(float lo[3], float hi[3]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
}

// wave_minmax over the workgroup (up to kRefitWaves waves; every thread gets the
// result); sh: LDS scratch of the workgroup, free again on return.
constexpr int kRefitWaves = 4;
constexpr long long kDirectReads = 2048;  // rt_ctx::refit_mode auto
__device__ __forceinline__ void block_minmax(float lo[3], float hi[3], float (*sh)[6]) {
    wave_minmax(lo, hi);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) {
            sh[threadIdx.x >> 6][a] = lo[a];
            sh[threadIdx.x >> 6][3 + a] = hi[a];
        }
    __syncthreads();
    for (int k = 0; k < nw; ++k)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], sh[k][a]);
            hi[a] = fmaxf(hi[a], sh[k][3 + a]);
        }
    __syncthreads();
}

// Record role, one lane per refit entry: rewrites its records and derives its two
// boxes (the reference's growToInclude box when it grows the nodes, and the
// accelerator's conservative one) for the node and slot roles. The class of the
// bound is decided here, on the device: a shape whose bound changed kind since the
// build (a triangle collapsing to a sliver, a sphere going infinite) gets an
// infinite conservative box, so every box above it is entered and it is tested like
// an always-tested shape -- the frame stays exact -- and `report` asks the host to
// rebuild the accelerator for speed. The cones above the shape are the slot role's.
// The conservative box an entry's current record contributes to the boxes above it
// (b): its classify() box; empty if it was always tested since the build (no box
// above it); infinite if its bound changed kind since (every box above it then
// entered). Returns whether the kind changed.
__device__ bool entry_cbox(const AnimOut& o, const FlatShape& s, int was, rta::Box3& b) {
    const int cls = rta::classify(s, b, o.origin_lim, o.mt != 0);
    const bool changed = cls != was;
    if (was != rta::BOUNDED || cls != rta::BOUNDED)
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = was != rta::BOUNDED ? INFINITY : -INFINITY;
            b.hi[a] = was != rta::BOUNDED ? -INFINITY : INFINITY;
        }
    return changed;
}

__device__ void refit_record(const AnimMaps& m, const AnimOut& o, const RefitArgs& r, int i) {
    if (i >= m.count) return;
    // Every map read first: the stores below may alias them as far as the compiler
    // knows, so a read after one would wait out its own latency, in a chain. The
    // first slot and prim of each list (most entries have one of each) are prefetched
    // with their dependants.
    const int id = m.ids[i], fl = r.flags[i], was = m.ecls[i];
    const int s0 = m.slot_off[i], s1 = m.slot_off[i + 1], p0 = m.prim_off[i], p1 = m.prim_off[i + 1];
    const int slot0 = s0 < s1 ? m.slot_list[s0] : 0;
    const int prim0 = o.anodes && p0 < p1 ? m.prim_list[p0] : 0;
    const int seq0 = o.anodes && p0 < p1 ? o.prim_seq[prim0] : 0;
    const FlatShape s = r.fresh[i];
    o.shapes[id] = s;
    const GeoRec g = pack_geo(s, id);
    store_geo(o.geo_lin + 5 * static_cast<size_t>(id), g);
    store_mat(o.mat, id, s.material);
    if (s0 < s1) store_geo(o.geo_leaf + 5 * static_cast<size_t>(slot0), g);
    for (int q = s0 + 1; q < s1; ++q) store_geo(o.geo_leaf + 5 * static_cast<size_t>(m.slot_list[q]), g);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (fl & AF_BOX) {  // several frames' boxes, unioned on the host
        const float4 a = r.gbox[2 * static_cast<size_t>(i)], b = r.gbox[2 * static_cast<size_t>(i) + 1];
        lo[0] = a.x, lo[1] = a.y, lo[2] = a.z, hi[0] = b.x, hi[1] = b.y, hi[2] = b.z;
    } else if (fl & AF_GROW) {
        reference_box(s, lo, hi);  // else the nodes keep their boxes
    }
    float4* sb = o.sbox + 4 * static_cast<size_t>(i);
    sb[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    sb[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    if (!o.anodes) {
        sb[2] = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        sb[3] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        return;
    }
    // rank in the reference walk (k_pack_prims)
    if (p0 < p1) store_prim(o.prims, prim0, pack_prim(g, seq0));
    for (int q = p0 + 1; q < p1; ++q) {
        const int p = m.prim_list[q];
        store_prim(o.prims, p, pack_prim(g, o.prim_seq[p]));
    }
    rta::Box3 b;
    if (entry_cbox(o, s, was, b)) *r.report = 1;  // the host rebuilds at its next flush
    const float4 c0 = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.f), c1 = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.f);
    sb[2] = c0;
    sb[3] = c1;
    if (was != rta::BOUNDED) return;  // always tested since the build: no box above it
    for (int q = p0; q < p1; ++q) {    // the prim's box for the slot refit
        float4* pb = o.pbox + 2 * static_cast<size_t>(q == p0 ? prim0 : m.prim_list[q]);
        pb[0] = c0;
        pb[1] = c1;
    }
}

// Node role, one wave per reference node listing a refit entry: the union of the
// entries' boxes (lanes stride the list, then a wave reduction), then one grow of
// the node's box - updateBVH's growToInclude of each listed shape, entries with
// AF_GROW only - and of its content box. A single writer per node: no atomics,
// and the min/max result is the same in any order (no stored value is NaN; a NaN
// coordinate adds nothing). The same lane writes the grown box through to every
// copy the kernels read: the packed node, the accelerator's exact box, its
// parent's child copy (wnodes: exact + content box) and the scene-tree items gated
// by it. Nodes listing no entry never change, so no other copy needs refreshing.
__device__ void grow_node(const AnimMaps& m, const AnimOut& o, const RefitArgs& r, int j, float (*sh)[6]) {
    const int tid = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    struct Two {
        Box4 ref, con;
    };
    range4(m.node_off[j], m.node_off[j + 1], tid, blockDim.x,
        [&](int q) {
            const int i = m.node_list[q];
            Two v;
            if (r.direct) {  // from the record itself (no wait for the record role)
                const FlatShape s = r.fresh[i];
                float rl[3] = {INFINITY, INFINITY, INFINITY}, rh[3] = {-INFINITY, -INFINITY, -INFINITY};
                if (r.flags[i] & AF_BOX) {
                    const float4 a = r.gbox[2 * static_cast<size_t>(i)], b = r.gbox[2 * static_cast<size_t>(i) + 1];
                    rl[0] = a.x, rl[1] = a.y, rl[2] = a.z, rh[0] = b.x, rh[1] = b.y, rh[2] = b.z;
                } else if (r.flags[i] & AF_GROW) {
                    reference_box(s, rl, rh);
                }
                rta::Box3 cb;
                if (o.anodes) entry_cbox(o, s, m.ecls[i], cb);
                else cb = rta::Box3{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
                v.ref = Box4{make_float4(rl[0], rl[1], rl[2], 0.f), make_float4(rh[0], rh[1], rh[2], 0.f)};
                v.con = Box4{make_float4(cb.lo[0], cb.lo[1], cb.lo[2], 0.f), make_float4(cb.hi[0], cb.hi[1], cb.hi[2], 0.f)};
            } else {
                const float4* sb = o.sbox + 4 * static_cast<size_t>(i);
                v.ref = Box4{sb[0], sb[1]};
                v.con = Box4{sb[2], sb[3]};
            }
            return v;
        },
        [&](const Two& v) {
            const float4 a = v.ref.a, b = v.ref.b, c = v.con.a, d = v.con.b;
            lo[0] = fminf(lo[0], a.x), lo[1] = fminf(lo[1], a.y), lo[2] = fminf(lo[2], a.z);
            hi[0] = fmaxf(hi[0], b.x), hi[1] = fmaxf(hi[1], b.y), hi[2] = fmaxf(hi[2], b.z);
            clo[0] = fminf(clo[0], c.x), clo[1] = fminf(clo[1], c.y), clo[2] = fminf(clo[2], c.z);
            chi[0] = fmaxf(chi[0], d.x), chi[1] = fmaxf(chi[1], d.y), chi[2] = fmaxf(chi[2], d.z);
        });
    block_minmax(lo, hi, sh);
    block_minmax(clo, chi, sh);
    if (tid != 0) return;
    const int k = m.node_ids[j];
    FlatNode& nd = o.nodes[k];
    float mn[3] = {nd.boundsMin.x, nd.boundsMin.y, nd.boundsMin.z};
    float mx[3] = {nd.boundsMax.x, nd.boundsMax.y, nd.boundsMax.z};
    bool grew = false;
    for (int a = 0; a < 3; ++a) {  // glm::min(Min, p) = (p < Min) ? p : Min (BoundingBox.hpp:46)
        grew = grew || lo[a] < mn[a] || mx[a] < hi[a];
        mn[a] = lo[a] < mn[a] ? lo[a] : mn[a];
        mx[a] = mx[a] < hi[a] ? hi[a] : mx[a];
    }
    if (grew) {  // only then: the node-set role may be writing this record in the same launch
        nd.boundsMin = rt_vec3{mn[0], mn[1], mn[2]};
        nd.boundsMax = rt_vec3{mx[0], mx[1], mx[2]};
        const bool leaf = nd.leftChild == -1;
        const int ca = leaf ? -(nd.startShapeIdx + 1) : nd.leftChild, cb = leaf ? nd.numShapes : nd.rightChild;
        o.packed[2 * static_cast<size_t>(k)] = make_float4(mn[0], mn[1], mn[2], __int_as_float(ca));
        o.packed[2 * static_cast<size_t>(k) + 1] = make_float4(mx[0], mx[1], mx[2], __int_as_float(cb));
    }
    if (!o.anodes) return;
    float4* an = o.anodes + 4 * static_cast<size_t>(k);
    if (grew) {
        an[0] = make_float4(mn[0], mn[1], mn[2], an[0].w);
        an[1] = make_float4(mx[0], mx[1], mx[2], an[1].w);
    }
    float4 c0 = an[2], c1 = an[3];  // content box (accel.h)
    c0 = make_float4(fminf(c0.x, clo[0]), fminf(c0.y, clo[1]), fminf(c0.z, clo[2]), c0.w);
    c1 = make_float4(fmaxf(c1.x, chi[0]), fmaxf(c1.y, chi[1]), fmaxf(c1.z, chi[2]), c1.w);
    an[2] = c0;
    an[3] = c1;
    for (int qq = m.wn_off[j]; qq < m.wn_off[j + 1]; ++qq) {
        const int ws = m.wn_list[qq];
        float4* q = o.wnodes + 8 * static_cast<size_t>(ws >> 1) + 4 * (ws & 1);
        if (grew) {
            q[0] = make_float4(mn[0], mn[1], mn[2], q[0].w);
            q[1] = make_float4(mx[0], mx[1], mx[2], q[1].w);
        }
        q[2] = make_float4(c0.x, c0.y, c0.z, q[2].w);
        q[3] = make_float4(c1.x, c1.y, c1.z, q[3].w);
    }
    if (!grew) return;
    for (int q = m.item_off[j]; q < m.item_off[j + 1]; ++q) {
        float4* t = o.titems + 2 * static_cast<size_t>(m.item_list[q]);
        t[0] = make_float4(mn[0], mn[1], mn[2], t[0].w);
        t[1] = make_float4(mx[0], mx[1], mx[2], t[1].w);
    }
}

// Node-set role (rt_update_nodes), one lane per node or scene-tree item: the host's
// node records (same topology) to every copy the kernels read. k < N: node k's
// record, packed copy and accelerator exact box, and for an inner node its
// children's exact boxes in its wnodes record; k >= N: item k - N's gating box (its
// reference leaf's). Content boxes, cones and codes are the shapes' and stay.
__device__ void set_node(const AnimOut& o, const RefitArgs& r, int k) {
    const FlatNode* __restrict__ src = r.nsrc;
    if (k < r.N) {
        const FlatNode n = src[k];
        o.nodes[k] = n;
        const bool leaf = n.leftChild == -1;
        const int ca = leaf ? -(n.startShapeIdx + 1) : n.leftChild, cb = leaf ? n.numShapes : n.rightChild;
        o.packed[2 * static_cast<size_t>(k)] =
            make_float4(n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, __int_as_float(ca));
        o.packed[2 * static_cast<size_t>(k) + 1] =
            make_float4(n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, __int_as_float(cb));
        if (!o.anodes) return;
        float* a = reinterpret_cast<float*>(o.anodes + 4 * static_cast<size_t>(k));
        a[0] = n.boundsMin.x, a[1] = n.boundsMin.y, a[2] = n.boundsMin.z;
        a[4] = n.boundsMax.x, a[5] = n.boundsMax.y, a[6] = n.boundsMax.z;
        if (leaf) return;
        const int ch[2] = {n.leftChild, n.rightChild};
        for (int s = 0; s < 2; ++s) {
            const FlatNode& cn = src[ch[s]];
            float* q = reinterpret_cast<float*>(o.wnodes + 8 * static_cast<size_t>(k) + 4 * s);
            q[0] = cn.boundsMin.x, q[1] = cn.boundsMin.y, q[2] = cn.boundsMin.z;
            q[4] = cn.boundsMax.x, q[5] = cn.boundsMax.y, q[6] = cn.boundsMax.z;
        }
    } else if (k - r.N < r.n_items && o.titems) {
        const int i = k - r.N;
        const FlatNode& ln = src[r.titem_ref[i]];
        float* t = reinterpret_cast<float*>(o.titems + 2 * static_cast<size_t>(i));
        t[0] = ln.boundsMin.x, t[1] = ln.boundsMin.y, t[2] = ln.boundsMin.z;
        t[4] = ln.boundsMax.x, t[5] = ln.boundsMax.y, t[6] = ln.boundsMax.z;
    }
}

// The current record of the shape of accelerator prim p, for the slot role: the
// staging copy (which the record role has brought up to date), or with `direct` a
// moved shape's record itself.
__device__ __forceinline__ const FlatShape& slot_shape(const AnimMaps& m, const AnimOut& o, const RefitArgs& r,
                                                       int p) {
    const int e = r.direct ? m.prim_entry[p] : -1;
    return e >= 0 ? r.fresh[e] : o.shapes[o.prim_shape[p]];
}

// The slot role's back-face cone (barycentric accelerators, accel.cpp build_cones
// and shape_cone): moved walls and triangles turn their stored normals (a wheel's),
// so the child's cone is recomputed from the current records below: axis = the unit
// normals' sum, half angle = the largest angle to the stored (float) axis, plus
// kConeMargin; any other shape or a normal sum near 0 makes it full. A child whose
// cone is full already (kConeNever: the build found it so, or culling is off) keeps
// it -- a word that never culls always holds -- which spares the large subtrees
// near the roots a pass over their prims.
__device__ void refit_slot_cone(const AnimMaps& m, const AnimOut& o, const RefitArgs& r, int4 d, int w, int sl,
                                int lane) {
    int* cw = reinterpret_cast<int*>(o.lnodes + kWideRec * static_cast<size_t>(w) + 6) + sl;
    if (*cw == rta::kConeNever) return;  // the same word for the whole wave
    auto load = [&](int p) {  // the stored normal (w: 0 for a shape without a cone)
        const FlatShape& s = slot_shape(m, o, r, p);
        const bool cone = s.type == RT_WALL || s.type == RT_TRIANGLE;
        return make_float4(s.planeNormal.x, s.planeNormal.y, s.planeNormal.z, cone ? 1.f : 0.f);
    };
    auto unit_normal = [](const float4& v, double n[3]) {  // accel.cpp shape_cone
        n[0] = v.x, n[1] = v.y, n[2] = v.z;
        const double l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (v.w == 0.f || !(l > 1e-20) || !isfinite(l)) return false;
        for (int a = 0; a < 3; ++a) n[a] /= l;
        return true;
    };
    double sn[3] = {0, 0, 0};
    int full = 0;
    range4(d.y, d.z, lane, load, [&](const float4& v) {
        double n[3];
        if (!unit_normal(v, n)) {
            full = 1;
            return;
        }
        for (int a = 0; a < 3; ++a) sn[a] += n[a];
    });
    for (int off = 32; off > 0; off >>= 1) {
        for (int a = 0; a < 3; ++a) sn[a] += __shfl_xor(sn[a], off);
        full |= __shfl_xor(full, off);
    }
    const double l = sqrt(sn[0] * sn[0] + sn[1] * sn[1] + sn[2] * sn[2]);
    if (full || !(l > 1e-6) || d.y >= d.z) {
        if (lane == 0) *cw = rta::kConeNever;
        return;
    }
    float af[3];  // the axis as lane 0 rounds it (the butterfly's sums may differ in the last bits)
    for (int a = 0; a < 3; ++a) af[a] = __shfl(static_cast<float>(sn[a] / l), 0);
    const double al = sqrt(static_cast<double>(af[0]) * af[0] + static_cast<double>(af[1]) * af[1] +
                           static_cast<double>(af[2]) * af[2]);
    double cmin = 1.0;  // the smallest cosine to the axis
    range4(d.y, d.z, lane, load, [&](const float4& v) {
        double n[3];
        unit_normal(v, n);
        cmin = fmin(cmin, (n[0] * af[0] + n[1] * af[1] + n[2] * af[2]) / al);
    });
    for (int off = 32; off > 0; off >>= 1) cmin = fmin(cmin, __shfl_xor(cmin, off));
    if (lane != 0) return;
    const double t = acos(fmax(-1.0, fmin(1.0, cmin))) + rta::kConeMargin;
    *cw = t >= 1.5707 ? rta::kConeNever : rta::cone_word(af[0], af[1], af[2], static_cast<float>(-sin(t)));
}

// The slot role's Moller-Trumbore part (MT accelerators have local trees only):
// the child's grazing cone, per-ray padding constants and slab (accel.cpp
// build_cones_mt), recomputed from the current records of every triangle below,
// since a refit moves and turns them (a wheel's). Two passes over the slot's prims:
// the normals' sum (each flipped towards the old axis) gives the new axis, stored as
// float; then s = the largest min(|n - a|, |n + a|) against that stored axis (for
// any a, |d.n| >= |d.a| - |n -+ a|: what mt_pad's cone term needs) and the slab of
// a . vertex. The constants take the worst triangle as the build's do, without its
// grow-only margin. A shape other than a bounded triangle below: no slab, as built.
__device__ void refit_slot_mt(const AnimMaps& m, const AnimOut& o, const RefitArgs& r, int4 d, int w, int sl,
                              int lane) {
    float* k = wide_box_f(o.lnodes, kWideRecMt, w, sl, 0) + 6;  // axis xyz, s, {cr, u X, M, 18 M + 10.5 Esum, w, h0}
    const double a0[3] = {k[0], k[1], k[2]};                      // every lane reads before lane 0 writes
    struct Tri {
        int type;
        rt_vec3 p1, p2, p3;
    };
    auto load = [&](int p) {
        const FlatShape& s = slot_shape(m, o, r, p);
        return Tri{s.type, s.triP1, s.triP2, s.triP3};
    };
    auto as_shape = [](const Tri& v) {  // what classify_mt_tight reads
        FlatShape s{};
        s.type = v.type, s.triP1 = v.p1, s.triP2 = v.p2, s.triP3 = v.p3;
        return s;
    };
    auto tri_normal = [](const FlatShape& s, double n[3]) {  // accel.cpp mt_normal, with |e1 x e2|
        const float e1[3] = {s.triP2.x - s.triP1.x, s.triP2.y - s.triP1.y, s.triP2.z - s.triP1.z};
        const float e2[3] = {s.triP3.x - s.triP1.x, s.triP3.y - s.triP1.y, s.triP3.z - s.triP1.z};
        n[0] = static_cast<double>(e1[1]) * e2[2] - static_cast<double>(e1[2]) * e2[1];
        n[1] = static_cast<double>(e1[2]) * e2[0] - static_cast<double>(e1[0]) * e2[2];
        n[2] = static_cast<double>(e1[0]) * e2[1] - static_cast<double>(e1[1]) * e2[0];
        const double l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int a = 0; a < 3; ++a) n[a] /= l;
    };
    double sn[3] = {0, 0, 0}, cr = INFINITY, X = 0, es = 0, mm = 0;
    int other = 0;
    range4(d.y, d.z, lane, load, [&](const Tri& v) {
        const FlatShape s = as_shape(v);
        rta::MtTri t;
        rta::Box3 tb;
        if (s.type != RT_TRIANGLE || rta::classify_mt_tight(s, tb, 0.0, t) != rta::BOUNDED) {
            other = 1;
            return;
        }
        double n[3];
        tri_normal(s, n);
        const double sg = n[0] * a0[0] + n[1] * a0[1] + n[2] * a0[2] < 0 ? -1.0 : 1.0;
        for (int a = 0; a < 3; ++a) sn[a] += sg * n[a];
        const double dz[3] = {t.p1[0] - o.mt_z[0], t.p1[1] - o.mt_z[1], t.p1[2] - o.mt_z[2]};
        cr = fmin(cr, t.cr);
        X = fmax(X, t.X);
        es = fmax(es, t.esum);
        mm = fmax(mm, sqrt(dz[0] * dz[0] + dz[1] * dz[1] + dz[2] * dz[2]));
    });
    for (int off = 32; off > 0; off >>= 1) {
        for (int a = 0; a < 3; ++a) sn[a] += __shfl_xor(sn[a], off);
        cr = fmin(cr, __shfl_xor(cr, off));
        X = fmax(X, __shfl_xor(X, off));
        es = fmax(es, __shfl_xor(es, off));
        mm = fmax(mm, __shfl_xor(mm, off));
        other |= __shfl_xor(other, off);
    }
    // the axis as lane 0 rounds it (the butterfly's sums may differ in the last bits)
    const double l = sqrt(sn[0] * sn[0] + sn[1] * sn[1] + sn[2] * sn[2]);
    const bool full = !(l > 1e-6) || !(X > 0);  // no triangle, or normals cancelling: a full cone
    float af[3];
    for (int a = 0; a < 3; ++a) af[a] = __shfl(full ? static_cast<float>(a0[a]) : static_cast<float>(sn[a] / l), 0);
    double sm = 0, lo = INFINITY, hi = -INFINITY;
    range4(d.y, full ? d.y : d.z, lane, load, [&](const Tri& v) {
        const FlatShape s = as_shape(v);
        rta::MtTri t;
        rta::Box3 tb;
        if (s.type != RT_TRIANGLE || rta::classify_mt_tight(s, tb, 0.0, t) != rta::BOUNDED) return;
        double n[3], dm = 0, dp = 0;
        tri_normal(s, n);
        for (int a = 0; a < 3; ++a) {
            dm += (n[a] - af[a]) * (n[a] - af[a]);
            dp += (n[a] + af[a]) * (n[a] + af[a]);
        }
        sm = fmax(sm, sqrt(fmin(dm, dp)));
        for (const rt_vec3& v : {s.triP1, s.triP2, s.triP3}) {
            const double x = static_cast<double>(af[0]) * v.x + static_cast<double>(af[1]) * v.y +
                             static_cast<double>(af[2]) * v.z;
            lo = fmin(lo, x);
            hi = fmax(hi, x);
        }
    });
    for (int off = 32; off > 0; off >>= 1) {
        sm = fmax(sm, __shfl_xor(sm, off));
        lo = fmin(lo, __shfl_xor(lo, off));
        hi = fmax(hi, __shfl_xor(hi, off));
    }
    if (lane != 0) return;
    const double up = 1.0 + 1e-5, sv = sm * (1.0 + 1e-6) + 2e-5;
    k[0] = af[0], k[1] = af[1], k[2] = af[2];
    // build_cones_mt: theta >= 1.5 is a full cone; so is every cone with culling off (the build's)
    k[3] = full || sv >= 1.3633 || !o.cone_cull ? 2.f : static_cast<float>(sv);
    if (!(X > 0)) {  // no triangle below: pad 0, no slab
        for (int a = 4; a < 9; ++a) k[a] = 0.f;
        k[9] = INFINITY;
        return;
    }
    k[4] = static_cast<float>(cr * (1.0 - 1e-5));
    k[5] = static_cast<float>(rta::kU * X * up);
    k[6] = static_cast<float>(mm * up + 1e-5);
    k[7] = static_cast<float>((18.0 * mm + 10.5 * es) * up + 1e-5);
    const bool slab = !full && !other && lo <= hi;
    const double wc = slab ? 0.5 * (lo + hi) : 0.0;
    k[8] = static_cast<float>(wc);
    k[9] = slab ? static_cast<float>(0.5 * (hi - lo) * up + 1e-5 * (fabs(wc) + 1.0)) : INFINITY;
}

// Slot role: exact refit of the local / scene-tree boxes above moved prims (they
// are the accelerator's own, so unlike the reference nodes they may shrink): one
// workgroup per dirty wide-record slot, the union of the box of the slot's prims
// that are not in the refit set (fixed: prepare_animation, dstatic) and of pbox over
// those that are (dlist) -- a subtree's prims are contiguous (accel.cpp
// LocalBuilder), the scene tree's top slots span every prim (the car: 4,020, against
// 640 refit prims). dirty[j] = (4*w + s, first prim, end prim, first of its dlist
// entries); dirty[j + 1].w ends them.
__device__ void refit_slot(const AnimMaps& m, const AnimOut& o, const RefitArgs& r, int j, float (*sh)[6],
                           bool block) {
    const int tid = block ? threadIdx.x : threadIdx.x & 63, lane = tid & 63;
    const int4 d = r.dirty[j];
    const float4* __restrict__ pbox = o.pbox;
    const float4 s0 = r.dstatic[2 * j], s1 = r.dstatic[2 * j + 1];
    float lo[3] = {s0.x, s0.y, s0.z}, hi[3] = {s1.x, s1.y, s1.z};
    range4(d.w, r.dirty[j + 1].w, tid, block ? static_cast<int>(blockDim.x) : 64,
        [&](int q) {
            const int p = r.dlist[q];
            const int e = r.direct ? m.prim_entry[p] : -1;
            if (e >= 0 && m.ecls[e] == rta::BOUNDED) {  // a moved prim, from its record itself
                rta::Box3 cb;
                entry_cbox(o, r.fresh[e], rta::BOUNDED, cb);
                return Box4{make_float4(cb.lo[0], cb.lo[1], cb.lo[2], 0.f), make_float4(cb.hi[0], cb.hi[1], cb.hi[2], 0.f)};
            }
            return Box4{pbox[2 * static_cast<size_t>(p)], pbox[2 * static_cast<size_t>(p) + 1]};
        },
        [&](const Box4& v) {
            const float4 a = v.a, b = v.b;
            lo[0] = fminf(lo[0], a.x), lo[1] = fminf(lo[1], a.y), lo[2] = fminf(lo[2], a.z);
            hi[0] = fmaxf(hi[0], b.x), hi[1] = fmaxf(hi[1], b.y), hi[2] = fmaxf(hi[2], b.z);
        });
    if (block)
        block_minmax(lo, hi, sh);
    else
        wave_minmax(lo, hi);
    if (tid >= 64) return;  // the cones: one wave
    const int w = d.x >> 2, sl = d.x & 3;
    if (lane < 6) {  // rows 0-5 of the wide record: lo.xyz, hi.xyz
        const float v = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lane == 3 ? hi[0] : lane == 4 ? hi[1] : hi[2];
        *wide_box_f(o.lnodes, r.rec, w, sl, lane) = v;
    }
    if (o.mt)
        refit_slot_mt(m, o, r, d, w, sl, lane);
    else
        refit_slot_cone(m, o, r, d, w, sl, lane);
}

// The per-frame refit of flush_updates, in workgroups of four roles:
//   [0, na)             record role (refit_record), a lane per entry;
//   [na, na + nd)       node-set role (set_node), a lane per node or item;
//   [na + nd, ...)      a workgroup each: node role (grow_node) for the first nb, then
//                       slot role (refit_slot); both read what the record role wrote.
// Launch shapes (rt_debug_refit), on the car's wheels (640 entries, 650 dirty slots):
//   1 two launches, records and node sets in one-wave workgroups, then nodes and slots
//     in kRefitWaves-wave ones: the kernel boundary orders them (11.4 + 8.4 us, no gap
//     between them; r05n);
//   2 one launch whose node / slot roles derive each entry's boxes from its record over
//     the host link themselves (direct; 72 us on the car, 4 us less than mode 1 for a
//     few records: what the auto policy picks up to kDirectReads).
// Tried and removed: one launch whose node / slot workgroups waited on a flag in global
// memory for the record workgroups (29-52 us, and the wait relied on a start order HIP
// does not promise; profiles/r05x_refit_record_probe.txt, r06_anim_probe_modes.txt), and
// the records copied to the device first (no faster). CHANGELOG has the measurements.
// The node-set role never runs with AF_GROW entries in the same flush (flush_updates
// applies host node records first), so no two roles write the same box.
__global__ __launch_bounds__(64 * kRefitWaves) void k_refit(AnimMaps m, AnimOut o, RefitArgs r) {
    __shared__ float sh[kRefitWaves][6];
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned t = blockIdx.x;
    if (t < static_cast<unsigned>(r.na)) {
        refit_record(m, o, r, static_cast<int>(t) * nt + tid);
        return;
    }
    t -= r.na;
    if (t < static_cast<unsigned>(r.nd)) {
        set_node(o, r, static_cast<int>(t) * nt + tid);
        return;
    }
    t -= r.nd;
    const int w = static_cast<int>(t) - r.nb;
    if (w < 0) {
        grow_node(m, o, r, w + r.nb, sh);
        return;
    }
    const int nbig = min(r.n_big, r.n_dirty);
    if (w < nbig) {
        refit_slot(m, o, r, w, sh, true);  // a long list: the whole workgroup
        return;
    }
    const int j = nbig + (w - nbig) * (nt >> 6) + (tid >> 6);  // a wave per slot
    if (j < r.n_dirty) refit_slot(m, o, r, j, sh, false);
}

// Scene-tree wide slots of the unbounded subtree (kNoPrune): their boxes are the
// reference leaves' padded boxes, which animation grows; while a set is animated
// they are infinite (entered by every ray; the items' exact boxes still gate).
__global__ void k_inf_slots(const int* __restrict__ slots, int n, float4* __restrict__ lnodes, int rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int w = slots[i] >> 2, sl = slots[i] & 3;
    for (int r = 0; r < 6; ++r) *wide_box_f(lnodes, rec, w, sl, r) = r < 3 ? -INFINITY : INFINITY;
}

}  // namespace

// ===========================================================================
// C ABI

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // used once the ring is full
    hipEvent_t sync_ev = nullptr;                  // rt_sync's poll target
    // rt_sync_frame: a latency-mode cost frame records frame_ev between its render and the
    // order's kernels (same stream), and the waited frame ends there (rt_debug_frame_event)
    int frame_event = 1;
    hipEvent_t frame_ev = nullptr;
    bool frame_ev_set = false;         // this context's last launch recorded frame_ev
    rt_ctx* frame_from = nullptr;      // the context whose launch rendered the last dispatch
    unsigned long long refit_launches = 0;  // k_refit launches so far
    unsigned long long frame_refits = 0;    // those of this context + sub-contexts at that dispatch
    hipEvent_t last0 = nullptr, last1 = nullptr;  // events of the latest dispatch
    bool timed = false;
    // per-dispatch event pairs since the last rt_kernel_times call
    std::vector<hipEvent_t> ring0, ring1;
    int ring_used = 0;
    bool timing = true;  // rt_set_kernel_timing: record the ring's events around each render
    // scene
    float4 *geo_lin = nullptr, *geo_leaf = nullptr, *mat = nullptr, *nodes = nullptr;
    int S = 0, N = 0, I = 0, max_stack = 1;
    bool have_scene = false, have_cam = false, have_light = false;
    std::vector<FlatNode> host_nodes;  // topology check for rt_update_nodes
    FlatShape* staging_shapes = nullptr;
    size_t staging_shapes_cap = 0;
    FlatNode* staging_nodes = nullptr;
    size_t staging_nodes_cap = 0;
    int* staging_idx = nullptr;
    size_t staging_idx_cap = 0;
    std::vector<int> host_idx;
    std::vector<FlatShape> host_shapes;
    // exact-result accelerator (accel.h); device copies in the layouts of AccelPtrs
    float4 *anodes = nullptr, *lnodes = nullptr, *wnodes = nullptr, *prims = nullptr;
    int4* tleaf = nullptr;
    float4* titems = nullptr;  // scene-tree items (AccelPtrs::titems)
    int* titem_ref = nullptr;  // per titems record: its reference leaf (device copy)
    std::vector<int> host_titem_ref;  // the same on the host (prepare_animation: items of a grown leaf)
    int n_titems = 0;
    int* anim_inf_slots = nullptr;  // wide slots whose boxes go infinite while animating (kNoPrune)
    int n_inf_slots = 0;
    bool inf_open = false;          // open_inf_slots ran since the accelerator was built
    int st_root = 0x7fffffff;  // scene-tree root code, kNoChild if none
    int tree_mode = 1;         // rt_set_tree
    int scene_stack = 0;       // rt_debug_scene_stack (0: the walk's own cap)
    int nfew = 0;              // few-leaf mode (AccelPtrs::nfew)
    int* prim_idx_dev = nullptr;
    bool accel_ok = false;
    size_t record_bytes = 0;   // device records k_accel reads (rt_accel_info::record_bytes)
    int boxes_finite = 0;
    rta::AccelHost accel;
    // frame constants
    FlatCamera cam{};
    FlatLight light{};                       // light 0: the one light of every existing kernel
    FlatLight lights[RT_MAX_LIGHTS]{};       // rt_set_lights: the whole set (lights[0] == light)
    int nlights = 1;                         // its size; >= 2: the k_lights kernels (rtp::lights_route)
    float soft_radii[RT_MAX_LIGHTS]{};       // rt_set_soft_shadows: light i's radius (0 from soft_count on)
    int soft_count = 0;                      // 0: off; a radius > 0 below nlights: the k_soft kernels
    int soft_samples = 0;                    // K (rtp::soft_route)
    int soft_form = 0;  // rt_debug_soft: 0 = the default form of later bounces' samples, 1 = repacked, 2 = per lane
    rt_params params{0.f, 0.f, 0, 0, 0, 0};  // the reference's first frame sees zeros
    bool have_params = false;                // rt_set_params was called (rt_trace_pixels needs resX / resY)
    // rt_trace_rays_host / rt_trace_pixels: staging for the rays (or pixels) and the hits,
    // grown on demand and kept between calls
    float4* trace_in = nullptr;
    size_t trace_in_cap = 0;
    float4* trace_hits = nullptr;
    size_t trace_hits_cap = 0;
    // rt_gbuffer_host: staging for the four planes, grown on demand and kept between calls
    float4* gbuf_stage = nullptr;
    size_t gbuf_stage_cap = 0;
    int gbuf_walk = 0;    // rt_debug_gbuffer: 1 = the accelerated form walks per lane (diagnostics)
    int gbuf_waves = 0;   // rt_debug_gbuffer: waves (tiles) per block, 0 = the default
    // rt_ao_host: staging for the two planes, grown on demand and kept between calls
    float* ao_stage = nullptr;
    size_t ao_stage_cap = 0;
    int ao_form = 0;      // rt_debug_ao: 0 = the default form (per hit lane), 1 = repacked, 2 = per hit lane
    int ao_waves = 0;     // rt_debug_ao: waves (tiles) per block, 0 = the default
    // rt_shade_rays_host / rt_camera_rays_host: staging for the rays and the pixels, grown on
    // demand and kept between calls
    float4* shade_in = nullptr;
    size_t shade_in_cap = 0;
    float4* shade_out = nullptr;
    size_t shade_out_cap = 0;
    int shade_split = 0;  // rt_debug_shade: 0 = the default k_shade instance, 1 = plain walks, 2 = split walks
    int kernel = RT_KERNEL_AUTO;
    int last_kind = 0;
    // own surface
    float* img = nullptr;
    size_t img_pitch = 0;
    int img_w = 0, img_h = 0;
    int img_fmt = RT_FORMAT_RGBA32F;   // the allocated surface's format
    int surf_fmt = RT_FORMAT_RGBA32F;  // rt_set_surface_format: the next rt_dispatch's
    // rt_set_samples: n x n samples per pixel. Frames k_accel renders reduce them in its
    // store (the SS instances); every other frame renders the sample frame into ss_buf
    // (compact rows, RGBA32F; kept between frames, reallocated when the size changes) and
    // k_box_filter writes the output. ss_general: rt_debug_ss_general forces the latter.
    int samples = 1;
    bool ss_general = false;
    bool convert_pass = false;  // rt_debug_convert_pass
    char* ss_buf = nullptr;
    size_t ss_bytes = 0;
    // rt_set_adaptive: with samples > 1 and adaptive >= 0 a dispatch refines only the pixels
    // whose one-sample value contrasts with a neighbour's. Frames k_accel renders: the
    // one-sample frame B into ss_buf (sized for the output frame), k_adaptive_classify,
    // k_accel_refine over ad_list; every other frame: the sample frame into ss_buf and
    // k_box_filter_adaptive. ad_count: the refined pixels, zeroed in stream order by each
    // adaptive dispatch; ad_from: the context (this one, brute or mtc) whose ad_count and
    // ad_pixels are the last adaptive dispatch's (rt_adaptive_stats).
    float adaptive = -1.0f;
    unsigned* ad_list = nullptr;
    size_t ad_cap = 0;
    unsigned* ad_count = nullptr;
    unsigned long long ad_pixels = 0;
    bool ad_ran = false;  // the last launch() ran adaptively
    rt_ctx* ad_from = nullptr;
    unsigned long long* stats_dev = nullptr;
    int cu_count = 256;
    int lane_from_depth = -1;  // bounces >= this use the per-lane walk (0: all, large: none;
                               // -1: auto, see walk_from)
    int cone_cull = 1;
    int split_max = kSplitMax, split_g = kSplitGroup;  // split per-lane walks (rt_debug_split)
    int heavy_k = kHeavyTiles, heavy_parts = kHeavyParts;  // heaviest tiles as several waves (rt_debug_heavy)
    int lane_k = -1, lane_k_mode = 2;  // heaviest slots' walk modes (rt_debug_lane_k; -1: auto)
    int cost_time = -1;                // tile cost: 0 lane work, else wave wall time (rt_debug_cost_time)
    int latency_mode = 0;              // rt_set_latency_mode
    int* tile_order = nullptr;  // diagnostics (rt_debug_tile_order): fixed dispatch order of the 8x8 tiles
    int tile_order_n = 0;
    // rt_set_schedule: per-tile durations of the last dispatch and the order derived from them
    int schedule = RT_SCHED_COST;
    unsigned* sched_cost = nullptr;
    unsigned long long* heavy_acc = nullptr;  // split heavy tiles' part counts + sums (cost-recording dispatches)
    size_t heavy_acc_cap = 0;
    int* sched_order = nullptr;
    unsigned* sched_sets = nullptr;      // 2 sets of per-group bucket histograms, alternating by frame
    int sched_parity = 0;
    int sched_cap = 0, sched_valid = 0;  // buffer capacity; tile count the order is for (0: none)
    // The order is re-derived on every sched_period-th dispatch (and whenever the tile
    // count changes); the dispatches between reuse it and record no work counts. 16:
    // car in flight -1.0 % against 8 (32: -0.9 %, 4: +1.5 %; profiles/r04z2_*)
    int sched_period = 16, sched_frame = 0;
    int cost_dilate = 0;                 // rt_debug_cost_dilate: radius in tiles (0: off)
    // The cost order of a dispatch whose camera differs from the last accelerated
    // dispatch's (rt_debug_moving; period 0: as any other): re-derived after every such
    // dispatch from whole-tile wall times dilated by one tile. The car's waited frame
    // along the orbit / dolly paths of bench.py --camera-path, against the same cameras
    // held still (median ratio over 8 cameras, tools/camera_probe.py, r05h / r05i):
    // the still policy (every 16th frame, undilated) 1.53 / 1.46; every frame undilated
    // 1.26; every 4th dilated by 2 1.16; every frame dilated by 1 1.09 / 1.06, with split
    // tiles on those frames 1.15 / 1.14 (a split tile ranked by its parts' sum), 1.15-1.19 by
    // half or a quarter of it, 1.18 / 1.13 by its longest part (r05z, r05z2).
    int moving_period = 1, moving_dilate = 1, moving_split = 0;
    FlatCamera sched_cam{};
    bool have_sched_cam = false;
    bool moving = false;  // this dispatch's camera moved
    unsigned* dil_cost = nullptr;        // its dilated costs (sched_cap) + bucket rows
    size_t dil_cap = 0;
    // compaction (rt_set_tail): bounces >= tail_from run in k_accel_tail (0: off)
    int tail_from = RT_TAIL_AUTO;
    float4* tail_queue = nullptr;
    size_t tail_cap = 0;     // queue entries
    int* tail_counts = nullptr;  // two sets of per-region counters, alternating by dispatch
    int tail_regions_cap = 0;
    int tail_max_lanes = 64;  // rt_debug_tail_lanes
    int shadow_walk_override = -1;  // rt_debug_shadow_walk (-1: policy)
    int tail_parity = 0;
    int lane_stack_override = 0;  // diagnostics only (rt_debug_lane_stack): breaks exactness if too small
    unsigned long long* tile_times = nullptr;  // diagnostics (rt_debug_tile_times)
    size_t tile_times_cap = 0;
    // animation (rt_set_animated / rt_animate) and the reference's own uploads
    // (rt_update_shapes / rt_update_nodes), both applied by the device refit
    std::vector<int> anim_ids;          // rt_set_animated's set, in rt_animate's record order
    // The refit set: every shape moved since the accelerator was built (the animated
    // set plus the shapes rt_update_shapes rewrote). One entry each; AnimMaps lists them.
    std::vector<int> refit_ids;
    std::vector<int> refit_of;          // per shape: its refit entry, -1 if none
    std::vector<int> anim_cls;          // per refit entry: accelerator class at the last build (accel_bound.h)
    std::vector<FlatShape> anim_base;   // per refit entry: the record the accelerator's cones were built from
    // rt_update_shapes / rt_update_nodes only write the host copies; the next device
    // operation (flush_updates) applies them in one refit, like glBufferSubData
    // calls that take effect at the next dispatch.
    std::vector<int> upd_ids;           // shapes written since the last flush
    std::vector<char> upd_mark;         // per shape: listed in upd_ids
    std::vector<std::pair<int, FlatShape>> upd_base;  // their build-time records (shapes new to the refit set)
    bool nodes_dirty = false;           // host_nodes newer than every device copy
    bool nodes_rebuild = false;         // host_nodes break a condition the accelerator was built on
    bool bounds_rebuild = false;        // a refit reported a shape whose bound changed kind
    int updates_flushed = 0;            // flushes that refit instead of rebuilding (diagnostics)
    // rt_debug_refit: 1 two launches (records and node sets, then the box roles), 2 one
    // launch (box roles read the records over the host link themselves); -1 auto: mode 2
    // while the records its readers fetch over the host link are few (direct_reads <=
    // kDirectReads), else mode 1. Waited animated frames, mode 1 against 2: config 2's
    // three spheres (~50 reads) 0.1062 against 0.1024 ms; the car's wheels (~7,500 reads)
    // 0.2449 against 0.2777 (r05q)
    int refit_mode = -1;
    long long direct_reads = 0, n_direct_slot_reads = 0;
    long long dirty_sum = 0;  // rt_debug_refit_stats: the slot refit's prim ranges (largest, total)
    long long last_flush_bytes = 0;  // rt_debug_refit_stats: the pinned records of the last flush
    int refit_compactions = 0;       // rt_debug_refit_stats: stale entries dropped (compact_refit_set)
    int dirty_max = 0;
    int* anim_maps = nullptr;           // AnimMaps lists, one allocation
    size_t anim_maps_cap = 0;
    AnimMaps anim{};
    // Per-frame records, FlatShape[count] then int flags[count]: a ring of pinned, mapped
    // host buffers that k_refit reads directly, so a flush waits only for the
    // k_refit kAnimRing flushes back (not for the previous frame's render). Each slot
    // ends in a report word k_refit sets when a shape's bound changed kind.
    static constexpr int kAnimRing = 3;
    void* anim_pinned[kAnimRing] = {nullptr, nullptr, nullptr};
    void* anim_pinned_dev[kAnimRing] = {nullptr, nullptr, nullptr};  // the same buffers as the device sees them
    size_t anim_pinned_cap[kAnimRing] = {0, 0, 0};
    hipEvent_t anim_copied[kAnimRing] = {nullptr, nullptr, nullptr};  // that slot's k_refit has run
    size_t report_at[kAnimRing] = {0, 0, 0};       // offset of the slot's report word
    bool report_pending[kAnimRing] = {false, false, false};  // its k_refit not yet checked
    bool slot_busy[kAnimRing] = {false, false, false};       // a k_refit reads it (anim_copied ends that)
    // The slot of the last k_refit whose anim_copied is not recorded yet. An event
    // costs the stream ~6 us wherever it sits (the car's animated frame: between k_refit
    // and the render kernel it held the render kernel back, behind the render kernel
    // it delayed rt_sync's own event; rocprofv3 --hip-trace, r05h / r05i), so it is
    // recorded only when needed: before the next k_refit (frames in flight), or when
    // the slot is wanted back. A wait that drains the stream (rt_sync) retires it
    // unrecorded (stream_drained).
    int mark_slot = -1;
    int anim_slot = 0;
    float4* anim_sbox = nullptr;        // per animated shape boxes (AnimOut::sbox)
    size_t anim_sbox_cap = 0;
    float4* pbox = nullptr;             // per prim conservative box (AnimOut::pbox)
    int4* refit_dirty = nullptr;        // k_refit's slot work list (RefitArgs::dirty)
    int n_big = 0;                      // its first n_big slots have long refit lists (RefitArgs::n_big)
    float4* refit_static = nullptr;     // RefitArgs::dstatic
    int* refit_list = nullptr;          // RefitArgs::dlist
    int n_dirty = 0;
    int anim_rebuilds = 0;              // host rebuilds rt_animate fell back to (diagnostics)
    // A refit that asks for a rebuild (a bound changed kind, or the node boxes stopped
    // nesting) starts it on a host thread over a snapshot of the records (AsyncBuild) and
    // the frames go on meanwhile, exact: a changed-kind shape is entered through every box
    // above it (k_refit), and while the boxes do not nest the rays walk the reference tree
    // (st_suspended). The first device operation after the build finishes swaps the new
    // accelerator in and refits it to the records written since the snapshot. rt_debug_
    // async_rebuild(0): the rebuild runs in the flush that asked for it, as before round 6.
    struct AsyncBuild {
        std::thread th;
        std::atomic<bool> done{false};
        bool ok = false;
        rta::AccelHost A;
        std::vector<FlatShape> shapes;  // the snapshot the accelerator is built from
        std::vector<FlatNode> nodes;
    };
    std::unique_ptr<AsyncBuild> rebuild;
    // The last swapped-in build's object, kept for the next rebuild: its snapshot buffers
    // are refilled in place, and its A (the replaced accelerator's host arrays) is
    // released by the next build on its thread -- freeing ~30-100 MB at the swap took
    // 5-11 ms of the frame on config 5 (munmap).
    std::unique_ptr<AsyncBuild> spare;
    int async_rebuild = 1;
    bool st_suspended = false;          // the scene tree is off until the rebuild lands
    int async_swaps = 0;                // rebuilt accelerators swapped in (diagnostics)
    bool nodes_on_device_newer = false; // staging_nodes grew past host_nodes
    // The root node's box as the next render sees it, kept on the host without a
    // readback: set from the records by rt_upload_scene / rt_update_nodes, grown by
    // rt_animate as k_refit grows it (reference_box of every animated shape the root
    // lists). rt_group computes its sky-row band from it (rtx::view_root).
    float root_lo[3] = {0.f, 0.f, 0.f}, root_hi[3] = {0.f, 0.f, 0.f};
    std::vector<char> entry_root;       // per refit entry: node N-1 lists it (k_refit grows the root by it)
    // rtx::animate_deferred (rt_group's frame slots): per animated shape (anim_ids order)
    // the union of the growToInclude boxes of every frame given since the last flush
    // (lo xyz, hi xyz), applied by the next flush as that shape's growth (AF_BOX)
    std::vector<float> grow_box;
    bool grow_pending = false;
    // per shape: its host record may differ from the one AccelHost::shape_cls / shape_box
    // were classified from (the build's, or prepare_animation's since): prepare_animation
    // then classifies it again and caches the result there
    std::vector<char> shape_moved;
    // The brute-force branch (useBVH = 0, gpu_shader.comp:523-620) tests every shape in
    // index order, keeps the strict-< first minimum and stops shadows at the first
    // occluder: exactly the BVH branch walking a tree of ONE leaf that lists shapes
    // 0..S-1 in order under an infinite box (which every ray with a non-NaN slab passes,
    // and for which a NaN ray gets no hit in either branch), except for the shadow
    // offset, 1e-5 instead of 1e-3 (:565 vs :469). `brute` is that second context: the
    // same shapes over the one-leaf tree, with its own accelerator, on this stream.
    rt_ctx* brute = nullptr;
    bool brute_stale = true;            // shapes changed since brute's upload
    int brute_accel = 1;                // rt_set_brute_accel
    // Moller-Trumbore frames (useMollerTrumbore = 1) render through `mtc`: the same
    // scene with its accelerator built for the MT test (accel.h AccelHost::mt).
    rt_ctx* mtc = nullptr;
    bool mtc_stale = true;              // shapes or nodes changed since mtc's upload
    bool build_mt = false;              // this context's accelerator is built for MT
};

namespace {

hipError_t sync_stream(rt_ctx* c);  // hipStreamSynchronize + the refit slots retired (below)

#pragma clang diagnostic ignored "-Wunused-result"
#define HIP_TRY(x)                                  \
    do {                                            \
        hipError_t e__ = (x);                       \
        if (e__ != hipSuccess) return RT_ERR_DEVICE; \
    } while (0)

int set_dev(rt_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    return RT_OK;
}

template <class T>
int ensure_staging(T*& p, size_t& cap, size_t n) {
    if (n <= cap && p) return RT_OK;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : sizeof(T)) != hipSuccess) return RT_ERR_NO_MEMORY;
    cap = n;
    return RT_OK;
}

// The dispatch path's device buffers (launch() and the steps under it): `p` of capacity `cap`
// (in the caller's units) freed, and allocated again with `bytes` for capacity n. The caller
// decides when (too small; ss_buf: any other size) and what precedes it (ss_buf, ad_list:
// the stream's work). `zero`: zeroed on the context's stream before it counts as there;
// otherwise the contents are undefined.
template <class T, class C>
void drop_buffer(T*& p, C& cap) {
    hipFree(p);
    p = nullptr;
    cap = 0;
}
template <class T, class C>
int renew_buffer(rt_ctx* c, T*& p, C& cap, C n, size_t bytes, bool zero = false) {
    drop_buffer(p, cap);
    if (hipMalloc(&p, bytes) != hipSuccess) return RT_ERR_NO_MEMORY;
    if (zero) HIP_TRY(hipMemsetAsync(p, 0, bytes, c->stream));
    cap = n;
    return RT_OK;
}

void free_accel(rt_ctx* c) {
    hipFree(c->anodes);
    hipFree(c->lnodes);
    hipFree(c->wnodes);
    hipFree(c->tleaf);
    hipFree(c->titems);
    c->titems = nullptr;
    hipFree(c->titem_ref);
    c->titem_ref = nullptr;
    c->n_titems = 0;
    c->host_titem_ref.clear();
    hipFree(c->anim_inf_slots);
    c->anim_inf_slots = nullptr;
    c->n_inf_slots = 0;
    c->inf_open = false;
    c->st_root = kNoChild;
    hipFree(c->prims);
    hipFree(c->prim_idx_dev);
    hipFree(c->pbox);
    hipFree(c->refit_dirty);
    hipFree(c->refit_static);
    hipFree(c->refit_list);
    c->pbox = nullptr;
    c->refit_dirty = nullptr;
    c->refit_static = nullptr;
    c->refit_list = nullptr;
    c->n_dirty = 0;
    c->anodes = c->lnodes = c->wnodes = c->prims = nullptr;
    c->tleaf = nullptr;
    c->prim_idx_dev = nullptr;
    c->accel_ok = false;
}

void discard_rebuild(rt_ctx* c);
void free_scene(rt_ctx* c) {
    discard_rebuild(c);
    hipFree(c->geo_lin);
    hipFree(c->geo_leaf);
    hipFree(c->mat);
    hipFree(c->nodes);
    c->geo_lin = c->geo_leaf = c->mat = c->nodes = nullptr;
    free_accel(c);
    c->have_scene = false;
}

// Checks the arrays the way the reference shader would dereference them and
// measures the reference walk's worst-case stack need (every box hit).
int check_tree(const FlatNode* nodes, int N, const int* idx, int I, int S, int* max_stack) {
    for (int i = 0; i < I; ++i)
        if (idx[i] < 0 || idx[i] >= S) return RT_ERR_BVH;
    for (int k = 0; k < N; ++k) {
        const FlatNode& n = nodes[k];
        if (n.leftChild == -1) {
            if (n.numShapes > 0 && (n.startShapeIdx < 0 || n.startShapeIdx > I - n.numShapes)) return RT_ERR_BVH;
        } else if (n.leftChild < 0 || n.leftChild >= N || n.rightChild < 0 || n.rightChild >= N) {
            return RT_ERR_BVH;
        }
    }
    int ms = N > 0 ? 1 : 0;
    if (N > 0) {
        std::vector<int> st;
        st.push_back(N - 1);
        long long visits = 0;
        while (!st.empty()) {
            int k = st.back();
            st.pop_back();
            if (++visits > 4ll * N + 8) return RT_ERR_BVH;  // cycle or exploding DAG
            if (nodes[k].leftChild != -1) {
                st.push_back(nodes[k].leftChild);
                st.push_back(nodes[k].rightChild);
                ms = static_cast<int>(st.size()) > ms ? static_cast<int>(st.size()) : ms;
            }
        }
    }
    if (ms > kMaxStack) return RT_ERR_BVH;
    *max_stack = ms;
    return RT_OK;
}

// Builds the accelerator from the host copies of the scene and uploads it;
// expects geo_lin to be packed (k_pack_prims copies from it). On failure the
// context keeps rendering with k_packet.
int upload_built_accel(rt_ctx* c);

// The packed host arrays are the device's float4 / int4 as they stand (accel_pack.h).
static_assert(sizeof(rta::F4) == sizeof(float4) && alignof(rta::F4) == alignof(float4), "F4 uploads as float4");
static_assert(sizeof(rta::I4) == sizeof(int4) && alignof(rta::I4) == alignof(int4), "I4 uploads as int4");

// A device array to allocate and the host array it is filled from (null: allocated only).
struct HostArray {
    void** dev;
    const void* src;
    size_t bytes;
};
template <class D, class T>
HostArray host_array(D*& dev, const T* src, size_t count) {
    static_assert(sizeof(D) == sizeof(T), "copied element for element");
    return HostArray{reinterpret_cast<void**>(&dev), src, count * sizeof(D)};
}
// Allocates every array, then issues their copies on the context's stream, in order.
int alloc_and_copy(rt_ctx* c, std::initializer_list<HostArray> arrays, PhaseLaps* lap = nullptr) {
    for (const HostArray& a : arrays)
        if (hipMalloc(a.dev, a.bytes) != hipSuccess) return RT_ERR_NO_MEMORY;
    if (lap) (*lap)("hipMalloc");
    for (const HostArray& a : arrays)
        if (a.src) HIP_TRY(hipMemcpyAsync(*a.dev, a.src, a.bytes, hipMemcpyHostToDevice, c->stream));
    return RT_OK;
}

// built: the host build already ran (rt_upload_scene overlaps it with the records'
// device upload) and returned *built; null: build here.
int build_upload_accel(rt_ctx* c, const bool* built = nullptr) {
    PhaseLaps lap("build_upload_accel");
    free_accel(c);
    const int N = c->N;
    if (N == 0) return RT_OK;
    lap("free");
    if (built ? !*built
              : !rta::build_accel(c->host_shapes.data(), c->S, c->host_nodes.data(), N, c->host_idx.data(), c->I,
                                  kLeafScan, kMaxStack, c->accel, c->build_mt))
        return RT_OK;
    lap("host build");
    return upload_built_accel(c);
}

// The device half of build_upload_accel: c->accel (built) to the device, with the
// current host node records' exact boxes and the device's current shape records.
int upload_built_accel(rt_ctx* c) {
    PhaseLaps lap("  upload");
    rta::PackedAccel pk;
    const bool packed = rta::pack_accel(c->accel, c->host_nodes.data(), c->N, c->cone_cull != 0, pk, &lap);
    // a refused pack (no accelerator: RT_OK without accel_ok) keeps what it had decided by then
    if (pk.boxes_finite >= 0) c->boxes_finite = pk.boxes_finite;
    if (pk.nfew >= 0) c->nfew = pk.nfew;
    if (pk.nfew >= 0 && pk.use_st) {
        int rc = alloc_and_copy(c, {host_array(c->titem_ref, pk.titem_ref.data(), pk.titem_ref.size())});
        if (rc != RT_OK) return rc;
        c->n_titems = static_cast<int>(pk.titem_ref.size());
        c->host_titem_ref = std::move(pk.titem_ref);
    }
    if (!packed) return RT_OK;
    const size_t P = c->accel.prim_shape.size();
    int rc = alloc_and_copy(c,
                            {host_array(c->anodes, pk.an.data(), pk.an.size()), host_array(c->lnodes, pk.ln.data(), pk.ln.size()),
                             host_array(c->wnodes, pk.wn.data(), pk.wn.size()), host_array(c->tleaf, pk.tl.data(), pk.tl.size()),
                             host_array(c->titems, pk.ti.data(), pk.ti.size()),
                             host_array(c->prims, static_cast<const float4*>(nullptr), 4 * (P ? P : 1)),
                             host_array(c->prim_idx_dev, pk.ps.data(), pk.ps.size())},
                            &lap);
    if (rc != RT_OK) return rc;
    if (P > 0)
        hipLaunchKernelGGL(k_pack_prims, dim3((P + 255) / 256), dim3(256), 0, c->stream, c->geo_lin, c->prim_idx_dev,
                           c->prim_idx_dev + P, static_cast<int>(P), c->prims);
    HIP_TRY(hipGetLastError());
    lap("copies issued");
    HIP_TRY(sync_stream(c));  // the packed arrays die with pk
    lap("copies + pack done");
    c->st_root = pk.st_root;
    c->accel_ok = true;
    c->record_bytes = (pk.an.size() + pk.ln.size() + pk.wn.size() + pk.tl.size() + pk.ti.size() + 4 * P +
                       2 * static_cast<size_t>(c->S)) * sizeof(float4);
    return RT_OK;
}

// Brings host_nodes up to the boxes rt_animate grew on the device.
int sync_host_nodes(rt_ctx* c) {
    if (!c->nodes_on_device_newer) return RT_OK;
    HIP_TRY(hipMemcpyAsync(c->host_nodes.data(), c->staging_nodes, c->N * sizeof(FlatNode), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(sync_stream(c));
    c->nodes_on_device_newer = false;
    return RT_OK;
}

// The scene tree's unbounded part (kNoPrune) has boxes padded from the reference
// leaves' exact boxes, which animation and rt_update_nodes change: once they may
// differ from the build's, those wide slots go infinite (entered by every ray; the
// items' exact boxes still gate). Idempotent; reset by every accelerator build.
int open_inf_slots(rt_ctx* c) {
    if (c->inf_open || !c->accel_ok) return RT_OK;
    c->inf_open = true;
    if (c->accel.st.wroot < 0) return RT_OK;
    const std::vector<int> slots = rta::noprune_slots(c->accel);
    hipFree(c->anim_inf_slots);
    c->anim_inf_slots = nullptr;
    c->n_inf_slots = static_cast<int>(slots.size());
    if (slots.empty()) return RT_OK;
    if (hipMalloc(&c->anim_inf_slots, slots.size() * sizeof(int)) != hipSuccess) return RT_ERR_NO_MEMORY;
    HIP_TRY(hipMemcpyAsync(c->anim_inf_slots, slots.data(), slots.size() * sizeof(int), hipMemcpyHostToDevice,
                           c->stream));
    hipLaunchKernelGGL(k_inf_slots, dim3((c->n_inf_slots + 255) / 256), dim3(256), 0, c->stream, c->anim_inf_slots,
                       c->n_inf_slots, c->lnodes, c->accel.mt ? kWideRecMt : kWideRec);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The device lists of the refit (AnimMaps) for the current scene, accelerator and
// refit set (refit_ids: the animated shapes and those rt_update_shapes rewrote).
// anim_base holds, per entry, the record the accelerator's bounds and cones were
// built from.
int prepare_animation(rt_ctx* c) {
    PhaseLaps lap("  prepare");
    const int n = static_cast<int>(c->refit_ids.size());
    c->anim = AnimMaps{};
    c->n_direct_slot_reads = 0;
    rta::RefitPlan pl;
    const rta::RefitState state{c->refit_of, c->anim_cls, c->entry_root};
    {
        rta::RefitSlots sl;  // the slot arrays die before the lists are built
        const int planned = rta::plan_refit_slots(c->accel, c->accel_ok, c->host_nodes.data(), c->N, c->host_idx.data(), c->S,
                                                  c->refit_ids, c->anim_base, c->host_shapes.data(),
                                                  rta::ShapeCache{c->accel.shape_cls, c->accel.shape_box, c->shape_moved}, state,
                                                  pl, sl, &lap);
        if (n == 0 || planned != RT_OK) return planned;
        if (pl.slots) {
            c->dirty_max = pl.dirty_max;
            c->dirty_sum = pl.dirty_sum;
            c->n_big = pl.n_big;
            hipFree(c->pbox);
            hipFree(c->refit_dirty);
            hipFree(c->refit_static);
            hipFree(c->refit_list);
            c->pbox = nullptr;
            c->refit_dirty = nullptr;
            c->refit_static = nullptr;
            c->refit_list = nullptr;
            c->n_dirty = 0;
            int rc = alloc_and_copy(c, {host_array(c->pbox, sl.pb.data(), sl.pb.size()),
                                        host_array(c->refit_dirty, sl.work.data(), sl.work.size()),
                                        host_array(c->refit_static, sl.st.data(), sl.st.size()),
                                        host_array(c->refit_list, sl.dl.data(), sl.dl.size())});
            if (rc != RT_OK) return rc;
            c->n_dirty = pl.n_dirty;
            c->n_direct_slot_reads = pl.n_direct_slot_reads;
            rc = open_inf_slots(c);
            if (rc != RT_OK) return rc;
        }
    }
    lap("slot uploads");
    static const std::vector<int> no_items;
    rta::plan_refit_lists(c->accel, c->accel_ok, c->host_nodes.data(), c->N, c->refit_ids,
                          c->accel_ok && c->titems ? c->host_titem_ref : no_items, state, pl);
    c->direct_reads = pl.direct_reads;
    lap("node lists");
    int rc = ensure_staging(c->anim_maps, c->anim_maps_cap, pl.buf.size());
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->anim_maps, pl.buf.data(), pl.buf.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(sync_stream(c));  // the plan's arrays die with pl
    lap("maps upload + sync");
    const int* d = c->anim_maps;
    const rta::RefitOffsets& o = pl.o;
    c->anim = AnimMaps{d + o.ids,       d + o.slot_off,  d + o.slot_list, d + o.prim_off, d + o.prim_list, d + o.wpos_off,
                       d + o.wpos_list, d + o.node_ids,  d + o.node_off,  d + o.node_list, d + o.wn_off,   d + o.wn_list,
                       d + o.item_off,  d + o.item_list, d + o.ecls,      d + o.prim_entry, n,              pl.n_nodes};
    return ensure_staging(c->anim_sbox, c->anim_sbox_cap, 4 * static_cast<size_t>(n));
}

// The root's box from the host's node records (rt_upload_scene, rt_update_nodes).
void set_root(rt_ctx* c) {
    if (c->N <= 0 || static_cast<int>(c->host_nodes.size()) != c->N) return;
    const FlatNode& r = c->host_nodes[c->N - 1];
    const float lo[3] = {r.boundsMin.x, r.boundsMin.y, r.boundsMin.z}, hi[3] = {r.boundsMax.x, r.boundsMax.y, r.boundsMax.z};
    std::memcpy(c->root_lo, lo, sizeof lo);
    std::memcpy(c->root_hi, hi, sizeof hi);
}

// (Re)builds the accelerator after the host copies changed, then the animation lists.
int upload_accel(rt_ctx* c, const bool* built = nullptr) {
    discard_rebuild(c);
    c->st_suspended = false;
    int rc = sync_host_nodes(c);
    if (rc != RT_OK) return rc;
    rc = build_upload_accel(c, built);
    c->shape_moved.assign(c->S, 0);  // built from the current host records
    // the degraded-bound reports of earlier refits concern the accelerator this replaced
    // (prepare_animation alone, when the refit set changes, keeps them: same accelerator)
    for (bool& pend : c->report_pending) pend = false;
    // the refit set stays (its shapes tend to move again), with the records just built from
    c->anim_base.resize(c->refit_ids.size());
    for (size_t i = 0; i < c->refit_ids.size(); ++i) c->anim_base[i] = c->host_shapes[c->refit_ids[i]];
    c->nodes_rebuild = c->bounds_rebuild = false;
    const int rc2 = prepare_animation(c);
    return rc != RT_OK ? rc : rc2;
}

// Whether every reachable inner node's children lie inside its box (accel.cpp
// boxes_nest), the condition the scene tree was built on.
bool host_nodes_nest(const rt_ctx* c) {
    const int N = c->N;
    if (N <= 0) return true;
    auto in = [](const FlatNode& p, const FlatNode& q) {
        const float* plo = &p.boundsMin.x;
        const float* phi = &p.boundsMax.x;
        const float* qlo = &q.boundsMin.x;
        const float* qhi = &q.boundsMax.x;
        for (int a = 0; a < 3; ++a)
            if (!(plo[a] <= qlo[a] && qlo[a] <= phi[a] && plo[a] <= qhi[a] && qhi[a] <= phi[a])) return false;
        return true;
    };
    std::vector<char> seen(N, 0);
    std::vector<int> st{N - 1};
    while (!st.empty()) {
        const int k = st.back();
        st.pop_back();
        if (seen[k]) continue;
        seen[k] = 1;
        const FlatNode& nd = c->host_nodes[k];
        if (nd.leftChild == -1) continue;
        if (!in(nd, c->host_nodes[nd.leftChild]) || !in(nd, c->host_nodes[nd.rightChild])) return false;
        st.push_back(nd.leftChild);
        st.push_back(nd.rightChild);
    }
    return true;
}

// Asynchronous rebuild (rt_ctx::AsyncBuild). A running build is joined and dropped
// by anything that replaces the scene or rebuilds synchronously.
void discard_rebuild(rt_ctx* c) {
    if (!c->rebuild) return;
    if (c->rebuild->th.joinable()) c->rebuild->th.join();
    c->rebuild.reset();
}

// Starts the rebuild over a snapshot of the host records (device-grown node boxes
// fetched first). A rebuild already running is left to finish: the refit that lands it
// checks the kinds of bound and the nesting again.
int start_rebuild(rt_ctx* c) {
    if (c->rebuild) return RT_OK;
    ++c->anim_rebuilds;
    const int rc = sync_host_nodes(c);
    if (rc != RT_OK) return rc;
    if (c->nodes_rebuild) c->st_suspended = true;  // exact meanwhile: the reference tree only
    c->nodes_rebuild = false;
    std::unique_ptr<rt_ctx::AsyncBuild> b = c->spare ? std::move(c->spare) : std::make_unique<rt_ctx::AsyncBuild>();
    b->done.store(false);
    b->ok = false;
    b->shapes.assign(c->host_shapes.begin(), c->host_shapes.end());  // into the spare's capacity
    b->nodes.assign(c->host_nodes.begin(), c->host_nodes.end());
    rt_ctx::AsyncBuild* raw = b.get();
    const std::vector<int>* idx = &c->host_idx;  // fixed while the build runs: an upload joins it first
    const int S = c->S, N = c->N, I = c->I;
    const bool mt = c->build_mt;
    raw->th = std::thread([raw, idx, S, N, I, mt] {
        try {  // (bad_alloc: swapped in as a failed build, no accelerator; never past the thread)
            raw->ok = rta::build_accel(raw->shapes.data(), S, raw->nodes.data(), N, idx->data(), I, kLeafScan,
                                       kMaxStack, raw->A, mt);
        } catch (...) {
            raw->A = rta::AccelHost();
            raw->ok = false;
        }
        raw->done.store(true, std::memory_order_release);
    });
    c->rebuild = std::move(b);
    return RT_OK;
}

// Swaps a finished rebuild in: its accelerator to the device (the frames in flight end
// first), then every shape whose record differs from the snapshot, and the animated
// ones, form the refit set with their snapshot records as the build-time base, so the
// next refit brings the new accelerator to the current records (the caller's flush).
int finish_rebuild(rt_ctx* c, bool* refit) {
    if (!c->rebuild || !c->rebuild->done.load(std::memory_order_acquire)) return RT_OK;
    PhaseLaps lap("finish_rebuild");
    std::unique_ptr<rt_ctx::AsyncBuild> b = std::move(c->rebuild);
    b->th.join();
    lap("join");
    int rc = sync_host_nodes(c);
    if (rc != RT_OK) return rc;
    HIP_TRY(sync_stream(c));
    lap("sync");
    free_accel(c);
    c->st_suspended = false;
    for (bool& pend : c->report_pending) pend = false;  // reports about the accelerator replaced
    ++c->async_swaps;
    // the replaced accelerator's host arrays go to b->A, freed by the next build's thread
    std::swap(c->accel, b->A);
    if (!b->ok) {  // as a failed synchronous build: no accelerator (k_packet)
        c->accel = rta::AccelHost();
        c->refit_ids.clear();
        c->anim_base.clear();
        c->spare = std::move(b);
        return prepare_animation(c);
    }
    lap("free");
    if ((rc = upload_built_accel(c)) != RT_OK) return rc;
    lap("upload");
    std::vector<char> in(c->S, 0);
    std::vector<int> ids;
    std::vector<FlatShape> base;
    auto add = [&](int id) {
        if (in[id]) return;
        in[id] = 1;
        ids.push_back(id);
        base.push_back(b->shapes[id]);
    };
    for (int id : c->anim_ids) add(id);
    c->shape_moved.assign(c->S, 0);
    for (int id = 0; id < c->S; ++id)
        if (std::memcmp(&c->host_shapes[id], &b->shapes[id], sizeof(FlatShape)) != 0) {
            add(id);
            c->shape_moved[id] = 1;
        }
    c->refit_ids.swap(ids);
    c->anim_base.swap(base);
    // pending writes stay pending (upd_ids): their shapes are in the set with the snapshot base
    for (auto& ub : c->upd_base) ub.second = b->shapes[ub.first];
    // the node records since the snapshot are in every copy already (upload_built_accel read
    // host_nodes; pending ones stay nodes_dirty); boxes that do not nest (any more) rebuild
    // again, exact meanwhile
    c->nodes_rebuild = c->accel_ok && c->accel.st.wroot >= 0 && !host_nodes_nest(c);
    *refit = !c->refit_ids.empty();
    lap("refit set");
    rc = prepare_animation(c);
    lap("prepare_animation");
    c->spare = std::move(b);  // reused by the next rebuild (not freed here)
    return rc;
}

// Reads the report words of earlier refits whose k_refit has run (block: wait for
// them): a shape whose bound changed kind leaves the accelerator exact but slower
// (k_refit enters every box above it) until the host rebuilds it.
// Every refit slot is free once the stream has drained: no event needed.
void stream_drained(rt_ctx* c) {
    c->mark_slot = -1;
    for (bool& b : c->slot_busy) b = false;
}

// hipStreamSynchronize of the context's stream, which also retires its refit slots
// (and its sub-contexts', which run on the same stream).
hipError_t sync_stream(rt_ctx* c) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess)
        for (rt_ctx* x : {c, c->brute, c->mtc})
            if (x) stream_drained(x);
    return e;
}

// Records the anim_copied event of the last k_refit's slot if it is still pending.
int record_mark(rt_ctx* c) {
    if (c->mark_slot < 0) return RT_OK;
    const int s = c->mark_slot;
    c->mark_slot = -1;
    HIP_TRY(hipEventRecord(c->anim_copied[s], c->stream));
    return RT_OK;
}

int check_reports(rt_ctx* c, bool block = false) {
    for (int s = 0; s < rt_ctx::kAnimRing; ++s) {
        if (!c->report_pending[s]) continue;
        if (s == c->mark_slot) {  // its event is not recorded yet: not done unless waited for
            if (!block) continue;
            if (const int rc = record_mark(c)) return rc;
        }
        if (block) {
            HIP_TRY(hipEventSynchronize(c->anim_copied[s]));
        } else {
            const hipError_t e = hipEventQuery(c->anim_copied[s]);
            if (e == hipErrorNotReady) continue;
            if (e != hipSuccess) return RT_ERR_DEVICE;
        }
        c->report_pending[s] = false;
        const int* rep = reinterpret_cast<const int*>(static_cast<const char*>(c->anim_pinned[s]) + c->report_at[s]);
        if (*rep) c->bounds_rebuild = true;
    }
    return RT_OK;
}

// A slot of the pinned ring k_refit reads from, `bytes` large plus its report word;
// waits for that slot's previous k_refit (kAnimRing flushes back).
int pinned_slot(rt_ctx* c, size_t bytes, char** host, const char** dev) {
    const int slot = c->anim_slot;
    c->anim_slot = (slot + 1) % rt_ctx::kAnimRing;
    if (!c->anim_copied[slot]) {
        HIP_TRY(hipEventCreateWithFlags(&c->anim_copied[slot], hipEventDisableTiming));
    } else if (c->slot_busy[slot]) {
        if (slot == c->mark_slot && record_mark(c) != RT_OK) return RT_ERR_DEVICE;
        HIP_TRY(hipEventSynchronize(c->anim_copied[slot]));  // this slot's last k_refit has run
        c->slot_busy[slot] = false;
        if (const int rc = check_reports(c)) return rc;
    }
    bytes = (bytes + 15) / 16 * 16;
    if (c->anim_pinned_cap[slot] < bytes + 16) {
        if (c->anim_pinned[slot]) hipHostFree(c->anim_pinned[slot]);
        c->anim_pinned[slot] = nullptr;
        c->anim_pinned_dev[slot] = nullptr;
        c->anim_pinned_cap[slot] = 0;
        // mapped and coherent: the kernel reads it over the host link, never a stale cached copy
        if (hipHostMalloc(&c->anim_pinned[slot], bytes + 16, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            return RT_ERR_NO_MEMORY;
        if (hipHostGetDevicePointer(&c->anim_pinned_dev[slot], c->anim_pinned[slot], 0) != hipSuccess)
            return RT_ERR_DEVICE;
        c->anim_pinned_cap[slot] = bytes + 16;
    }
    c->report_at[slot] = bytes;
    *host = static_cast<char*>(c->anim_pinned[slot]);
    *dev = static_cast<const char*>(c->anim_pinned_dev[slot]);
    *reinterpret_cast<int*>(*host + bytes) = 0;
    return slot;
}

// The refit set only grows while shapes join it (rt_update_shapes of a shape not in
// it), and every flush copies and refits all of it. A host that writes a different
// few shapes each frame would make that every shape it ever touched. So once the
// entries that are neither animated nor written since the last flush ("stale")
// outnumber kRefitSlack, S / 16 and the live ones, they leave the set: their device
// records are current (the last flush that listed them wrote them), and
// prepare_animation folds their current boxes into the slots' fixed parts, which it
// recomputes from the host records. An entry whose bound changed kind since the build
// stays (the fixed part has no box for it; its report rebuilds the accelerator).
// Per-flush entries stay below about 2 x live + max(kRefitSlack, S / 16).
constexpr size_t kRefitSlack = 4096;
void compact_refit_set(rt_ctx* c) {
    const size_t n = c->refit_ids.size(), live = c->anim_ids.size() + c->upd_ids.size();
    if (n <= live || n - live <= std::max({kRefitSlack, static_cast<size_t>(c->S) / 16, live})) return;
    std::vector<char> keep_shape(c->S, 0);
    for (int id : c->anim_ids) keep_shape[id] = 1;
    for (int id : c->upd_ids) keep_shape[id] = 1;
    std::vector<int> ids;
    std::vector<FlatShape> base;
    for (size_t i = 0; i < n; ++i) {
        const int id = c->refit_ids[i];
        bool keep = keep_shape[id] != 0;
        if (!keep && i < c->anim_cls.size()) {
            rta::Box3 b;
            keep = rta::classify(c->host_shapes[id], b, c->accel.origin_lim, c->accel.mt) != c->anim_cls[i];
        }
        if (keep) {
            ids.push_back(id);
            base.push_back(c->anim_base[i]);
        }
    }
    c->refit_ids.swap(ids);
    c->anim_base.swap(base);
    ++c->refit_compactions;
}

// Applies what rt_update_shapes / rt_update_nodes left on the host, and an
// rt_animate frame (grow: the animated entries grow the nodes listing them, as
// updateBVH does), to every device copy with one launch of k_refit on the stream:
// every refit entry's records (read from the pinned ring), the nodes listing an
// entry (their content boxes; with grow their exact boxes), the local and
// scene-tree boxes above its prims, and the host's node records (rt_update_nodes).
// The host does no per-shape work beyond copying the records: whether a bound
// changed kind is decided by k_refit, which keeps such a frame exact and reports it.
// The host rebuilds the accelerator (for speed) once a report comes in, and (for
// exactness of the scene tree) when new node boxes stop nesting. Called by every
// operation that reads the device scene.
int flush_updates(rt_ctx* c, bool grow = false) {
    if (!c->have_scene) return RT_OK;
    bool swapped = false;  // a rebuilt accelerator landed: its refit set is refit now
    int rc = finish_rebuild(c, &swapped);
    if (rc != RT_OK) return rc;
    PhaseLaps lap(swapped ? "flush after swap" : nullptr);
    rc = check_reports(c);
    if (rc != RT_OK) return rc;
    lap("check_reports");
    const bool gbox = c->grow_pending && !c->anim_ids.empty();
    const bool work = !c->upd_ids.empty() || c->nodes_dirty || grow || gbox || swapped;
    if (!work && !c->bounds_rebuild) return RT_OK;
    if (work) {
        // shapes new to the refit set join it with their build-time records
        bool added = false;
        for (const auto& ub : c->upd_base)
            if (c->refit_of[ub.first] < 0) {
                c->refit_of[ub.first] = static_cast<int>(c->refit_ids.size());
                c->refit_ids.push_back(ub.first);
                c->anim_base.push_back(ub.second);
                added = true;
            }
        if (added) compact_refit_set(c);
        if (added && (rc = prepare_animation(c)) != RT_OK) return rc;
        lap("refit set joined");
        const int n = static_cast<int>(c->refit_ids.size());
        const bool nodes = c->nodes_dirty && c->N > 0;
        const size_t rec_bytes = static_cast<size_t>(n) * (sizeof(FlatShape) + sizeof(int));
        const size_t node_bytes = nodes ? static_cast<size_t>(c->N) * sizeof(FlatNode) : 0;
        const size_t box_at = (rec_bytes + node_bytes + 15) / 16 * 16;  // growth boxes (AF_BOX), 2 float4 per entry
        const size_t bytes = gbox ? box_at + static_cast<size_t>(n) * 2 * sizeof(float4) : rec_bytes + node_bytes;
        c->last_flush_bytes = static_cast<long long>(bytes);
        if (bytes > 0) {
            char* pin = nullptr;
            const char* pin_dev = nullptr;
            const int slot = pinned_slot(c, bytes, &pin, &pin_dev);
            if (slot < 0) return slot;
            lap("pinned slot");
            for (int i = 0; i < n; ++i)
                std::memcpy(pin + i * sizeof(FlatShape), &c->host_shapes[c->refit_ids[i]], sizeof(FlatShape));
            int* flags = reinterpret_cast<int*>(pin + n * sizeof(FlatShape));
            std::memset(flags, 0, n * sizeof(int));
            if (grow)
                for (int id : c->anim_ids) flags[c->refit_of[id]] = AF_GROW;
            if (gbox) {
                float4* gb = reinterpret_cast<float4*>(pin + box_at);
                for (size_t k = 0; k < c->anim_ids.size(); ++k) {
                    const int e = c->refit_of[c->anim_ids[k]];
                    const float* b = &c->grow_box[6 * k];
                    flags[e] = AF_GROW | AF_BOX;
                    gb[2 * e] = make_float4(b[0], b[1], b[2], 0.f);
                    gb[2 * e + 1] = make_float4(b[3], b[4], b[5], 0.f);
                }
            }
            if (nodes) std::memcpy(pin + rec_bytes, c->host_nodes.data(), c->N * sizeof(FlatNode));
            const bool acc = c->accel_ok;
            const size_t P = c->accel.prim_shape.size();
            const AnimOut out{c->staging_shapes, c->staging_nodes, c->geo_lin, c->geo_leaf, c->mat, c->nodes,
                              acc ? c->anodes : nullptr, acc ? c->lnodes : nullptr, acc ? c->prims : nullptr,
                              acc ? c->wnodes : nullptr, acc ? c->titems : nullptr,
                              acc ? c->pbox : nullptr, acc ? c->prim_idx_dev + P : nullptr, c->anim_sbox,
                              c->accel.origin_lim, c->accel.mt ? 1 : 0,
                              {c->accel.mt_z[0], c->accel.mt_z[1], c->accel.mt_z[2]},
                              acc ? c->prim_idx_dev : nullptr, c->cone_cull};
            const int mode = c->refit_mode >= 0 ? c->refit_mode : c->direct_reads <= kDirectReads ? 2 : 1;
            RefitArgs r{};
            r.fresh = reinterpret_cast<const FlatShape*>(pin_dev);
            r.flags = reinterpret_cast<const int*>(pin_dev + n * sizeof(FlatShape));
            r.gbox = gbox ? reinterpret_cast<const float4*>(pin_dev + box_at) : nullptr;
            r.nsrc = nodes ? reinterpret_cast<const FlatNode*>(pin_dev + rec_bytes) : nullptr;
            r.report = reinterpret_cast<int*>(const_cast<char*>(pin_dev) + c->report_at[slot]);
            r.na = (n + 63) / 64;  // the record and node-set roles always run in one-wave workgroups
            r.N = c->N;
            r.n_items = nodes && acc ? c->n_titems : 0;
            r.titem_ref = c->titem_ref;
            r.nd = nodes ? (c->N + r.n_items + 63) / 64 : 0;
            r.nb = n > 0 ? c->anim.nodes : 0;
            r.dirty = c->refit_dirty;
            r.n_big = c->n_big;
            r.dstatic = c->refit_static;
            r.dlist = c->refit_list;
            r.n_dirty = n > 0 && acc ? c->n_dirty : 0;
            r.rec = c->accel.mt ? kWideRecMt : kWideRec;
            r.direct = mode == 2;
            // waves per workgroup: the node and slot roles' own launch takes kRefitWaves (a
            // slot's or node's list in one step), a launch with the one-wave roles one
            auto go = [&](const RefitArgs& ra, int waves) -> int {
                const int small = std::max(0, ra.n_dirty - ra.n_big);
                const int grid = ra.na + ra.nd + ra.nb + std::min(ra.n_big, ra.n_dirty) + (small + waves - 1) / waves;
                if (grid == 0) return RT_OK;
                hipLaunchKernelGGL(k_refit, dim3(grid), dim3(64 * waves), 0, c->stream, c->anim, out, ra);
                HIP_TRY(hipGetLastError());
                return RT_OK;
            };
            if (mode == 1) {  // records and node sets, then (a kernel boundary later) the boxes
                RefitArgs r1 = r, r2 = r;
                r1.nb = r1.n_dirty = 0;
                r2.na = r2.nd = 0;
                if ((rc = go(r1, 1)) != RT_OK || (rc = go(r2, kRefitWaves)) != RT_OK) return rc;
            } else if ((rc = go(r, 1)) != RT_OK) {
                return rc;
            }
            lap("records staged, k_refit launched");
            // the slot may be refilled once its event (recorded behind the next dispatch) is done
            if ((rc = record_mark(c)) != RT_OK) return rc;
            c->mark_slot = slot;
            c->slot_busy[slot] = true;
            ++c->refit_launches;  // rt_sync_frame: a slot taken since the frame's dispatch
            c->report_pending[slot] = n > 0 && acc;
            if (nodes && (rc = open_inf_slots(c)) != RT_OK) return rc;
        }
        if (grow || gbox) c->nodes_on_device_newer = true;  // the device grew the nodes past host_nodes
        if (gbox) {
            c->grow_pending = false;
            for (size_t k = 0; k < c->anim_ids.size(); ++k)
                for (int a = 0; a < 3; ++a) {
                    c->grow_box[6 * k + a] = INFINITY;
                    c->grow_box[6 * k + 3 + a] = -INFINITY;
                }
        }
        c->nodes_dirty = false;
        for (int id : c->upd_ids) c->upd_mark[id] = 0;
        c->upd_ids.clear();
        c->upd_base.clear();
        lap("flush end");
    }
    if (!c->nodes_rebuild && !c->bounds_rebuild) {
        ++c->updates_flushed;
        return RT_OK;
    }
    // a bound changed kind (reported by an earlier k_refit), or the node boxes stopped
    // nesting: rebuild from the host copies (which the refit above brought to the device),
    // on a host thread while the frames go on (rt_ctx::AsyncBuild), or here
    c->bounds_rebuild = false;
    if (c->async_rebuild) return start_rebuild(c);
    ++c->anim_rebuilds;
    return upload_accel(c);
}

size_t sched_set_words(int tiles) {
    return static_cast<size_t>((tiles + kOrderThreads - 1) / kOrderThreads) * kOrderBuckets;
}

// The camera terms of getRay (primary_ray).
void fill_camera(const FlatCamera& cam, KParams& kp) {
    kp.cam_pos = V{cam.Position.x, cam.Position.y, cam.Position.z};
    kp.cam_front = V{cam.Front.x, cam.Front.y, cam.Front.z};
    kp.cam_right = V{cam.Right.x, cam.Right.y, cam.Right.z};
    kp.cam_up = V{cam.Up.x, cam.Up.y, cam.Up.z};
    // gpu_shader.comp:156-157 (radians = deg * 0.0174532925..., glm/GLSL).
    const float h = 2.0f * std::tan((cam.fov / 2.0f) * 0.01745329251994329576923690768489f);
    kp.plane_h = h;
    kp.plane_w = h * cam.aspectRatio;
}

// The camera of `c` and its resolution, for the launches that form camera rays of the frame as set.
void camera_params(const rt_ctx* c, KParams& kp) {
    fill_camera(c->cam, kp);
    kp.resX = c->params.resX;
    kp.resY = c->params.resY;
}

// Per-lane LDS stack entries of the walks over t's accelerator (rt_debug_lane_stack overrides).
int lane_stack_entries(const rt_ctx* t) {
    return t->lane_stack_override > 0 ? t->lane_stack_override : t->accel.max_stack;
}

// The device scene of `t` and its stack depths: what every kernel's walks read.
void scene_params(const rt_ctx* t, KParams& kp) {
    kp.geo_leaf = t->geo_leaf;
    kp.geo_lin = t->geo_lin;
    kp.nodes = t->nodes;
    kp.S = t->S;
    kp.N = t->N;
    kp.I = t->I;
    kp.max_stack = t->max_stack < 1 ? 1 : t->max_stack;
    kp.lane_stack = lane_stack_entries(t);
}

// Dynamic LDS: a wave's per-lane stacks over the accelerator (codes, then bf16 entry
// parameters: 6 B an entry), and a block's stacks of the literal reference walk.
size_t lane_stack_lds(const KParams& kp) { return static_cast<size_t>(kp.lane_stack) * 64 * 6; }
size_t ref_stack_lds(const KParams& kp) { return static_cast<size_t>(kp.max_stack) * kBlock * sizeof(int); }

// The root's current bounds for the tile kernels' sky skip:
// the root's bounds as kernel arguments while the host copy is current; once
// rt_animate grew the boxes on the device, from the accelerator's copy of the
// root record (which the refit keeps current)
void root_bounds(const rt_ctx* t, KParams& kp) {
    kp.root_ok = 0;
    if (kp.N > 0 && t->nodes_on_device_newer) kp.root_ok = 2;
    if (kp.N > 0 && !t->nodes_on_device_newer && static_cast<int>(t->host_nodes.size()) == kp.N) {
        const FlatNode& rn = t->host_nodes[kp.N - 1];
        kp.root_ok = 1;
        kp.root_lo[0] = rn.boundsMin.x;
        kp.root_lo[1] = rn.boundsMin.y;
        kp.root_lo[2] = rn.boundsMin.z;
        kp.root_hi[0] = rn.boundsMax.x;
        kp.root_hi[1] = rn.boundsMax.y;
        kp.root_hi[2] = rn.boundsMax.z;
    }
}

// Bytes per pixel of an rt_format (0: not a format) and the alignment of its dst and pitch:
// a pixel is one store of 16 B (RGBA32F), three of 4 B (RGB32F), one of 4 B (the 8-bit
// formats) or one of 8 B (RGBA16F).
size_t format_bytes(int format) {
    switch (format) {
        case RT_FORMAT_RGBA32F:
        case RT_FORMAT_RGBA32F_IMAGE: return 16;
        case RT_FORMAT_RGB32F: return 12;
        case RT_FORMAT_RGBA8:
        case RT_FORMAT_SRGBA8: return 4;
        case RT_FORMAT_RGBA16F: return 8;
        default: return 0;
    }
}
size_t format_align(int format) {
    const size_t px = format_bytes(format);
    return px == 12 || px == 0 ? 4 : px;
}

// ss > 1 (rt_set_samples): width .. out_rows are the SAMPLE frame's, ss times the output
// frame's that dst, pitch and format describe (KParams::ss); resX, resY are scaled to match.
int fill_kparams(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows, float* dst,
                 size_t pitch, KParams& kp, int format = RT_FORMAT_RGBA32F, int ss = 1) {
    if (!c->have_scene || !c->have_cam || !c->have_light) return RT_ERR_NO_SCENE;
    const size_t px = format_bytes(format), align = format_align(format);
    if (width <= 0 || height <= 0 || stripe <= 0 || period < stripe || out_rows < 0 || y0 < 0 || !dst ||
        px == 0 || ss < 1 || pitch < static_cast<size_t>(width / ss) * px ||
        (pitch % align) != 0 || (reinterpret_cast<uintptr_t>(dst) % align) != 0)
        return RT_ERR_INVALID;
    std::memset(&kp, 0, sizeof kp);
    scene_params(c, kp);
    kp.mat = c->mat;
    fill_camera(c->cam, kp);
    kp.light_pos = V{c->light.position.x, c->light.position.y, c->light.position.z};
    kp.light_color = V{c->light.color.x, c->light.color.y, c->light.color.z};
    kp.resX = c->params.resX * static_cast<float>(ss);  // a power of two: exact
    kp.resY = c->params.resY * static_cast<float>(ss);
    kp.ss = ss;
    kp.maxBounces = c->params.maxBounces;
    kp.useBVH = c->params.useBVH;
    kp.useFresnel = c->params.useFresnel;
    kp.useMT = c->params.useMollerTrumbore;
    kp.width = width;
    kp.height = height;
    kp.y0 = y0;
    kp.stripe = stripe;
    kp.period = period;
    kp.out_rows = out_rows;
    kp.dst = reinterpret_cast<char*>(dst);
    kp.pitch = pitch;
    kp.shadow_off = 1e-3f;
    kp.rgb = format;  // RT_FORMAT_*: 0 RGBA32F, 1 RGB32F, 2 RGBA32F at the image row, 3-5 display formats
    kp.heavy_k = 0;
    kp.heavy_parts = 1;
    kp.lane_k = 0;
    kp.lane_k_mode = 0;
    kp.cost_time = 0;
    return RT_OK;
}

bool accel_usable(const rt_ctx* c, const KParams& kp) {
    const float cmag = std::max({std::fabs(kp.cam_pos.x), std::fabs(kp.cam_pos.y), std::fabs(kp.cam_pos.z)});
    return c->accel_ok && kp.useBVH && (kp.useMT != 0) == c->accel.mt && cmag <= c->accel.origin_lim;
}

// The accelerator's device records as the walks take them.
AccelPtrs accel_ptrs(const rt_ctx* c) {
    // Animated scenes keep the scene tree: rt_animate refits its boxes and items (prepare_animation).
    // (off while a rebuild for node boxes that stopped nesting runs: st_suspended)
    const int troot = c->tree_mode == RT_TREE_SCENE && !c->st_suspended ? c->st_root : kNoChild;
    return AccelPtrs{c->anodes, c->prims, c->lnodes, c->wnodes, c->tleaf, c->titems, troot,
                     c->scene_stack > 0 ? c->scene_stack : kMaxStack, c->nfew, c->N, c->accel.origin_lim,
                     c->boxes_finite, c->split_max, c->split_g, c->prim_idx_dev,
                     {c->accel.mt_z[0], c->accel.mt_z[1], c->accel.mt_z[2]}};
}

int launch(rt_ctx* c, const KParams& kp, bool stats);

// A sub-context on this context's stream (brute / mtc), created on first use.
rt_ctx* sub_ctx(rt_ctx* c, rt_ctx*& sub, bool& stale) {
    if (!sub) {
        if (rtx::create_ctx(&sub, c->device, c->stream) != RT_OK) return nullptr;
        stale = true;
    }
    return sub;
}

// The frame constants and walk settings of `c`, for a sub-context rendering its frame.
void inherit(rt_ctx* b, const rt_ctx* c) {
    b->cam = c->cam;
    b->light = c->light;
    std::copy(c->lights, c->lights + RT_MAX_LIGHTS, b->lights);
    b->nlights = c->nlights;
    std::copy(c->soft_radii, c->soft_radii + RT_MAX_LIGHTS, b->soft_radii);
    b->soft_count = c->soft_count;
    b->soft_samples = c->soft_samples;
    b->soft_form = c->soft_form;
    b->have_cam = b->have_light = true;
    b->params = c->params;
    b->kernel = RT_KERNEL_ACCEL;
    b->lane_from_depth = c->lane_from_depth;
    b->cone_cull = c->cone_cull;
    b->split_max = c->split_max;
    b->split_g = c->split_g;
    b->heavy_k = c->heavy_k;
    b->heavy_parts = c->heavy_parts;
    b->lane_k = c->lane_k;
    b->lane_k_mode = c->lane_k_mode;
    b->cost_time = c->cost_time;
    b->latency_mode = c->latency_mode;
    b->schedule = c->schedule;
    b->sched_period = c->sched_period;
    b->cost_dilate = c->cost_dilate;
    b->moving_period = c->moving_period;
    b->moving_dilate = c->moving_dilate;
    b->moving_split = c->moving_split;
    b->frame_event = c->frame_event;
    b->refit_mode = c->refit_mode;
    b->async_rebuild = c->async_rebuild;
    b->tail_from = c->tail_from;
    b->tail_max_lanes = c->tail_max_lanes;
    b->shadow_walk_override = c->shadow_walk_override;
    b->tree_mode = c->tree_mode;
    b->scene_stack = c->scene_stack;
    b->lane_stack_override = c->lane_stack_override;
    b->ss_general = c->ss_general;
    b->adaptive = c->adaptive;
    b->convert_pass = c->convert_pass;
}

// The walk policy in force (rt_set_walk, or auto): barycentric frames walk camera
// rays and their shadows as packets and reflections per lane (1, measured fastest on
// configs 2, 3 and 5). Moller-Trumbore frames over a shallow reference tree with
// big leaves (the car's 3 nodes, whose local BVHs carry the grazing cones) walk every
// bounce as packets, since the cones force entries that neighbouring rays share: car
// MT frame 8.99 ms at 1, 7.73 at 2, 7.00 at 3 (= all packets at depth 3), 12.2 per
// lane for every bounce. Over a deep tree of small leaves (config 5: 6.86 ms at 1,
// 11.39 all packets) they keep 1; the monkey is equal either way
// (profiles/r02zz5_abf_mt_walk*.jsonl).
int walk_from(const rt_ctx* c) {
    if (c->lane_from_depth >= 0) return c->lane_from_depth;
    return c->accel.mt && c->N < kMtPacketMaxNodes ? kMtWalkFrom : 1;
}

bool sub_usable(const rt_ctx* b, const KParams& kp) {
    const float cmag = std::max({std::fabs(kp.cam_pos.x), std::fabs(kp.cam_pos.y), std::fabs(kp.cam_pos.z)});
    return b->accel_ok && cmag <= b->accel.origin_lim;
}

// The brute branch through `brute` (rt_ctx::brute): the same shapes under one
// leaf listing 0..S-1 with an infinite box, built on first use after the
// shapes change. nullptr: render the branch literally (k_packet).
rt_ctx* brute_ctx(rt_ctx* c, const KParams& kp) {
    if (!c->brute_accel || kp.useBVH || c->S <= 0 ||
        (c->kernel != RT_KERNEL_AUTO && c->kernel != RT_KERNEL_ACCEL))
        return nullptr;
    rt_ctx* b = sub_ctx(c, c->brute, c->brute_stale);
    if (!b) return nullptr;
    if (c->brute_stale) {
        FlatNode leaf;
        std::memset(&leaf, 0, sizeof leaf);
        const float inf = std::numeric_limits<float>::infinity();
        leaf.boundsMin = rt_vec3{-inf, -inf, -inf};
        leaf.boundsMax = rt_vec3{inf, inf, inf};
        leaf.leftChild = leaf.rightChild = -1;
        leaf.startShapeIdx = 0;
        leaf.numShapes = c->S;
        std::vector<int> order(c->S);
        for (int i = 0; i < c->S; ++i) order[i] = i;
        if (rt_upload_scene(b, c->host_shapes.data(), c->S, &leaf, 1, order.data(), c->S) != RT_OK) return nullptr;
        c->brute_stale = false;
    }
    inherit(b, c);
    b->params.useBVH = 1;
    return b;  // its own MT forwarding (mt_ctx) applies on the next hop
}

// Moller-Trumbore frames through `mtc` (rt_ctx::mtc): the same shapes and tree,
// the accelerator built for the MT test.
rt_ctx* mt_ctx(rt_ctx* c, const KParams& kp) {
    if (!kp.useBVH || !kp.useMT || c->build_mt || c->S <= 0 || c->N <= 0 ||
        (c->kernel != RT_KERNEL_AUTO && c->kernel != RT_KERNEL_ACCEL))
        return nullptr;
    rt_ctx* b = sub_ctx(c, c->mtc, c->mtc_stale);
    if (!b) return nullptr;
    if (c->mtc_stale) {
        b->build_mt = true;
        if (sync_host_nodes(c) != RT_OK ||
            rt_upload_scene(b, c->host_shapes.data(), c->S, c->host_nodes.data(), c->N, c->host_idx.data(),
                            c->I) != RT_OK ||
            (!c->anim_ids.empty() &&  // rt_animate frames forward to it from now on
             rt_set_animated(b, c->anim_ids.data(), static_cast<int>(c->anim_ids.size())) != RT_OK))
            return nullptr;
        c->mtc_stale = false;
    }
    inherit(b, c);
    return b;
}

// rt_dispatch_rows' render: through `brute` (useBVH = 0) and / or `mtc`
// (Moller-Trumbore) when they apply and their accelerator can take the frame,
// timed by this context's events (rt_kernel_times) like any other dispatch.
unsigned long long refit_launches(const rt_ctx* c, int depth = 0) {
    if (!c) return 0;
    unsigned long long n = c->refit_launches;
    if (depth < 2) n += refit_launches(c->brute, depth + 1) + refit_launches(c->mtc, depth + 1);
    return n;
}

int render_frame(rt_ctx* c, const KParams& kp, rt_ctx** from);

// rt_dispatch_rows' render (render_frame), remembering for rt_sync_frame which context's
// launch drew it and the refit launches so far
int render(rt_ctx* c, const KParams& kp) {
    rt_ctx* from = nullptr;
    const int rc = render_frame(c, kp, &from);
    c->frame_from = rc == RT_OK ? from : nullptr;
    c->frame_refits = refit_launches(c);
    return rc;
}

// One hop of a frame or a ray list from `t` towards the context that renders it: the brute
// sub-context (which sets the shader's shadow offset for useBVH = 0 in `off`), else the
// Moller-Trumbore one, else nullptr. `sel`: the useBVH / useMT in force at `t`.
rt_ctx* next_hop(rt_ctx* t, const KParams& sel, float& off) {
    rt_ctx* nxt = brute_ctx(t, sel);
    if (nxt) off = 1e-5f;  // gpu_shader.comp:565
    else nxt = mt_ctx(t, sel);
    return nxt;
}

// rt_set_kernel_timing: the event pair around one dispatch, from the ring while it has room
// (rt_kernel_times), else the context's overflow pair (rt_last_kernel_ms alone).
struct TimedSpan {
    hipEvent_t e0, e1;
    bool ended;  // e1 is recorded (mark_end)
};

int begin_timed(rt_ctx* c, TimedSpan& s) {
    s = TimedSpan{c->ev0, c->ev1, false};
    if (c->ring_used < static_cast<int>(c->ring0.size())) {
        s.e0 = c->ring0[c->ring_used];
        s.e1 = c->ring1[c->ring_used];
    }
    HIP_TRY(hipEventRecord(s.e0, c->stream));
    return RT_OK;
}

// The span's end here on the stream, ahead of work end_timed's caller still issues.
int mark_end(rt_ctx* c, TimedSpan& s) {
    HIP_TRY(hipEventRecord(s.e1, c->stream));
    s.ended = true;
    return RT_OK;
}

int end_timed(rt_ctx* c, TimedSpan& s) {
    if (!s.ended)
        if (const int rc = mark_end(c, s)) return rc;
    c->last0 = s.e0;
    c->last1 = s.e1;
    if (c->ring_used < static_cast<int>(c->ring0.size())) ++c->ring_used;
    c->timed = true;
    return RT_OK;
}

int render_frame(rt_ctx* c, const KParams& kp, rt_ctx** from) {
    // this context's own pending writes first, also when a sub-context renders the frame
    if (const int rc = flush_updates(c)) return rc;
    rt_ctx* t = c;
    KParams kt = kp;
    for (int hop = 0; hop < 2; ++hop) {
        float off = kt.shadow_off;
        rt_ctx* nxt = next_hop(t, kt, off);
        if (!nxt) break;
        KParams kn;
        const int rc = fill_kparams(nxt, kt.width, kt.height, kt.y0, kt.stripe, kt.period, kt.out_rows,
                                    reinterpret_cast<float*>(kt.dst), kt.pitch, kn,
                                    kt.rgb, kt.ss);
        if (rc != RT_OK) return rc;
        kn.shadow_off = off;
        t = nxt;
        kt = kn;
    }
    if (t == c || !accel_usable(t, kt)) {
        *from = c;
        return launch(c, kp, false);
    }
    *from = t;
    t->timing = false;  // the sub-context's own events would not be read: this context's time it
    if (!c->timing) {
        const int rc = launch(t, kt, false);
        if (t->ad_ran) c->ad_from = t;
        c->last_kind = t->last_kind;
        c->timed = false;  // no events recorded for this dispatch
        return rc;
    }
    TimedSpan span;
    if (const int rc = begin_timed(c, span)) return rc;
    const int rc = launch(t, kt, false);
    if (rc != RT_OK) return rc;
    if (t->ad_ran) c->ad_from = t;
    if (const int rc2 = end_timed(c, span)) return rc2;
    c->last_kind = t->last_kind;
    t->ring_used = 0;  // its own records are not read
    return RT_OK;
}

// The output-side launch of k_box_filter for a sample frame rendered into c->ss_buf
// (`out`: the dispatch's own KParams, `out.ss` = n; rt_ctx::samples).
void launch_box_filter(rt_ctx* c, const KParams& out) {
    const int n = out.ss, w = out.width / n, rows = out.out_rows / n;
    if (n > 1 && c->adaptive >= 0.0f) {  // rt_set_adaptive's general path (launch() zeroed ad_count)
        const bool disp = out.rgb >= RT_FORMAT_RGBA8;
        auto afn = n == 2   ? (disp ? k_box_filter_adaptive<2, true> : k_box_filter_adaptive<2>)
                   : n == 4 ? (disp ? k_box_filter_adaptive<4, true> : k_box_filter_adaptive<4>)
                            : (disp ? k_box_filter_adaptive<8, true> : k_box_filter_adaptive<8>);
        hipLaunchKernelGGL(afn, dim3((w + 63) / 64, (rows + 3) / 4), dim3(256), 0, c->stream, c->ss_buf,
                           static_cast<size_t>(out.width) * sizeof(float4), out.dst, out.pitch, w, out.height / n,
                           out.y0 / n, out.stripe / n, out.period / n, rows, out.rgb, c->adaptive, c->ad_count);
        return;
    }
    auto kfn = n == 2 ? k_box_filter<2> : n == 4 ? k_box_filter<4> : k_box_filter<8>;
    if (out.rgb >= RT_FORMAT_RGBA8)  // n == 1: the conversion alone (rt_debug_convert_pass)
        kfn = n == 1   ? k_box_filter<1, true>
              : n == 2 ? k_box_filter<2, true>
              : n == 4 ? k_box_filter<4, true>
                       : k_box_filter<8, true>;
    hipLaunchKernelGGL(kfn, dim3((w + 63) / 64, (rows + 3) / 4), dim3(256), 0, c->stream, c->ss_buf,
                       static_cast<size_t>(out.width) * sizeof(float4), out.dst, out.pitch, w, out.height / n,
                       out.y0 / n, out.stripe / n, out.period / n, rows, out.rgb);
}

// Passes 2 and 3 of rt_set_adaptive's fast path, behind the one-sample render of B into
// c->ss_buf: `out` is B's frame with the dispatch's dst / pitch / format, `smp` the sample
// frame. The host never reads the list's length: the refine grid is the worst case.
void launch_adaptive(rt_ctx* c, const AccelPtrs& A, const KParams& out, const KParams& smp) {
    const dim3 grid((out.width + kTileW - 1) / kTileW, (out.out_rows + kTileH - 1) / kTileH);
    hipLaunchKernelGGL(k_adaptive_classify, grid, dim3(kBlock), 0, c->stream, out, c->ss_buf,
                       static_cast<size_t>(out.width) * sizeof(float4), c->adaptive, c->ad_list, c->ad_count);
    const bool disp = smp.rgb >= RT_FORMAT_RGBA8;
    auto kfn = c->accel.mt ? (disp ? k_accel_refine<true, true> : k_accel_refine<true, false>)
                           : (disp ? k_accel_refine<false, true> : k_accel_refine<false, false>);
    const unsigned long long per = 64 / (smp.ss * smp.ss);  // pixels per wave
    const unsigned long long px = static_cast<unsigned long long>(out.width) * out.out_rows;
    hipLaunchKernelGGL(kfn, dim3(static_cast<unsigned>((px + per - 1) / per)), dim3(64), lane_stack_lds(smp), c->stream,
                       A, c->mat, smp, c->ad_list, c->ad_count);
}

// KParams' row mapping as dispatch_plan.h takes it, and back.
rtp::Frame frame_of(const KParams& k) {
    return rtp::Frame{k.width, k.height, k.y0, k.stripe, k.period, k.out_rows, k.resX, k.resY};
}
void set_frame(KParams& k, const rtp::Frame& f) {
    k.width = f.width;
    k.height = f.height;
    k.y0 = f.y0;
    k.stripe = f.stripe;
    k.period = f.period;
    k.out_rows = f.out_rows;
    k.resX = f.resX;
    k.resY = f.resY;
}

// The dispatch order of a k_accel frame of k2.tiles tiles, and whether it records its tiles'
// costs for the next frame's (k2.tile_cost): the caller's own order (rt_set_tile_order), or
// with rt_set_schedule the context's cost order once a frame of this size recorded one; a
// cost frame when there is none, and every `period` frames.
int cost_order_setup(rt_ctx* c, KParams& k2, int period) {
    k2.tile_order = nullptr;
    k2.tile_cost = nullptr;
    if (c->tile_order && c->tile_order_n == k2.tiles) {
        k2.tile_order = c->tile_order;
        return RT_OK;
    }
    if (c->schedule == RT_SCHED_ROWS) return RT_OK;
    if (c->sched_cap < k2.tiles) {
        // costs, order and bucket sets share one capacity: the context's once all three stand
        int cap = 0;
        drop_buffer(c->sched_cost, c->sched_cap);
        drop_buffer(c->sched_order, c->sched_cap);
        drop_buffer(c->sched_sets, c->sched_cap);
        c->sched_valid = 0;
        if (renew_buffer(c, c->sched_cost, cap, k2.tiles, k2.tiles * sizeof(unsigned)) != RT_OK ||
            renew_buffer(c, c->sched_order, cap, k2.tiles, k2.tiles * sizeof(int)) != RT_OK)
            return RT_ERR_NO_MEMORY;
        if (const int rc = renew_buffer(c, c->sched_sets, cap, k2.tiles,
                                        2 * sched_set_words(k2.tiles) * sizeof(unsigned), true))
            return rc;
        c->sched_parity = 0;
        c->sched_cap = cap;
    }
    k2.sched_hist = c->sched_sets + c->sched_parity * sched_set_words(c->sched_cap);
    const bool have = c->sched_valid == k2.tiles;
    if (have) k2.tile_order = c->sched_order;
    if (!have || c->sched_frame % period == 0) {
        k2.tile_cost = c->sched_cost;
        c->sched_frame = 0;
    }
    ++c->sched_frame;
    return RT_OK;
}

// The split tiles' part sums and counts of a cost frame (k_accel's comment), zeroed on the stream.
int heavy_acc_setup(rt_ctx* c, KParams& k2) {
    k2.heavy_acc = nullptr;
    if (!k2.tile_cost || k2.heavy_k <= 0) return RT_OK;
    const size_t need = static_cast<size_t>(k2.heavy_k);
    if (c->heavy_acc_cap < need)
        if (const int rc = renew_buffer(c, c->heavy_acc, c->heavy_acc_cap, need, need * sizeof(unsigned long long)))
            return rc;
    HIP_TRY(hipMemsetAsync(c->heavy_acc, 0, need * sizeof(unsigned long long), c->stream));
    k2.heavy_acc = c->heavy_acc;
    return RT_OK;
}

// The queue and the region counters of a compacting dispatch (rtp::tail_plan).
int tail_setup(rt_ctx* c, KParams& k2, const rtp::TailPlan& t) {
    const size_t need = static_cast<size_t>(t.regions) * kTailRegion;
    if (need > c->tail_cap)
        // 3 float4 records, then the pixel words (rt_device.h, tail_queue)
        if (const int rc = renew_buffer(c, c->tail_queue, c->tail_cap, need, need * (3 * sizeof(float4) + sizeof(int))))
            return rc;
    if (t.regions > c->tail_regions_cap)
        if (const int rc = renew_buffer(c, c->tail_counts, c->tail_regions_cap, t.regions,
                                        2 * static_cast<size_t>(t.regions) * sizeof(int), true))
            return rc;
    k2.tail_queue = c->tail_queue;
    k2.tail_px = reinterpret_cast<int*>(c->tail_queue + 3 * c->tail_cap);
    k2.tail_count = c->tail_counts + c->tail_parity * c->tail_regions_cap;
    k2.tail_count_next = c->tail_counts + (1 - c->tail_parity) * c->tail_regions_cap;
    k2.tail_from = t.tail_from;
    k2.tail_rx = t.rx;
    k2.tail_regions = t.regions;
    k2.tail_counters = c->tail_regions_cap;
    k2.tail_max_lanes = c->tail_max_lanes;
    return RT_OK;
}

// Behind a cost frame's render:
// the next frame's order; stream-ordered after this dispatch (and after its
// end event, so rt_kernel_times is the render kernel alone), before the next
int launch_cost_order(rt_ctx* c, const KParams& k2, bool latency, int dilate, TimedSpan* span) {
    if (span)
        if (const int rc = mark_end(c, *span)) return rc;
    const unsigned* set = c->sched_sets + c->sched_parity * sched_set_words(c->sched_cap);
    unsigned* next = c->sched_sets + (1 - c->sched_parity) * sched_set_words(c->sched_cap);
    const int groups = (k2.tiles + kOrderThreads - 1) / kOrderThreads;
    const unsigned* cost = c->sched_cost;
    if (latency && c->frame_event) {
        // a waited frame ends here (rt_sync_frame); the order runs behind it on the same
        // stream, within the host's turnaround to the next dispatch
        if (!c->frame_ev && hipEventCreateWithFlags(&c->frame_ev, hipEventDisableTiming) != hipSuccess)
            return RT_ERR_DEVICE;
        HIP_TRY(hipEventRecord(c->frame_ev, c->stream));
        c->frame_ev_set = true;
    }
    if (dilate > 0) {
        const size_t need = static_cast<size_t>(k2.tiles) + static_cast<size_t>(groups) * kOrderBuckets;
        if (c->dil_cap < need)
            if (const int rc = renew_buffer(c, c->dil_cost, c->dil_cap, need, need * sizeof(unsigned))) return rc;
        hipLaunchKernelGGL(k_cost_dilate, dim3(groups), dim3(kOrderThreads), 0, c->stream, c->sched_cost,
                           k2.tiles, k2.tiles_x, dilate, c->dil_cost, c->dil_cost + k2.tiles);
        cost = c->dil_cost;
        set = c->dil_cost + k2.tiles;
    }
    hipLaunchKernelGGL(k_tile_order, dim3(groups), dim3(kOrderThreads),
                       0, c->stream, cost, k2.tiles, set, next,
                       static_cast<int>(sched_set_words(c->sched_cap)), c->sched_order,
                       c->schedule == RT_SCHED_COST_XCD ? 1 : 0);
    c->sched_parity = 1 - c->sched_parity;
    c->sched_valid = k2.tiles;
    return RT_OK;
}

// launch()'s RT_KERNEL_ACCEL branch. `kp`: the frame k_accel renders; `kin`: the dispatch's
// own frame, `kout` its one-sample output frame (rt_set_adaptive); `span`: the dispatch's
// timing span, or nullptr when it records none.
int launch_accel(rt_ctx* c, const KParams& kin, const KParams& kout, const KParams& kp, const rtp::Samples& sp,
                 TimedSpan* span) {
    KParams k2 = kp;
    k2.tiles_x = (kp.width + 7) / 8;
    k2.tiles = k2.tiles_x * ((kp.out_rows + 7) / 8);
    const bool latency = rtp::latency_frame(c->latency_mode, k2.tiles, c->cu_count);
    // a moved camera's cost order (moving_period): waited frames only -- with frames in
    // flight a cost frame after every move cost the car's orbit 0.194 -> 0.238 ms per
    // frame (r05j), and the order matters less there
    c->moving = latency && c->have_sched_cam && std::memcmp(&c->sched_cam, &c->cam, sizeof c->cam) != 0 &&
                c->moving_period > 0;
    c->sched_cam = c->cam;
    c->have_sched_cam = true;
    const int period = c->moving ? c->moving_period : c->sched_period;
    const int dilate = c->moving ? c->moving_dilate : c->cost_dilate;
    k2.tile_times = c->tile_times;
    if (c->tile_times)
        HIP_TRY(hipMemsetAsync(c->tile_times, 0, kTileRec * c->tile_times_cap * sizeof(unsigned long long),
                               c->stream));
    k2.heavy_k = 0;
    k2.heavy_parts = 1;
    if (const int rc = cost_order_setup(c, k2, period)) return rc;
    k2.lane_from_depth = walk_from(c);
    // (not with maxBounces = 0: the shader traces nothing then and the pixel is black, while
    // the kernel's root test would hand a ray that misses the root its background)
    k2.root_ok = 0;
    if (kp.maxBounces > 0 && kp.useBVH) root_bounds(c, k2);
    // big scenes (the RT_TAIL_AUTO criterion): camera rays' shadow walks per lane too
    // (measured on config 5: -3.7 %; on the car the packet walk is faster)
    const size_t items = c->accel.st.item_ref.size();
    k2.shadow_lane_from = c->shadow_walk_override >= 0 ? c->shadow_walk_override
                          : (rtp::many_items(items) && k2.lane_from_depth <= 1 ? 0 : k2.lane_from_depth);
    k2.lane_stack = lane_stack_entries(c);  // the accelerator's as flush_updates left it
    const bool lanes = std::min(k2.lane_from_depth, k2.shadow_lane_from) < k2.maxBounces;
    const bool ordered = k2.tile_order && k2.tile_order == c->sched_order;
    if (ordered) {
        const rtp::LaneSlots ls = rtp::lane_k_slots(c->lane_k, c->lane_k_mode, lanes, k2.tiles);
        if (ls.k > 0) {
            k2.lane_k = ls.k;
            k2.lane_k_mode = ls.mode;
        }
    }
    // LDS stacks for the per-lane walks (also those of the lane_k slots)
    const size_t lds = lanes || k2.lane_k > 0 ? lane_stack_lds(k2) : 0;
    if (ordered) {
        const bool whole = k2.tile_cost && c->cost_time != 0 && !c->tile_times && latency &&
                           !(c->moving && c->moving_split);
        const rtp::HeavySplit hs = rtp::heavy_split(rtp::HeavyIn{
            k2.tiles, c->cu_count, latency, lanes, c->heavy_k, c->heavy_parts, c->tile_times != nullptr,
            c->tile_times_cap, whole, sp.ss_fused, k2.ss});
        k2.heavy_k = hs.k;
        k2.heavy_parts = hs.parts;
    }
    // the cost measure: explicit (rt_debug_cost_time) or the waves' wall time
    k2.cost_time = c->cost_time != 0 ? 1 : 0;
    if (const int rc = heavy_acc_setup(c, k2)) return rc;
    const AccelPtrs A = accel_ptrs(c);
    k2.tail_queue = nullptr;
    const rtp::TailPlan tp = rtp::tail_plan(c->tail_from, items, k2.maxBounces, sp.ss_fused, k2.width, k2.out_rows,
                                            k2.tiles_x, k2.tiles);
    if (tp.tail)
        if (const int rc = tail_setup(c, k2, tp)) return rc;
    const rtp::Cost cost = !k2.tile_cost ? rtp::kCostNone : k2.cost_time ? rtp::kCostTime : rtp::kCostCounters;
    const rtp::AccelInstance inst =
        rtp::accel_instance(c->accel.mt, c->tile_times != nullptr, tp.tail, latency, cost, sp.ss_fused);
    if (!inst.queue) k2.tail_queue = nullptr;  // an instance without compaction
    const AccelFn kfn = accel_kernel(inst, k2.rgb >= RT_FORMAT_RGBA8);
    if (!kfn) return RT_ERR_INVALID;
    // one wave per dispatch slot: the split heavy tiles' extra waves too
    const int blocks = k2.tiles + k2.heavy_k * (k2.heavy_parts - 1);
    hipLaunchKernelGGL(kfn, dim3(blocks), dim3(64), lds, c->stream, A, c->mat, k2);
    if (inst.queue) {
        const int tgrid = tp.regions * (kTailRegion / 64);  // one wave per possible chunk
        hipLaunchKernelGGL(k_accel_tail, dim3(tgrid), dim3(64), lane_stack_lds(k2), c->stream, A, c->mat, k2);
        c->tail_parity = 1 - c->tail_parity;
    }
    if (sp.filter) launch_box_filter(c, kin);
    if (sp.ad_fast) {
        KParams smp = kin;  // the sample frame, walked per lane
        smp.lane_stack = k2.lane_stack;
        launch_adaptive(c, A, kout, smp);
    }
    return k2.tile_cost ? launch_cost_order(c, k2, latency, dilate, span) : RT_OK;
}

// launch()'s render of a frame of two or more lights (rtp::lights_route): k_lights over the
// context's accelerator, one wave per 8x8 tile in row-major order, or k_lights_ref on k_lane's
// grid. The set is the context's (a sub-context inherits its parent's). No cost order, no
// latency mode, no compaction, no walk policy: the frame's walks are fixed (k_lights).
// The frame of k_lights / k_soft: one wave per 8x8 tile in row-major tile order, the root's
// bounds for the sky skip, the lane stacks.
KParams tile_frame(rt_ctx* c, const KParams& kp) {
    KParams k2 = kp;
    k2.tiles_x = (kp.width + 7) / 8;
    k2.tiles = k2.tiles_x * ((kp.out_rows + 7) / 8);
    k2.root_ok = 0;  // (not with maxBounces = 0: launch_accel)
    if (kp.maxBounces > 0 && kp.useBVH) root_bounds(c, k2);
    k2.lane_stack = lane_stack_entries(c);
    return k2;
}

void launch_lights(rt_ctx* c, const KParams& kp, bool accel, dim3 lane_grid) {
    const LightSet L = make_light_set(c->lights, c->nlights);
    const ShadeArgs q{nullptr, 0};
    const bool disp = kp.rgb >= RT_FORMAT_RGBA8;
    if (!accel) {
        auto kfn = disp ? k_lights_ref<true, true> : k_lights_ref<false, true>;
        hipLaunchKernelGGL(kfn, lane_grid, dim3(kBlock), ref_stack_lds(kp), c->stream, q, L, kp);
        return;
    }
    const KParams k2 = tile_frame(c, kp);
    auto kfn = c->accel.mt ? (disp ? k_lights<true, true, true> : k_lights<true, false, true>)
                           : (disp ? k_lights<false, true, true> : k_lights<false, false, true>);
    hipLaunchKernelGGL(kfn, dim3(k2.tiles), dim3(64), lane_stack_lds(k2), c->stream, accel_ptrs(c), c->mat, q, L, k2);
}

// Later bounces' sample rays repacked over the wave (k_soft's PACK) or per live lane:
// rtp::soft_repack, the measured rule; rt_debug_soft overrides it.
bool soft_pack(const rt_ctx* c, const KParams& kp) { return rtp::soft_repack(c->soft_form, kp.maxBounces); }
size_t soft_lds(const KParams& kp, bool pack) {
    return lane_stack_lds(kp) + (pack ? kSoftSlot * 64 * sizeof(int) : 0);
}
using SoftKernel = void (*)(AccelPtrs, const float4*, ShadeArgs, LightSet, SoftSet, KParams);
template <bool FRAME, bool PACK>
SoftKernel soft_kernel_of(bool mt, bool disp) {
    return mt ? (disp ? k_soft<true, true, FRAME, PACK> : k_soft<true, false, FRAME, PACK>)
              : (disp ? k_soft<false, true, FRAME, PACK> : k_soft<false, false, FRAME, PACK>);
}
template <bool FRAME>
SoftKernel soft_kernel(bool mt, bool disp, bool pack) {
    return pack ? soft_kernel_of<FRAME, true>(mt, disp) : soft_kernel_of<FRAME, false>(mt, disp);
}

// launch()'s render of a soft frame (rtp::soft_route): launch_lights with the context's radii
// and K -- k_soft over the accelerator, one wave per 8x8 tile in row-major order, or k_soft_ref
// on k_lane's grid.
void launch_soft(rt_ctx* c, const KParams& kp, bool accel, dim3 lane_grid) {
    const LightSet L = make_light_set(c->lights, c->nlights);
    const SoftSet S = make_soft_set(c->soft_radii, c->soft_count, c->soft_samples);
    const ShadeArgs q{nullptr, 0};
    const bool disp = kp.rgb >= RT_FORMAT_RGBA8;
    if (!accel) {
        auto kfn = disp ? k_soft_ref<true, true> : k_soft_ref<false, true>;
        hipLaunchKernelGGL(kfn, lane_grid, dim3(kBlock), ref_stack_lds(kp), c->stream, q, L, S, kp);
        return;
    }
    const KParams k2 = tile_frame(c, kp);
    const bool pack = soft_pack(c, k2);
    hipLaunchKernelGGL(soft_kernel<true>(c->accel.mt, disp, pack), dim3(k2.tiles), dim3(64), soft_lds(k2, pack), c->stream,
                       accel_ptrs(c), c->mat, q, L, S, k2);
}

int launch(rt_ctx* c, const KParams& kin, bool stats) {
    c->frame_ev_set = false;
    c->ad_ran = false;
    if (const int rc = flush_updates(c)) return rc;  // rt_update_shapes / rt_update_nodes since the last dispatch
    if (kin.out_rows == 0) return RT_OK;
    dim3 grid((kin.width + kTileW - 1) / kTileW, (kin.out_rows + kTileH - 1) / kTileH);
    if (grid.y > 65535u) return RT_ERR_INVALID;
    int kind = c->kernel;
    const bool usable = accel_usable(c, kin);
    if (kind == RT_KERNEL_AUTO) kind = usable ? RT_KERNEL_ACCEL : RT_KERNEL_PACKET;
    if (kind == RT_KERNEL_ACCEL && !usable) kind = RT_KERNEL_PACKET;  // same image either way
    // rt_set_lights: two or more lights render in k_lights / k_lights_ref; one light takes
    // every path below as it always did
    const rtp::LightsRoute lr = rtp::lights_route(c->nlights, stats, kind == RT_KERNEL_ACCEL);
    // rt_set_soft_shadows: a light of the set with a radius > 0 renders in k_soft / k_soft_ref,
    // one light included; consulted first, and off for every frame without such a light
    const rtp::SoftRoute so = rtp::soft_route(c->nlights, c->soft_radii, stats, kind == RT_KERNEL_ACCEL);
    const rtp::Samples sp =
        rtp::samples_plan(stats, kin.ss, rtp::accel_renders(kind == RT_KERNEL_ACCEL, lr, so), c->tile_times != nullptr,
                          c->ss_general, c->adaptive >= 0.0f, c->convert_pass, kin.rgb >= RT_FORMAT_RGBA8);
    KParams kout = kin;  // adaptive: the one-sample output frame, B's, with the dispatch's dst / pitch / format
    if (sp.adaptive) {
        set_frame(kout, rtp::output_frame(frame_of(kin), kin.ss));
        kout.ss = 1;
    }
    KParams kp = sp.ad_fast ? kout : kin;
    if (sp.adaptive) {
        if (!c->ad_count && hipMalloc(&c->ad_count, 4 * sizeof(unsigned)) != hipSuccess) return RT_ERR_NO_MEMORY;
        const size_t cap = static_cast<size_t>(kout.width) * static_cast<size_t>(kout.out_rows);
        if (sp.ad_fast && cap > c->ad_cap) {
            HIP_TRY(sync_stream(c));
            if (const int rc = renew_buffer(c, c->ad_list, c->ad_cap, cap, cap * sizeof(unsigned))) return rc;
        }
    }
    if (sp.filter || sp.ad_fast) {
        const size_t spitch = static_cast<size_t>(kp.width) * sizeof(float4);
        const size_t need = spitch * static_cast<size_t>(kp.out_rows);
        if (need != c->ss_bytes) {
            HIP_TRY(sync_stream(c));
            if (const int rc = renew_buffer(c, c->ss_buf, c->ss_bytes, need, need)) return rc;
        }
        kp.dst = c->ss_buf;
        kp.pitch = spitch;
        kp.rgb = RT_FORMAT_RGBA32F;
        kp.ss = 1;
    }
    const size_t lds = ref_stack_lds(kp);
    const bool rec = !stats && c->timing;  // rt_set_kernel_timing
    TimedSpan span;
    if (rec)
        if (const int rc = begin_timed(c, span)) return rc;
    if (sp.adaptive) {
        // the refined-pixel counter, zeroed in stream order; its last value stays for rt_adaptive_stats
        HIP_TRY(hipMemsetAsync(c->ad_count, 0, sizeof(unsigned), c->stream));
        c->ad_ran = true;
        c->ad_from = c;
        c->ad_pixels = rtp::dispatch_pixels(frame_of(kout));
    }
    if (stats) {
        hipLaunchKernelGGL(k_lane<true>, grid, dim3(kBlock), lds, c->stream, c->geo_leaf, c->geo_lin, c->mat,
                           c->nodes, kp);
    } else if (so != rtp::kSoftOff) {
        launch_soft(c, kp, so == rtp::kSoftAccel, grid);
        if (sp.filter) launch_box_filter(c, kin);
        kind = so == rtp::kSoftAccel ? RT_KERNEL_SOFT : RT_KERNEL_LANE;
    } else if (lr != rtp::kLightsOff) {
        launch_lights(c, kp, lr == rtp::kLightsAccel, grid);
        if (sp.filter) launch_box_filter(c, kin);
        kind = lr == rtp::kLightsAccel ? RT_KERNEL_LIGHTS : RT_KERNEL_LANE;
    } else if (kind == RT_KERNEL_LANE) {
        hipLaunchKernelGGL(k_lane<false>, grid, dim3(kBlock), lds, c->stream, c->geo_leaf, c->geo_lin, c->mat,
                           c->nodes, kp);
        if (sp.filter) launch_box_filter(c, kin);
    } else if (kind == RT_KERNEL_ACCEL) {
        // (on cost frames the span ends between the render and the order kernels: mark_end)
        if (const int rc = launch_accel(c, kin, kout, kp, sp, rec ? &span : nullptr)) return rc;
    } else {
        hipLaunchKernelGGL(k_packet, grid, dim3(kBlock), 0, c->stream, c->geo_leaf, c->geo_lin, c->mat, c->nodes,
                           kp);
        if (sp.filter) launch_box_filter(c, kin);
    }
    c->last_kind = stats ? RT_KERNEL_LANE : kind;
    HIP_TRY(hipGetLastError());
    if (rec) {
        if (const int rc = end_timed(c, span)) return rc;
    } else if (!stats) {
        c->timed = false;  // rt_set_kernel_timing(0): rt_last_kernel_ms has no dispatch to report
    }
    return RT_OK;
}

// One query launch on the context's stream (rt_trace_rays and its host forms): pending
// scene writes first, as one refit; then k_trace over the accelerator the next dispatch
// would walk (the context's own, or mtc's for Moller-Trumbore), or k_trace_ref's literal
// walk when there is none or rt_set_kernel chose the lane / packet kernel. None of the
// render state (last_kind, the timing ring, the frame marker, the cost order) is touched.
// The context whose device scene a query or a geometry buffer reads, after its pending
// scene writes went in as one refit: the context's own, or mtc for Moller-Trumbore.
// *accel: its accelerator serves the walk (else the literal reference walk).
int query_target(rt_ctx* c, rt_ctx** target, bool* accel) {
    if (const int rc = flush_updates(c)) return rc;
    const bool mt = c->params.useMollerTrumbore != 0;
    rt_ctx* t = c;
    if (mt) {
        KParams sel;
        std::memset(&sel, 0, sizeof sel);
        sel.useBVH = sel.useMT = 1;
        if (rt_ctx* b = mt_ctx(c, sel)) {
            if (const int rc = flush_updates(b)) return rc;
            if (b->accel_ok) t = b;
        }
    }
    *target = t;
    *accel = (c->kernel == RT_KERNEL_AUTO || c->kernel == RT_KERNEL_ACCEL) && t->accel_ok && t->accel.mt == mt;
    return RT_OK;
}

int trace_launch(rt_ctx* c, const float4* rays, const int2* xy, int n, float4* hits, int mode) {
    rt_ctx* t = c;
    bool accel = false;
    if (const int rc = query_target(c, &t, &accel)) return rc;
    const bool mt = c->params.useMollerTrumbore != 0;
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    scene_params(t, kp);
    kp.useBVH = 1;
    kp.useMT = mt ? 1 : 0;
    if (xy) camera_params(c, kp);
    const TraceArgs q{rays, xy, hits, n};
    const bool any = mode == RT_TRACE_ANY;
    if (accel) {
        auto kfn = mt ? (any ? k_trace<RT_TRACE_ANY, true> : k_trace<RT_TRACE_CLOSEST, true>)
                      : (any ? k_trace<RT_TRACE_ANY, false> : k_trace<RT_TRACE_CLOSEST, false>);
        hipLaunchKernelGGL(kfn, dim3((n + 63) / 64), dim3(64), lane_stack_lds(kp), c->stream, accel_ptrs(t), q, kp);
    } else {
        auto kfn = any ? k_trace_ref<RT_TRACE_ANY> : k_trace_ref<RT_TRACE_CLOSEST>;
        hipLaunchKernelGGL(kfn, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), ref_stack_lds(kp), c->stream, q, kp);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The checks every query form shares; RT_OK with *run = false when there is nothing to launch.
int trace_check(const rt_ctx* c, const void* in, int n, const void* hits, int mode, bool* run) {
    *run = false;
    if (!c || n < 0 || (mode != RT_TRACE_CLOSEST && mode != RT_TRACE_ANY) || (n > 0 && (!in || !hits)))
        return RT_ERR_INVALID;
    if (!c->have_scene) return RT_ERR_NO_SCENE;
    *run = n > 0;
    return RT_OK;
}

// Host queries: `in` (n records of in_bytes each: rt_ray, or a pixel's two ints) through
// the context's staging buffers, the launch, and the hits back.
int trace_staged(rt_ctx* c, const void* in, size_t in_bytes, bool pixels, int n, rt_hit* hits, int mode) {
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    const size_t in16 = (static_cast<size_t>(n) * in_bytes + 15) / 16;
    int rc = ensure_staging(c->trace_in, c->trace_in_cap, in16);
    if (rc == RT_OK) rc = ensure_staging(c->trace_hits, c->trace_hits_cap, static_cast<size_t>(n));
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->trace_in, in, static_cast<size_t>(n) * in_bytes, hipMemcpyHostToDevice, c->stream));
    rc = trace_launch(c, pixels ? nullptr : c->trace_in, pixels ? reinterpret_cast<const int2*>(c->trace_in) : nullptr,
                      n, c->trace_hits, mode);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hits, c->trace_hits, static_cast<size_t>(n) * sizeof(rt_hit), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

// Geometry buffers. The checks of rt_dispatch_gbuffer and rt_gbuffer_host (include/rt_api.h),
// before anything is launched; RT_OK with *run = false when there is nothing to launch.
// Tiles per block: one, as k_accel and k_trace. Two and four measured equal or slower
// (tools/bench_gbuffer.py's a_w2 and a_w4, DESIGN.md §4 "Geometry buffers").
constexpr int kGbufWaves = 1;

// A per-pixel plane dispatch's row mapping (as fill_kparams checks a frame's) and its size: a
// grid of tile rows the launch can have, and row * width + x in 32 bits.
bool plane_rows_ok(int width, int height, int y0, int stripe, int period, int out_rows) {
    return width > 0 && height > 0 && stripe > 0 && period >= stripe && out_rows >= 0 && y0 >= 0 &&
           (static_cast<long long>(out_rows) + kTileH - 1) / kTileH <= 65535 &&
           static_cast<unsigned long long>(width) * static_cast<unsigned long long>(out_rows) < (1ull << 32);
}

int gbuffer_check(const rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows,
                  const rt_gbuffer* out, bool* run) {
    *run = false;
    if (!c || !out || (!out->shape && !out->depth && !out->normal && !out->position)) return RT_ERR_INVALID;
    if (!c->have_scene || !c->have_cam || !c->have_params) return RT_ERR_NO_SCENE;
    if (!plane_rows_ok(width, height, y0, stripe, period, out_rows)) return RT_ERR_INVALID;
    const struct {
        const void* p;
        size_t pitch, px;
    } planes[4] = {{out->shape, out->shape_pitch, 4},
                   {out->depth, out->depth_pitch, 4},
                   {out->normal, out->normal_pitch, 16},
                   {out->position, out->position_pitch, 16}};
    for (const auto& pl : planes)
        if (pl.p && (pl.pitch < static_cast<size_t>(width) * pl.px || pl.pitch % pl.px != 0 ||
                     reinterpret_cast<uintptr_t>(pl.p) % pl.px != 0))
            return RT_ERR_INVALID;
    *run = out_rows > 0;
    return RT_OK;
}

// The kernel parameters of a geometry-buffer or ambient-occlusion launch over target t: the
// scene, the stacks, the camera and the row mapping; nothing of the shading.
KParams plane_params(const rt_ctx* c, const rt_ctx* t, int width, int height, int y0, int stripe, int period,
                     int out_rows) {
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    scene_params(t, kp);
    kp.useBVH = 1;
    kp.useMT = c->params.useMollerTrumbore != 0 ? 1 : 0;
    camera_params(c, kp);
    kp.width = width;
    kp.height = height;
    kp.y0 = y0;
    kp.stripe = stripe;
    kp.period = period;
    kp.out_rows = out_rows;
    kp.tiles_x = (width + 7) / 8;
    kp.tiles = kp.tiles_x * ((out_rows + 7) / 8);
    return kp;
}

// One geometry-buffer launch on the context's stream: pending scene writes first, as one
// refit (query_target); then k_gbuffer over the accelerator a query would walk -- as packets
// while the camera lies inside its origin bound, per lane beyond it -- or k_gbuffer_ref's
// literal walk. Like a query it touches none of the render state.
int gbuffer_launch(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows,
                   const rt_gbuffer& g) {
    rt_ctx* t = c;
    bool accel = false;
    if (const int rc = query_target(c, &t, &accel)) return rc;
    const bool mt = c->params.useMollerTrumbore != 0;
    KParams kp = plane_params(c, t, width, height, y0, stripe, period, out_rows);
    if (!accel) {
        const dim3 grid((width + kTileW - 1) / kTileW, (out_rows + kTileH - 1) / kTileH);
        hipLaunchKernelGGL(k_gbuffer_ref, grid, dim3(kBlock), ref_stack_lds(kp), c->stream, g, kp);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
    root_bounds(t, kp);  // whatever maxBounces says (plane_params leaves it 0): the camera ray is always traced
    // the packet form needs the shared origin inside the accelerator's bound (accel_usable)
    const float cmag = std::max({std::fabs(kp.cam_pos.x), std::fabs(kp.cam_pos.y), std::fabs(kp.cam_pos.z)});
    const bool lane = c->gbuf_walk == 1 || !(cmag <= t->accel.origin_lim);
    int waves = c->gbuf_waves > 0 ? c->gbuf_waves : kGbufWaves;
    // the lane form's stacks (lane_stack x 6 B a lane) within the 64 KB a block may ask for
    while (lane && waves > 1 && lane_stack_lds(kp) * waves > 65536) waves /= 2;
    const dim3 grid((kp.tiles + waves - 1) / waves), block(64 * waves);
    auto kfn = lane ? (mt ? k_gbuffer<true, true> : k_gbuffer<false, true>)
                    : (mt ? k_gbuffer<true, false> : k_gbuffer<false, false>);
    const size_t lds = lane ? lane_stack_lds(kp) * waves : 0;  // the packet form: no LDS
    hipLaunchKernelGGL(kfn, grid, block, lds, c->stream, accel_ptrs(t), g, kp);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Ambient occlusion. The checks of rt_dispatch_ao and rt_ao_host (include/rt_api.h), before
// anything is launched; RT_OK with *run = false when there is nothing to launch.
// The default form: per hit lane. It measured 5-23 % faster than the repacked form in 17 of the
// 18 rows of tools/bench_ao.py (three scenes, K = 4, 16, 64, radius 2.0 and +inf) and equal in
// one (DESIGN.md §4 "Ambient occlusion"): most tiles of those frames are all hits or all sky,
// where repacking only adds its LDS traffic. Tiles per block: one; two and four measured equal or slower.
constexpr bool kAoPack = false;
constexpr int kAoWaves = 1;

int ao_check(const rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows,
             const rt_ao_params* p, const rt_ao* out, bool* run) {
    *run = false;
    if (!c || !p || !out || (!out->count && !out->visibility)) return RT_ERR_INVALID;
    if (!c->have_scene || !c->have_cam || !c->have_params) return RT_ERR_NO_SCENE;
    if (!plane_rows_ok(width, height, y0, stripe, period, out_rows)) return RT_ERR_INVALID;
    if (p->rays < 1 || p->rays > 64 || !(p->radius > 0.0f) || !(p->bias >= 0.0f) || std::isinf(p->bias) ||
        p->reserved != 0)
        return RT_ERR_INVALID;
    if (out->count && out->count_pitch < static_cast<size_t>(width)) return RT_ERR_INVALID;
    if (out->visibility && (out->visibility_pitch < static_cast<size_t>(width) * 4 || out->visibility_pitch % 4 != 0 ||
                            reinterpret_cast<uintptr_t>(out->visibility) % 4 != 0))
        return RT_ERR_INVALID;
    *run = out_rows > 0;
    return RT_OK;
}

// One ambient-occlusion launch on the context's stream, set up as gbuffer_launch: the same
// target, parameters and camera-walk choice; k_ao's LDS is the lane stacks of its occlusion
// walks (always) and, repacked (rt_debug_ao form 1), 15 dwords per lane for the hit lanes'
// frames and counters.
int ao_launch(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows, const rt_ao_params& p,
              const rt_ao& out) {
    rt_ctx* t = c;
    bool accel = false;
    if (const int rc = query_target(c, &t, &accel)) return rc;
    const bool mt = c->params.useMollerTrumbore != 0;
    KParams kp = plane_params(c, t, width, height, y0, stripe, period, out_rows);
    const AoArgs q{out, p.rays, p.radius, p.bias};
    if (!accel) {
        const dim3 grid((width + kTileW - 1) / kTileW, (out_rows + kTileH - 1) / kTileH);
        hipLaunchKernelGGL(k_ao_ref, grid, dim3(kBlock), ref_stack_lds(kp), c->stream, q, kp);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
    root_bounds(t, kp);
    const float cmag = std::max({std::fabs(kp.cam_pos.x), std::fabs(kp.cam_pos.y), std::fabs(kp.cam_pos.z)});
    const bool lane = !(cmag <= t->accel.origin_lim);
    const bool pack = c->ao_form == 0 ? kAoPack : c->ao_form == 1;
    const size_t per_wave = lane_stack_lds(kp) + (pack ? kAoSlot * 64 * sizeof(int) : 0);
    int waves = c->ao_waves > 0 ? c->ao_waves : kAoWaves;
    while (waves > 1 && per_wave * waves > 65536) waves /= 2;  // within the 64 KB a block may ask for
    const dim3 grid((kp.tiles + waves - 1) / waves), block(64 * waves);
    auto pick = [&](auto m, auto l) {
        return pack ? k_ao<decltype(m)::value, decltype(l)::value, true> : k_ao<decltype(m)::value, decltype(l)::value, false>;
    };
    using T = std::true_type;
    using F = std::false_type;
    auto kfn = mt ? (lane ? pick(T{}, T{}) : pick(T{}, F{})) : (lane ? pick(F{}, T{}) : pick(F{}, F{}));
    hipLaunchKernelGGL(kfn, grid, block, per_wave * waves, c->stream, accel_ptrs(t), q, kp);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Shaded rays. The checks of rt_shade_rays and rt_shade_rays_host (include/rt_api.h), before
// anything is launched; RT_OK with *run = false when there is nothing to launch. `device`: the
// pointers are device addresses and must be aligned for the kernels' loads and stores.
int shade_check(const rt_ctx* c, const void* rays, int n, const void* pixels, int format, bool device, bool* run) {
    *run = false;
    if (!c || n < 0 || format == RT_FORMAT_RGBA32F_IMAGE || format_bytes(format) == 0 || (n > 0 && (!rays || !pixels)))
        return RT_ERR_INVALID;
    if (device && n > 0 &&
        (reinterpret_cast<uintptr_t>(rays) % 16 != 0 || reinterpret_cast<uintptr_t>(pixels) % format_align(format) != 0))
        return RT_ERR_INVALID;
    if (!c->have_scene || !c->have_light || !c->have_params) return RT_ERR_NO_SCENE;
    *run = n > 0;
    return RT_OK;
}

// The k_shade instance with split walks (lane_walk_any's SPLIT) for barycentric scenes of at
// least this many scene-tree items, the plain one below: k_accel's rule (RT_TAIL_AUTO).
// Measured over the frame's own rays at 1920x1080, 3 bounces (tools/bench_shade.py,
// profiles/shade_bench.jsonl), split against plain: the car (1,293 items) 0.376 against
// 0.365 ms, +3 %; 100k triangles 4.514 against 4.555 ms, -1 %; the monkey scene +3 %.
// Moller-Trumbore lists always take the plain instance, as every MT frame does.
constexpr size_t kShadeSplitItems = rtp::kTailAutoItems;

// One shading launch on the context's stream: pending scene writes first, as one refit; then
// the context render_frame would take the frame to -- the brute sub-context for useBVH = 0
// (shadow offset 1e-5), the Moller-Trumbore sub-context -- without accel_usable's camera test
// (no camera enters; lane_walk handles any origin per ray); k_shade when that target's
// accelerator is built for the wanted triangle test, else k_shade_ref over this context's own
// records. Like a query it touches none of the render state.
int shade_launch(rt_ctx* c, const float4* rays, int n, void* pixels, int format) {
    if (const int rc = flush_updates(c)) return rc;
    rt_ctx* t = c;
    KParams sel;
    std::memset(&sel, 0, sizeof sel);
    sel.useBVH = c->params.useBVH;
    sel.useMT = c->params.useMollerTrumbore;
    float off = 1e-3f;
    for (int hop = 0; hop < 2; ++hop) {
        rt_ctx* nxt = next_hop(t, sel, off);
        if (!nxt) break;
        sel.useBVH = nxt->params.useBVH;
        sel.useMT = nxt->params.useMollerTrumbore;
        t = nxt;
    }
    const bool mt = sel.useMT != 0;
    const bool accel = (c->kernel == RT_KERNEL_AUTO || c->kernel == RT_KERNEL_ACCEL) && t->accel_ok && sel.useBVH &&
                       t->accel.mt == mt;
    if (!accel) t = c;
    if (t != c) {  // the sub-context's own pending writes (launch() applies them for a frame)
        if (const int rc = flush_updates(t)) return rc;
    }
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    scene_params(t, kp);
    kp.mat = t->mat;
    kp.light_pos = V{c->light.position.x, c->light.position.y, c->light.position.z};
    kp.light_color = V{c->light.color.x, c->light.color.y, c->light.color.z};
    kp.maxBounces = c->params.maxBounces;
    kp.useBVH = accel ? 1 : c->params.useBVH;
    kp.useFresnel = c->params.useFresnel;
    kp.useMT = accel ? (mt ? 1 : 0) : c->params.useMollerTrumbore;
    kp.shadow_off = off;
    kp.stripe = kp.period = 1;
    kp.dst = static_cast<char*>(pixels);
    kp.pitch = format_bytes(format) << kShadeRowShift;  // shade_row / shade_col
    kp.rgb = format;
    kp.ss = 1;
    kp.heavy_parts = 1;
    const ShadeArgs q{rays, n};
    const bool disp = format >= RT_FORMAT_RGBA8;
    // rt_set_lights: two or more lights (this context's set) in k_lights' list form, over the
    // same target; one light takes k_shade / k_shade_ref as it always did
    const rtp::LightsRoute lr = rtp::lights_route(c->nlights, false, accel);
    // rt_set_soft_shadows: a radius > 0 in the set takes k_soft's list form, consulted first
    const rtp::SoftRoute so = rtp::soft_route(c->nlights, c->soft_radii, false, accel);
    const LightSet L = make_light_set(c->lights, c->nlights);
    const SoftSet S = make_soft_set(c->soft_radii, c->soft_count, c->soft_samples);
    const dim3 waves((static_cast<unsigned>(n) + 63u) / 64u), blocks((static_cast<unsigned>(n) + kBlock - 1u) / kBlock);
    if (so == rtp::kSoftAccel) {
        const bool pack = soft_pack(c, kp);
        hipLaunchKernelGGL(soft_kernel<false>(mt, disp, pack), waves, dim3(64), soft_lds(kp, pack), c->stream,
                           accel_ptrs(t), t->mat, q, L, S, kp);
    } else if (so == rtp::kSoftRef) {
        auto kfn = disp ? k_soft_ref<true, false> : k_soft_ref<false, false>;
        hipLaunchKernelGGL(kfn, blocks, dim3(kBlock), ref_stack_lds(kp), c->stream, q, L, S, kp);
    } else if (lr == rtp::kLightsAccel) {
        auto kfn = mt ? (disp ? k_lights<true, true, false> : k_lights<true, false, false>)
                      : (disp ? k_lights<false, true, false> : k_lights<false, false, false>);
        hipLaunchKernelGGL(kfn, waves, dim3(64), lane_stack_lds(kp), c->stream, accel_ptrs(t), t->mat, q, L, kp);
    } else if (lr == rtp::kLightsRef) {
        auto kfn = disp ? k_lights_ref<true, false> : k_lights_ref<false, false>;
        hipLaunchKernelGGL(kfn, blocks, dim3(kBlock), ref_stack_lds(kp), c->stream, q, L, kp);
    } else if (accel) {
        const bool split = !mt && (c->shade_split ? c->shade_split == 2 : t->accel.st.item_ref.size() >= kShadeSplitItems);
        auto kfn = mt      ? (disp ? k_shade<true, false, true> : k_shade<true, false, false>)
                   : split ? (disp ? k_shade<false, true, true> : k_shade<false, true, false>)
                           : (disp ? k_shade<false, false, true> : k_shade<false, false, false>);
        hipLaunchKernelGGL(kfn, dim3((static_cast<unsigned>(n) + 63u) / 64u), dim3(64), lane_stack_lds(kp), c->stream,
                           accel_ptrs(t), t->mat, q, kp);
    } else {
        auto kfn = disp ? k_shade_ref<true> : k_shade_ref<false>;
        hipLaunchKernelGGL(kfn, dim3((static_cast<unsigned>(n) + kBlock - 1u) / kBlock), dim3(kBlock), ref_stack_lds(kp),
                           c->stream, q, kp);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The checks of rt_camera_rays and rt_camera_rays_host; no launch for an error.
int camera_rays_check(const rt_ctx* c, int width, int height, int y0, int rows, const void* out, bool device) {
    if (!c || width <= 0 || height <= 0 || rows <= 0 || y0 < 0 || static_cast<long long>(y0) + rows > height || !out ||
        static_cast<long long>(width) * rows >= (1ll << 31) || (device && reinterpret_cast<uintptr_t>(out) % 16 != 0))
        return RT_ERR_INVALID;
    if (!c->have_cam || !c->have_params) return RT_ERR_NO_SCENE;
    return RT_OK;
}

int camera_rays_launch(rt_ctx* c, int width, int height, int y0, int rows, float4* out) {
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    camera_params(c, kp);
    kp.width = width;
    kp.height = height;
    kp.y0 = y0;
    const unsigned n = static_cast<unsigned>(width) * static_cast<unsigned>(rows);
    hipLaunchKernelGGL(k_camera_rays, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, c->stream, kp, out, n);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

}  // namespace

extern "C" {

const char* rt_status_string(int s) {
    switch (s) {
        case RT_OK: return "ok";
        case RT_ERR_INVALID: return "invalid argument";
        case RT_ERR_DEVICE: return "HIP runtime error";
        case RT_ERR_NO_MEMORY: return "device allocation failed";
        case RT_ERR_NO_SCENE: return "scene, camera or light not uploaded";
        case RT_ERR_BVH: return "node/index arrays out of range or deeper than the 64-entry stack";
        case RT_ERR_NO_DEVICE: return "no such HIP device";
        case RT_ERR_COMM: return "RCCL call failed (the group's communicator is aborted)";
        case RT_ERR_TIMEOUT: return "timed out waiting for a group's frames (the communicator is aborted)";
        default: return "unknown status";
    }
}

int rt_create(rt_ctx** out, int device) { return rtx::create_ctx(out, device, nullptr); }

}  // extern "C"

hipError_t rtx::make_stream(hipStream_t* s, bool own_queue) {
    if (own_queue) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
            prop.multiProcessorCount > 0) {
            std::vector<uint32_t> mask((prop.multiProcessorCount + 31) / 32, 0xffffffffu);
            if (hipExtStreamCreateWithCUMask(s, static_cast<uint32_t>(mask.size()), mask.data()) == hipSuccess)
                return hipSuccess;
        }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

namespace {
bool env_cumask() {
    static const bool on = [] {
        const char* e = std::getenv("RT_STREAMS_CUMASK");
        return e && e[0] == '1';
    }();
    return on;
}
}  // namespace

int rtx::create_ctx(rt_ctx** out, int device, hipStream_t stream) {
    if (!out) return RT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RT_ERR_NO_DEVICE;
    rt_ctx* c = new (std::nothrow) rt_ctx();
    if (!c) return RT_ERR_NO_MEMORY;
    c->device = device;
    c->stream = stream;
    if (set_dev(c) != RT_OK || (!stream && rtx::make_stream(&c->stream, env_cumask()) != hipSuccess) ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc(&c->stats_dev, ST_COUNT * sizeof(unsigned long long)) != hipSuccess) {
        rt_destroy(c);
        return RT_ERR_DEVICE;
    }
    c->own_stream = !stream;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess)
            c->cu_count = prop.multiProcessorCount;
        if (c->cu_count <= 0) c->cu_count = 256;
    }
    c->ring0.resize(kRing, nullptr);
    c->ring1.resize(kRing, nullptr);
    for (int i = 0; i < kRing; ++i)
        if (hipEventCreate(&c->ring0[i]) != hipSuccess || hipEventCreate(&c->ring1[i]) != hipSuccess) {
            rt_destroy(c);
            return RT_ERR_DEVICE;
        }
    *out = c;
    return RT_OK;
}

bool rtx::matches_view(const rt_ctx* c, const FlatCamera& cam, const float lo[3], const float hi[3]) {
    if (!c || !c->have_cam || std::memcmp(&c->cam, &cam, sizeof cam) != 0) return false;
    if (c->N <= 0) return true;
    return std::memcmp(c->root_lo, lo, sizeof c->root_lo) == 0 && std::memcmp(c->root_hi, hi, sizeof c->root_hi) == 0;
}

int rtx::animate_deferred(rt_ctx* c, const FlatShape* shapes) {
    if (!c || !c->have_scene || c->anim_ids.empty() || !shapes) return RT_ERR_INVALID;
    const int n = static_cast<int>(c->anim_ids.size());
    // node records the host wrote before this frame apply first (as rt_animate): a refit
    // never carries both the host's node records and growth (k_refit's roles would both
    // write the grown boxes)
    if (c->nodes_dirty) {
        if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
        if (const int rc = flush_updates(c)) return rc;
    }
    if (c->grow_box.size() != 6 * static_cast<size_t>(n)) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const int id = c->anim_ids[i];
        c->host_shapes[id] = shapes[i];
        if (id < static_cast<int>(c->shape_moved.size())) c->shape_moved[id] = 1;
        // the growth of this frame, on the host with the device's operations
        // (reference_box: BoundingBox::growToInclude), unioned with the pending frames'
        float lo[3], hi[3];
        reference_box(shapes[i], lo, hi);
        float* b = &c->grow_box[6 * static_cast<size_t>(i)];
        for (int a = 0; a < 3; ++a) {
            b[a] = lo[a] < b[a] ? lo[a] : b[a];
            b[3 + a] = b[3 + a] < hi[a] ? hi[a] : b[3 + a];
        }
        const int e = c->refit_of[id];
        if (e >= 0 && e < static_cast<int>(c->entry_root.size()) && c->entry_root[e])
            for (int a = 0; a < 3; ++a) {
                c->root_lo[a] = lo[a] < c->root_lo[a] ? lo[a] : c->root_lo[a];
                c->root_hi[a] = c->root_hi[a] < hi[a] ? hi[a] : c->root_hi[a];
            }
    }
    c->grow_pending = true;
    // the sub-contexts follow as rt_animate makes them: brute force the records (no nodes),
    // Moller-Trumbore the same deferred frame
    if (c->brute && !c->brute_stale)
        for (int i = 0; i < n && !c->brute_stale; ++i)
            if (rt_update_shapes(c->brute, c->anim_ids[i], 1, &shapes[i]) != RT_OK) c->brute_stale = true;
    if (c->mtc && !c->mtc_stale && rtx::animate_deferred(c->mtc, shapes) != RT_OK) c->mtc_stale = true;
    return RT_OK;
}

bool rtx::view_root(const rt_ctx* c, float lo[3], float hi[3]) {
    if (!c || !c->have_scene || c->N <= 0) return false;
    std::memcpy(lo, c->root_lo, sizeof c->root_lo);
    std::memcpy(hi, c->root_hi, sizeof c->root_hi);
    return true;
}

extern "C" {

int rt_destroy(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID;
    hipSetDevice(c->device);
    if (c->stream) sync_stream(c);
    if (c->brute) rt_destroy(c->brute);  // it runs on this context's stream
    c->brute = nullptr;
    if (c->mtc) rt_destroy(c->mtc);
    c->mtc = nullptr;
    free_scene(c);
    hipFree(c->staging_shapes);
    hipFree(c->staging_nodes);
    hipFree(c->staging_idx);
    hipFree(c->img);
    hipFree(c->ss_buf);
    hipFree(c->ad_list);
    hipFree(c->ad_count);
    hipFree(c->stats_dev);
    hipFree(c->trace_in);
    hipFree(c->trace_hits);
    hipFree(c->gbuf_stage);
    hipFree(c->ao_stage);
    hipFree(c->shade_in);
    hipFree(c->shade_out);
    hipFree(c->tail_queue);
    hipFree(c->tail_counts);
    hipFree(c->tile_times);
    hipFree(c->tile_order);
    hipFree(c->sched_cost);
    hipFree(c->dil_cost);
    hipFree(c->heavy_acc);
    hipFree(c->sched_order);
    hipFree(c->sched_sets);
    hipFree(c->anim_maps);
    hipFree(c->anim_sbox);
    for (int k = 0; k < rt_ctx::kAnimRing; ++k) {
        if (c->anim_pinned[k]) hipHostFree(c->anim_pinned[k]);
        if (c->anim_copied[k]) hipEventDestroy(c->anim_copied[k]);
    }
    for (hipEvent_t e : c->ring0) if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->ring1) if (e) hipEventDestroy(e);
    if (c->sync_ev) hipEventDestroy(c->sync_ev);
    if (c->frame_ev) hipEventDestroy(c->frame_ev);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
    return RT_OK;
}

int rt_set_stream(rt_ctx* c, void* s) {
    if (!c) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    if (const int rc = record_mark(c)) return rc;  // on the stream the k_refit ran on
    HIP_TRY(sync_stream(c));
    if (c->own_stream) hipStreamDestroy(c->stream);
    if (s) {
        c->stream = static_cast<hipStream_t>(s);
        c->own_stream = false;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    for (rt_ctx* sub : {c->brute, c->mtc})  // sub-contexts run on this context's stream (synchronised above)
        if (sub) {
            rt_set_stream(sub, c->stream);
        }
    return RT_OK;
}

int rt_upload_scene(rt_ctx* c, const FlatShape* shapes, int S, const FlatNode* nodes, int N, const int* idx,
                    int I) {
    if (!c || S < 0 || N < 0 || I < 0 || (S > 0 && !shapes) || (N > 0 && !nodes) || (I > 0 && !idx))
        return RT_ERR_INVALID;
    int ms = 0;
    int rc = check_tree(nodes, N, idx, I, S, &ms);
    if (rc != RT_OK) return rc;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    PhaseLaps lap("rt_upload_scene");
    HIP_TRY(sync_stream(c));
    free_scene(c);  // (joins a rebuild in flight: it reads the host copies)
    lap("free");
    c->host_nodes.assign(nodes, nodes + N);
    c->host_idx.assign(idx, idx + I);
    c->host_shapes.assign(shapes, shapes + S);
    lap("host copies");
    // The accelerator's host build (from the host copies into c->accel, which nothing
    // else touches meanwhile) runs on its own thread while this one uploads and packs
    // the records: the build does not wait for the device, nor the copies for the build
    // (config 5: 64 -> 53 ms). Small scenes build afterwards on this thread as before (a
    // new thread's allocations start in a fresh heap arena: the car's upload 3.0 -> 3.5 ms).
    constexpr int kOverlapShapes = 32768;
    const bool overlap = N > 0 && S >= kOverlapShapes;
    bool built = false;
    std::thread builder;
    if (overlap)
        builder = std::thread([c, S, N, I, &built] {
            try {  // (bad_alloc: no accelerator, as a failed build; never past the thread)
                built = rta::build_accel(c->host_shapes.data(), S, c->host_nodes.data(), N, c->host_idx.data(), I,
                                         kLeafScan, kMaxStack, c->accel, c->build_mt);
            } catch (...) {
                c->accel = rta::AccelHost();
                built = false;
            }
        });
    const auto records = [&]() -> int {
        const size_t sS = S > 0 ? S : 1, sI = I > 0 ? I : 1, sN = N > 0 ? N : 1;
        if (hipMalloc(&c->geo_lin, sS * 5 * sizeof(float4)) != hipSuccess ||
            hipMalloc(&c->geo_leaf, sI * 5 * sizeof(float4)) != hipSuccess ||
            hipMalloc(&c->mat, sS * 2 * sizeof(float4)) != hipSuccess ||
            hipMalloc(&c->nodes, sN * 2 * sizeof(float4)) != hipSuccess)
            return RT_ERR_NO_MEMORY;
        int r2;
        if ((r2 = ensure_staging(c->staging_shapes, c->staging_shapes_cap, sS)) != RT_OK) return r2;
        if ((r2 = ensure_staging(c->staging_nodes, c->staging_nodes_cap, sN)) != RT_OK) return r2;
        if ((r2 = ensure_staging(c->staging_idx, c->staging_idx_cap, sI)) != RT_OK) return r2;
        if (S > 0) HIP_TRY(hipMemcpyAsync(c->staging_shapes, shapes, S * sizeof(FlatShape), hipMemcpyHostToDevice, c->stream));
        if (N > 0) HIP_TRY(hipMemcpyAsync(c->staging_nodes, nodes, N * sizeof(FlatNode), hipMemcpyHostToDevice, c->stream));
        if (I > 0) HIP_TRY(hipMemcpyAsync(c->staging_idx, idx, I * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (S + I > 0)
            hipLaunchKernelGGL(k_pack_shapes, dim3((S + I + 255) / 256), dim3(256), 0, c->stream, c->staging_shapes, S,
                               c->staging_idx, I, c->geo_lin, c->geo_leaf, c->mat);
        if (N > 0)
            hipLaunchKernelGGL(k_pack_nodes, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->staging_nodes, N,
                               c->nodes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(sync_stream(c));
        return RT_OK;
    };
    rc = records();
    if (builder.joinable()) builder.join();
    lap("records (build alongside)");
    if (rc != RT_OK) {
        free_scene(c);
        return rc;
    }
    c->S = S;
    c->N = N;
    c->I = I;
    c->max_stack = ms;
    c->have_scene = true;
    c->nodes_on_device_newer = false;
    set_root(c);
    c->anim_ids.clear();  // ids refer to the previous scene
    c->refit_ids.clear();
    c->anim_base.clear();
    c->upd_ids.clear();
    c->upd_base.clear();
    c->upd_mark.assign(S, 0);
    c->nodes_dirty = c->nodes_rebuild = c->bounds_rebuild = false;
    c->brute_stale = c->mtc_stale = true;
    rc = upload_accel(c, overlap ? &built : nullptr);
    lap("accelerator");
    return rc;
}

int rt_update_shapes(rt_ctx* c, int first, int count, const FlatShape* shapes) {
    if (!c || !c->have_scene || first < 0 || count < 0 || first > c->S - count || (count > 0 && !shapes))
        return RT_ERR_INVALID;
    if (count == 0) return RT_OK;
    // glBufferSubData of shape records (updateScene, src/main.cpp:981-992): the host copy
    // now, the device copies at the next operation that reads them (flush_updates), as
    // one refit with whatever else was written by then. The host array may be reused
    // when this returns. Node boxes stay as they are until rt_update_nodes.
    for (int j = 0; j < count; ++j) {
        const int id = first + j;
        if (!c->upd_mark[id]) {
            if (c->refit_of[id] < 0) c->upd_base.emplace_back(id, c->host_shapes[id]);  // the build's record
            c->upd_mark[id] = 1;
            c->upd_ids.push_back(id);
        }
        c->host_shapes[id] = shapes[j];
        if (id < static_cast<int>(c->shape_moved.size())) c->shape_moved[id] = 1;
    }
    // the sub-contexts hold the same shapes in the same order (brute: under its one
    // leaf; mtc: the MT accelerator): they refit too
    if (c->brute && !c->brute_stale && rt_update_shapes(c->brute, first, count, shapes) != RT_OK)
        c->brute_stale = true;
    if (c->mtc && !c->mtc_stale && rt_update_shapes(c->mtc, first, count, shapes) != RT_OK) c->mtc_stale = true;
    return RT_OK;
}

int rt_update_nodes(rt_ctx* c, const FlatNode* nodes, int N) {
    if (!c || !c->have_scene || N != c->N || (N > 0 && !nodes)) return RT_ERR_INVALID;
    if (c->grow_pending) {  // deferred growth (rtx::animate_deferred) applies before these records
        if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
        if (const int rc = flush_updates(c)) return rc;
    }
    for (int k = 0; k < N; ++k) {
        const FlatNode &a = nodes[k], &b = c->host_nodes[k];
        if (a.leftChild != b.leftChild || a.rightChild != b.rightChild ||
            (a.leftChild == -1 && (a.startShapeIdx != b.startShapeIdx || a.numShapes != b.numShapes)))
            return RT_ERR_BVH;  // topology must not change: use rt_upload_scene
    }
    if (N == 0) return RT_OK;
    // glBufferSubData of the node records (src/main.cpp:340-345): the host copy now,
    // every device copy of the boxes at the next device operation (flush_updates).
    c->host_nodes.assign(nodes, nodes + N);
    c->nodes_on_device_newer = false;  // these boxes replace any the device grew
    set_root(c);
    c->nodes_dirty = true;
    c->boxes_finite = 1;
    for (int k = 0; k < N; ++k)
        for (float v : {nodes[k].boundsMin.x, nodes[k].boundsMin.y, nodes[k].boundsMin.z, nodes[k].boundsMax.x,
                        nodes[k].boundsMax.y, nodes[k].boundsMax.z})
            if (std::isnan(v)) c->boxes_finite = 0;
    // the scene tree holds only while the boxes nest (accel.h SceneTree)
    // (recomputed per call: a later write that restores nesting before the flush
    // cancels the rebuild an earlier one asked for)
    c->nodes_rebuild = c->accel_ok && c->accel.st.wroot >= 0 && !host_nodes_nest(c);
    if (c->mtc && !c->mtc_stale && rt_update_nodes(c->mtc, nodes, N) != RT_OK) c->mtc_stale = true;
    return RT_OK;
}

int rt_set_animated(rt_ctx* c, const int* ids, int count) {
    if (!c || !c->have_scene || count < 0 || (count > 0 && !ids)) return RT_ERR_INVALID;
    std::vector<char> seen(c->S, 0);
    for (int i = 0; i < count; ++i) {
        if (ids[i] < 0 || ids[i] >= c->S || seen[ids[i]]) return RT_ERR_INVALID;
        seen[ids[i]] = 1;
    }
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    if (c->grow_pending) {  // deferred frames of the old set first (rtx::animate_deferred)
        const int rc = flush_updates(c);
        if (rc != RT_OK) return rc;
    }
    c->anim_ids.assign(ids, ids + count);
    c->grow_box.assign(6 * static_cast<size_t>(count), 0.f);
    for (int i = 0; i < count; ++i)
        for (int a = 0; a < 3; ++a) {
            c->grow_box[6 * i + a] = INFINITY;
            c->grow_box[6 * i + 3 + a] = -INFINITY;
        }
    // The refit set takes the new ids with the records the accelerator was built from
    // (a shape rewritten since: its record before the first rewrite); shapes already in
    // it keep their base, and shapes that stop being animated stay in it.
    bool added = false;
    for (int i = 0; i < count; ++i) {
        const int id = ids[i];
        if (c->refit_of[id] >= 0) continue;
        FlatShape base = c->host_shapes[id];
        if (c->upd_mark[id])
            for (const auto& ub : c->upd_base)
                if (ub.first == id) base = ub.second;
        c->refit_of[id] = static_cast<int>(c->refit_ids.size());
        c->refit_ids.push_back(id);
        c->anim_base.push_back(base);
        added = true;
    }
    if (c->mtc && !c->mtc_stale && rt_set_animated(c->mtc, ids, count) != RT_OK) c->mtc_stale = true;
    return added ? prepare_animation(c) : RT_OK;
}

int rt_animate(rt_ctx* c, const FlatShape* shapes) {
    if (!c || !c->have_scene || c->anim_ids.empty() || !shapes) return RT_ERR_INVALID;
    PhaseLaps lap(c->rebuild && c->rebuild->done.load() ? "rt_animate (swap)" : nullptr);
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    int rc = RT_OK;
    if (c->grow_pending) {  // deferred frames pending (rtx::animate_deferred): this one joins them
        if ((rc = rtx::animate_deferred(c, shapes)) != RT_OK) return rc;
        return flush_updates(c);
    }
    // node records the host wrote before this frame apply first, then this frame's growth
    if (c->nodes_dirty && (rc = flush_updates(c)) != RT_OK) return rc;
    const int n = static_cast<int>(c->anim_ids.size());
    for (int i = 0; i < n; ++i) c->host_shapes[c->anim_ids[i]] = shapes[i];
    for (int i = 0; i < n; ++i)
        if (c->anim_ids[i] < static_cast<int>(c->shape_moved.size())) c->shape_moved[c->anim_ids[i]] = 1;
    // the root's box as k_refit grows it (grow_node: glm::min / max of the listed
    // shapes' growToInclude boxes), for rtx::view_root
    for (int i = 0; i < n; ++i) {
        const int e = c->refit_of[c->anim_ids[i]];
        if (e < 0 || e >= static_cast<int>(c->entry_root.size()) || !c->entry_root[e]) continue;
        float lo[3], hi[3];
        reference_box(shapes[i], lo, hi);
        for (int a = 0; a < 3; ++a) {
            c->root_lo[a] = lo[a] < c->root_lo[a] ? lo[a] : c->root_lo[a];
            c->root_hi[a] = c->root_hi[a] < hi[a] ? hi[a] : c->root_hi[a];
        }
    }
    if (c->brute && !c->brute_stale)  // the brute-force context: the same records, no nodes to grow
        for (int i = 0; i < n && !c->brute_stale; ++i)
            if (rt_update_shapes(c->brute, c->anim_ids[i], 1, &shapes[i]) != RT_OK) c->brute_stale = true;
    // the MT context: the same frame, its nodes grown the same way (its set follows c's)
    if (c->mtc && !c->mtc_stale && rt_animate(c->mtc, shapes) != RT_OK) c->mtc_stale = true;
    lap("host records");
    // the records and the growth on the device (one k_refit launch); a host rebuild
    // only after a bound changed kind
    rc = flush_updates(c, true);
    lap("flush");
    return rc;
}

int rt_build_lbvh(rt_ctx* c, float* device_ms) {
    if (!c || !c->have_scene) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    if (const int rc0 = flush_updates(c)) return rc0;  // staging_shapes current
    const int S = c->S;
    const int N = S > 0 ? 2 * S - 1 : 0;
    std::vector<FlatNode> nodes(static_cast<size_t>(N));
    std::vector<int> idx(static_cast<size_t>(S));
    float ms = 0.f;
    if (S > 0) {
        FlatNode* dn = nullptr;
        int* di = nullptr;
        if (hipMalloc(&dn, N * sizeof(FlatNode)) != hipSuccess || hipMalloc(&di, S * sizeof(int)) != hipSuccess) {
            (void)hipFree(dn);
            return RT_ERR_NO_MEMORY;
        }
        // staging_shapes holds the current records (uploads, updates and rt_animate frames)
        int rc = rtl::lbvh_build(c->staging_shapes, S, dn, di, c->stream, &ms) == 0 ? RT_OK : RT_ERR_DEVICE;
        if (rc == RT_OK &&
            (hipMemcpyAsync(nodes.data(), dn, N * sizeof(FlatNode), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
             hipMemcpyAsync(idx.data(), di, S * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
             sync_stream(c) != hipSuccess))
            rc = RT_ERR_DEVICE;
        (void)hipFree(dn);
        (void)hipFree(di);
        if (rc != RT_OK) return rc;
    }
    if (device_ms) *device_ms = ms;
    // adopt the tree exactly as if the host had uploaded it (validation, leaf
    // order, accelerator); the animated set is cleared as by any upload
    const std::vector<FlatShape> shapes(c->host_shapes);
    return rt_upload_scene(c, shapes.data(), S, nodes.data(), N, idx.data(), S);
}

int rt_scene_size(rt_ctx* c, int* num_shapes, int* num_nodes, int* num_indices) {
    if (!c || !c->have_scene) return RT_ERR_INVALID;
    if (num_shapes) *num_shapes = c->S;
    if (num_nodes) *num_nodes = c->N;
    if (num_indices) *num_indices = c->I;
    return RT_OK;
}

int rt_read_indices(rt_ctx* c, int* indices, int num_indices) {
    if (!c || !c->have_scene || num_indices != c->I || (num_indices > 0 && !indices)) return RT_ERR_INVALID;
    std::copy(c->host_idx.begin(), c->host_idx.end(), indices);
    return RT_OK;
}

int rt_read_nodes(rt_ctx* c, FlatNode* nodes, int N) {
    if (!c || !c->have_scene || N != c->N || (N > 0 && !nodes)) return RT_ERR_INVALID;
    if (N == 0) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    if (const int rc = flush_updates(c)) return rc;
    HIP_TRY(hipMemcpyAsync(nodes, c->staging_nodes, N * sizeof(FlatNode), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

int rt_set_camera(rt_ctx* c, const FlatCamera* cam) {
    if (!c || !cam) return RT_ERR_INVALID;
    c->cam = *cam;
    c->have_cam = true;
    return RT_OK;
}

int rt_set_light(rt_ctx* c, const FlatLight* l) { return rt_set_lights(c, l, 1); }

int rt_set_lights(rt_ctx* c, const FlatLight* lights, int count) {
    if (!c || !lights || count < 1 || count > RT_MAX_LIGHTS) return RT_ERR_INVALID;
    for (int i = 0; i < RT_MAX_LIGHTS; ++i) c->lights[i] = i < count ? lights[i] : FlatLight{};
    c->light = c->lights[0];
    c->nlights = count;
    c->have_light = true;
    return RT_OK;
}

int rt_get_lights(rt_ctx* c, FlatLight* lights, int cap, int* count) {
    if (!c || (lights && cap < 0)) return RT_ERR_INVALID;
    const int n = c->have_light ? c->nlights : 0;
    if (lights)
        for (int i = 0; i < std::min(cap, n); ++i) lights[i] = c->lights[i];
    if (count) *count = n;
    return RT_OK;
}

int rt_set_soft_shadows(rt_ctx* c, const float* radii, int count, int samples) {
    if (!c || count < 0 || count > RT_MAX_LIGHTS) return RT_ERR_INVALID;
    if (count > 0) {
        if (!radii || samples < 1 || samples > RT_MAX_SHADOW_SAMPLES) return RT_ERR_INVALID;
        for (int i = 0; i < count; ++i)
            if (!std::isfinite(radii[i]) || radii[i] < 0.0f) return RT_ERR_INVALID;
    }
    for (int i = 0; i < RT_MAX_LIGHTS; ++i) c->soft_radii[i] = i < count ? radii[i] : 0.0f;
    c->soft_count = count;
    c->soft_samples = count > 0 ? samples : 0;
    return RT_OK;
}

int rt_get_soft_shadows(rt_ctx* c, float* radii, int cap, int* count, int* samples) {
    if (!c || (radii && cap < 0)) return RT_ERR_INVALID;
    if (radii)
        for (int i = 0; i < std::min(cap, c->soft_count); ++i) radii[i] = c->soft_radii[i];
    if (count) *count = c->soft_count;
    if (samples) *samples = c->soft_samples;
    return RT_OK;
}

int rt_set_params(rt_ctx* c, const rt_params* p) {
    if (!c || !p || p->maxBounces < 0) return RT_ERR_INVALID;
    c->params = *p;
    c->have_params = true;
    return RT_OK;
}

int rt_set_kernel(rt_ctx* c, int kernel) {
    if (!c || kernel < RT_KERNEL_AUTO || kernel > RT_KERNEL_ACCEL) return RT_ERR_INVALID;
    c->kernel = kernel;
    return RT_OK;
}

int rt_dispatch_rows(rt_ctx* c, int width, int height, int y0, int stripe, int step, int out_rows, float* dst,
                     size_t pitch) {
    return rt_dispatch_rows_fmt(c, width, height, y0, stripe, step, out_rows, dst, pitch, RT_FORMAT_RGBA32F);
}

// period = stripe * step, refused when it does not fit an int
static int stripe_period(int stripe, int step) {
    if (stripe <= 0 || step <= 0 || step > INT_MAX / stripe) return -1;
    return stripe * step;
}

int rt_dispatch_rows_fmt(rt_ctx* c, int width, int height, int y0, int stripe, int step, int out_rows, float* dst,
                         size_t pitch, int format) {
    return rt_dispatch_rows_ex(c, width, height, y0, stripe, stripe_period(stripe, step), out_rows, dst, pitch,
                               format);
}

int rt_dispatch_rows_ex(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows, float* dst,
                        size_t pitch, int format) {
    if (!c) return RT_ERR_INVALID;
    KParams kp;
    const int n = c->samples;
    if (n > 1) {
        // rt_set_samples: the sample frame is the same mapping with every extent times n.
        // Refused before anything is launched when it breaks a limit of the one-sample
        // dispatch: an int overflows, more than 65535 tile rows, width * rows >= 2^32.
        const long long lim = INT_MAX / n;
        if (width > lim || height > lim || y0 > lim || stripe > lim || period > lim || out_rows > lim ||
            width < 0 || height < 0 || y0 < 0 || stripe < 0 || period < 0 || out_rows < 0)
            return RT_ERR_INVALID;
        if (width > 0 && out_rows > 0 &&
            ((static_cast<long long>(out_rows) * n + kTileH - 1) / kTileH > 65535 ||
             static_cast<unsigned long long>(width) * n * (static_cast<unsigned long long>(out_rows) * n) >=
                 (1ull << 32)))
            return RT_ERR_INVALID;
    }
    int rc = fill_kparams(c, width * n, height * n, y0 * n, stripe * n, period * n, out_rows * n, dst, pitch, kp,
                          format, n);
    if (rc != RT_OK) return rc;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    return render(c, kp);
}

int rt_set_samples(rt_ctx* c, int n) {
    if (!c || (n != 1 && n != 2 && n != 4 && n != 8)) return RT_ERR_INVALID;
    c->samples = n;
    return RT_OK;
}

int rt_set_adaptive(rt_ctx* c, float threshold) {
    if (!c || threshold != threshold) return RT_ERR_INVALID;  // NaN: the setting stays
    c->adaptive = threshold < 0.0f ? -1.0f : threshold;
    return RT_OK;
}

int rt_adaptive_stats(rt_ctx* c, uint64_t* refined, uint64_t* pixels) {
    if (!c || !c->ad_from) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    HIP_TRY(sync_stream(c));  // the sub-contexts (brute, mtc) render on this stream
    unsigned n = 0;
    HIP_TRY(hipMemcpy(&n, c->ad_from->ad_count, sizeof n, hipMemcpyDeviceToHost));
    if (refined) *refined = n;
    if (pixels) *pixels = c->ad_from->ad_pixels;
    return RT_OK;
}

int rt_dispatch(rt_ctx* c, int width, int height, int y0, int y1) {
    if (!c || width <= 0 || height <= 0 || y0 < 0 || y1 > height || y0 > y1) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    if (width != c->img_w || height != c->img_h || c->surf_fmt != c->img_fmt || !c->img) {
        HIP_TRY(sync_stream(c));
        hipFree(c->img);
        c->img = nullptr;
        c->img_w = c->img_h = 0;
        size_t pitch = 0;
        const size_t row = static_cast<size_t>(width) * format_bytes(c->surf_fmt);
        if (hipMallocPitch(reinterpret_cast<void**>(&c->img), &pitch, row, height) != hipSuccess)
            return RT_ERR_NO_MEMORY;
        HIP_TRY(hipMemset2DAsync(c->img, pitch, 0, row, height, c->stream));
        c->img_pitch = pitch;
        c->img_w = width;
        c->img_h = height;
        c->img_fmt = c->surf_fmt;
    }
    return rt_dispatch_rows_fmt(c, width, height, y0, 1, 1, y1 - y0,
                                reinterpret_cast<float*>(reinterpret_cast<char*>(c->img) + y0 * c->img_pitch),
                                c->img_pitch, c->img_fmt);
}

int rt_set_surface_format(rt_ctx* c, int format) {
    if (!c || (format != RT_FORMAT_RGBA32F && format != RT_FORMAT_RGBA8 && format != RT_FORMAT_SRGBA8 &&
               format != RT_FORMAT_RGBA16F))
        return RT_ERR_INVALID;
    c->surf_fmt = format;
    return RT_OK;
}

int rt_surface_format(rt_ctx* c, int* format) {
    if (!c || !format) return RT_ERR_INVALID;
    *format = c->surf_fmt;
    return RT_OK;
}

int rt_srgb_thresholds(float* out255) {
    static const float t[255] = {RT_SRGB_THRESHOLDS};
    if (!out255) return RT_ERR_INVALID;
    std::memcpy(out255, t, sizeof t);
    return RT_OK;
}

int rt_sync(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    // A host that waits for every frame (the reference's loop, src/main.cpp:290-462)
    // waits ~0.25 ms per frame: poll back to back (yielding the core) for the first
    // rtg::kSpinMs, then nap between polls (csrc/group_wait.h). The poll is on an event
    // recorded behind the stream's work, not on the stream: hipStreamQuery saw an empty
    // kernel end 15.2 us after its launch, the event 10.7 us (and 247.3 against 245.8 us
    // for a 235-us kernel; tools/native/wait_probe.hip, profiles/r04_wait_probe.txt). No
    // deadline: a single context has no peer to wait on.
    if (!c->sync_ev && hipEventCreateWithFlags(&c->sync_ev, hipEventDisableTiming) != hipSuccess) return RT_ERR_DEVICE;
    HIP_TRY(hipEventRecord(c->sync_ev, c->stream));
    const hipEvent_t ev = c->sync_ev;
    const rtg::WaitResult w = rtg::wait_bounded(
        [ev] {
            const hipError_t e = hipEventQuery(ev);
            return e == hipSuccess ? 0 : (e == hipErrorNotReady ? 1 : -1);
        },
        [] { return false; }, 0.0);
    if (w != rtg::kWaitDone) return RT_ERR_DEVICE;
    for (rt_ctx* x : {c, c->brute, c->mtc})  // the sub-contexts run on this stream
        if (x) stream_drained(x);
    return RT_OK;
}

int rt_sync_frame(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID;
    // The last dispatch's frame ended at frame_ev if its launch recorded one (a latency-mode
    // cost frame, before the cost order's kernels) and no refit slot was taken since;
    // otherwise (and for work enqueued after the dispatch) the whole stream, as rt_sync.
    rt_ctx* t = c->frame_from;
    const bool known = t && (t == c || t == c->brute || t == c->mtc || (c->brute && t == c->brute->mtc) ||
                             (c->mtc && t == c->mtc->brute));
    if (!known || !t->frame_ev_set || !t->frame_ev || refit_launches(c) != c->frame_refits) return rt_sync(c);
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    const hipEvent_t ev = t->frame_ev;
    const rtg::WaitResult w = rtg::wait_bounded(
        [ev] {
            const hipError_t e = hipEventQuery(ev);
            return e == hipSuccess ? 0 : (e == hipErrorNotReady ? 1 : -1);
        },
        [] { return false; }, 0.0);
    if (w != rtg::kWaitDone) return RT_ERR_DEVICE;
    // every refit slot in use was taken before the frame's render (none since): free
    for (rt_ctx* x : {c, c->brute, c->mtc})
        if (x) stream_drained(x);
    return RT_OK;
}

int rt_read_surface(rt_ctx* c, void* dst, size_t pitch, int width, int height) {
    if (!c || !dst || !c->img || width != c->img_w || height != c->img_h) return RT_ERR_INVALID;
    const size_t row = static_cast<size_t>(c->img_w) * format_bytes(c->img_fmt);
    if (pitch < row) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    HIP_TRY(hipMemcpy2DAsync(dst, pitch, c->img, c->img_pitch, row, c->img_h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

int rt_read_image(rt_ctx* c, float* dst, size_t pitch, int width, int height) {
    if (!c || c->img_fmt != RT_FORMAT_RGBA32F) return RT_ERR_INVALID;
    return rt_read_surface(c, dst, pitch, width, height);
}

int rt_device_image(rt_ctx* c, void** p, size_t* pitch) {
    if (!c || !p || !pitch || !c->img) return RT_ERR_INVALID;
    *p = c->img;
    *pitch = c->img_pitch;
    return RT_OK;
}

int rt_collect_stats(rt_ctx* c, int width, int height, int y0, int stripe, int step, int out_rows, rt_stats* out) {
    return rt_collect_stats_ex(c, width, height, y0, stripe, stripe_period(stripe, step), out_rows, out);
}

int rt_collect_stats_ex(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows,
                        rt_stats* out) {
    if (!c || !out) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    // The counting kernel needs a destination; use a scratch surface.
    float* scratch = nullptr;
    const size_t pitch = static_cast<size_t>(width > 0 ? width : 1) * 16;
    if (hipMalloc(&scratch, pitch * static_cast<size_t>(out_rows > 0 ? out_rows : 1)) != hipSuccess)
        return RT_ERR_NO_MEMORY;
    KParams kp;
    int rc = fill_kparams(c, width, height, y0, stripe, period, out_rows, scratch, pitch, kp);
    if (rc == RT_OK) {
        kp.stats = c->stats_dev;
        if (hipMemsetAsync(c->stats_dev, 0, ST_COUNT * sizeof(unsigned long long), c->stream) != hipSuccess)
            rc = RT_ERR_DEVICE;
        if (rc == RT_OK) rc = launch(c, kp, true);
        unsigned long long h[ST_COUNT];
        if (rc == RT_OK && (hipMemcpyAsync(h, c->stats_dev, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                            sync_stream(c) != hipSuccess))
            rc = RT_ERR_DEVICE;
        if (rc == RT_OK) {
            out->pixels = h[ST_PIXELS];
            out->closest_rays = h[ST_CLOSEST];
            out->shadow_rays = h[ST_SHADOW];
            out->node_visits = h[ST_NODES];
            for (int i = 0; i < 4; ++i) {
                out->bvh_tests[i] = h[ST_BVH0 + i];
                out->brute_tests[i] = h[ST_BR0 + i];
            }
            out->closest_updates = h[ST_UPD];
            out->hits = h[ST_HITS];
        }
    }
    sync_stream(c);
    hipFree(scratch);
    return rc;
}

int rt_kernel_times(rt_ctx* c, float* ms, int cap) {
    if (!c || (cap > 0 && !ms) || cap < 0) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    const int n = c->ring_used;
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipEventSynchronize(c->ring1[i]));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, c->ring0[i], c->ring1[i]));
        if (i < cap) ms[i] = t;
    }
    c->ring_used = 0;
    return n;
}

int rt_last_kernel_ms(rt_ctx* c, float* ms) {
    if (!c || !ms || !c->timed) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    HIP_TRY(hipEventSynchronize(c->last1));
    HIP_TRY(hipEventElapsedTime(ms, c->last0, c->last1));
    return RT_OK;
}

int rt_trace_rays(rt_ctx* c, const rt_ray* dev_rays, int n, rt_hit* dev_hits, int mode) {
    bool run;
    if (const int rc = trace_check(c, dev_rays, n, dev_hits, mode, &run)) return rc;
    if (!run) return RT_OK;
    if (reinterpret_cast<uintptr_t>(dev_rays) % 16 != 0 || reinterpret_cast<uintptr_t>(dev_hits) % 16 != 0)
        return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    return trace_launch(c, reinterpret_cast<const float4*>(dev_rays), nullptr, n, reinterpret_cast<float4*>(dev_hits),
                        mode);
}

int rt_trace_rays_host(rt_ctx* c, const rt_ray* rays, int n, rt_hit* hits, int mode) {
    bool run;
    if (const int rc = trace_check(c, rays, n, hits, mode, &run)) return rc;
    return run ? trace_staged(c, rays, sizeof(rt_ray), false, n, hits, mode) : RT_OK;
}

int rt_trace_pixels(rt_ctx* c, int width, int height, const int* xy, int n, rt_hit* hits) {
    bool run;
    if (const int rc = trace_check(c, xy, n, hits, RT_TRACE_CLOSEST, &run)) return rc;
    if (!c->have_cam || !c->have_params) return RT_ERR_NO_SCENE;
    if (width <= 0 || height <= 0) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (xy[2 * i] < 0 || xy[2 * i] >= width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= height) return RT_ERR_INVALID;
    return run ? trace_staged(c, xy, 2 * sizeof(int), true, n, hits, RT_TRACE_CLOSEST) : RT_OK;
}

int rt_dispatch_gbuffer(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows,
                        const rt_gbuffer* out) {
    bool run;
    if (const int rc = gbuffer_check(c, width, height, y0, stripe, period, out_rows, out, &run)) return rc;
    if (!run) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    return gbuffer_launch(c, width, height, y0, stripe, period, out_rows, *out);
}

int rt_gbuffer_host(rt_ctx* c, int width, int height, const rt_gbuffer* host_out) {
    bool run;
    if (const int rc = gbuffer_check(c, width, height, 0, 1, 1, height, host_out, &run)) return rc;
    if (!run) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    // the wanted planes side by side in the staging buffer, rows packed (every offset a multiple of 16 B)
    const size_t px = static_cast<size_t>(width) * static_cast<size_t>(height);
    const size_t small16 = (px * 4 + 15) / 16;
    const size_t need = (host_out->shape ? small16 : 0) + (host_out->depth ? small16 : 0) +
                        (host_out->normal ? px : 0) + (host_out->position ? px : 0);
    if (const int rc = ensure_staging(c->gbuf_stage, c->gbuf_stage_cap, need)) return rc;
    float4* at = c->gbuf_stage;
    rt_gbuffer dev{};
    const size_t w4 = static_cast<size_t>(width) * 4, w16 = static_cast<size_t>(width) * 16;
    if (host_out->shape) dev.shape = reinterpret_cast<int*>(at), dev.shape_pitch = w4, at += small16;
    if (host_out->depth) dev.depth = reinterpret_cast<float*>(at), dev.depth_pitch = w4, at += small16;
    if (host_out->normal) dev.normal = reinterpret_cast<float*>(at), dev.normal_pitch = w16, at += px;
    if (host_out->position) dev.position = reinterpret_cast<float*>(at), dev.position_pitch = w16, at += px;
    if (const int rc = gbuffer_launch(c, width, height, 0, 1, 1, height, dev)) return rc;
    const struct {
        void* dst;
        size_t dpitch;
        const void* src;
        size_t row;
    } copies[4] = {{host_out->shape, host_out->shape_pitch, dev.shape, w4},
                   {host_out->depth, host_out->depth_pitch, dev.depth, w4},
                   {host_out->normal, host_out->normal_pitch, dev.normal, w16},
                   {host_out->position, host_out->position_pitch, dev.position, w16}};
    for (const auto& cp : copies)
        if (cp.dst)
            HIP_TRY(hipMemcpy2DAsync(cp.dst, cp.dpitch, cp.src, cp.row, cp.row, static_cast<size_t>(height),
                                     hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

int rt_dispatch_ao(rt_ctx* c, int width, int height, int y0, int stripe, int period, int out_rows,
                   const rt_ao_params* params, const rt_ao* out) {
    bool run;
    if (const int rc = ao_check(c, width, height, y0, stripe, period, out_rows, params, out, &run)) return rc;
    if (!run) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    return ao_launch(c, width, height, y0, stripe, period, out_rows, *params, *out);
}

int rt_ao_host(rt_ctx* c, int width, int height, const rt_ao_params* params, const rt_ao* host_out) {
    bool run;
    if (const int rc = ao_check(c, width, height, 0, 1, 1, height, params, host_out, &run)) return rc;
    if (!run) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    // visibility first (4-byte rows), then count, rows packed
    const size_t px = static_cast<size_t>(width) * static_cast<size_t>(height);
    const size_t need = (host_out->visibility ? px : 0) + (host_out->count ? (px + 3) / 4 : 0);
    if (const int rc = ensure_staging(c->ao_stage, c->ao_stage_cap, need)) return rc;
    rt_ao dev{};
    const size_t w1 = static_cast<size_t>(width), w4 = w1 * 4;
    float* at = c->ao_stage;
    if (host_out->visibility) dev.visibility = at, dev.visibility_pitch = w4, at += px;
    if (host_out->count) dev.count = reinterpret_cast<uint8_t*>(at), dev.count_pitch = w1;
    if (const int rc = ao_launch(c, width, height, 0, 1, 1, height, *params, dev)) return rc;
    if (host_out->visibility)
        HIP_TRY(hipMemcpy2DAsync(host_out->visibility, host_out->visibility_pitch, dev.visibility, w4, w4,
                                 static_cast<size_t>(height), hipMemcpyDeviceToHost, c->stream));
    if (host_out->count)
        HIP_TRY(hipMemcpy2DAsync(host_out->count, host_out->count_pitch, dev.count, w1, w1,
                                 static_cast<size_t>(height), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

int rt_ao_table(float* dirs64x3, float* rot16x2) {
    static const float d[64 * 3] = {RT_AO_DIRS};
    static const float r[16 * 2] = {RT_AO_ROT};
    if (dirs64x3) std::memcpy(dirs64x3, d, sizeof d);
    if (rot16x2) std::memcpy(rot16x2, r, sizeof r);
    return RT_OK;
}

int rt_shade_rays(rt_ctx* c, const rt_view_ray* dev_rays, int n, void* dev_pixels, int format) {
    bool run;
    if (const int rc = shade_check(c, dev_rays, n, dev_pixels, format, true, &run)) return rc;
    if (!run) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    return shade_launch(c, reinterpret_cast<const float4*>(dev_rays), n, dev_pixels, format);
}

int rt_shade_rays_host(rt_ctx* c, const rt_view_ray* rays, int n, void* pixels, int format) {
    bool run;
    if (const int rc = shade_check(c, rays, n, pixels, format, false, &run)) return rc;
    if (!run) return RT_OK;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    const size_t bytes = static_cast<size_t>(n) * format_bytes(format);
    int rc = ensure_staging(c->shade_in, c->shade_in_cap, 2 * static_cast<size_t>(n));
    if (rc == RT_OK) rc = ensure_staging(c->shade_out, c->shade_out_cap, (bytes + 15) / 16);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->shade_in, rays, static_cast<size_t>(n) * sizeof(rt_view_ray), hipMemcpyHostToDevice,
                           c->stream));
    if ((rc = shade_launch(c, c->shade_in, n, c->shade_out, format)) != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pixels, c->shade_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

int rt_camera_rays(rt_ctx* c, int width, int height, int y0, int rows, rt_view_ray* dev_rays) {
    if (const int rc = camera_rays_check(c, width, height, y0, rows, dev_rays, true)) return rc;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    return camera_rays_launch(c, width, height, y0, rows, reinterpret_cast<float4*>(dev_rays));
}

int rt_camera_rays_host(rt_ctx* c, int width, int height, int y0, int rows, rt_view_ray* rays) {
    if (const int rc = camera_rays_check(c, width, height, y0, rows, rays, false)) return rc;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(rows);
    // the rays' own staging buffer: a host may shade the list it just generated
    if (const int rc = ensure_staging(c->shade_in, c->shade_in_cap, 2 * n)) return rc;
    if (const int rc = camera_rays_launch(c, width, height, y0, rows, c->shade_in)) return rc;
    HIP_TRY(hipMemcpyAsync(rays, c->shade_in, n * sizeof(rt_view_ray), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream(c));
    return RT_OK;
}

}  // extern "C"

extern "C" int rt_accel_info_get(rt_ctx* c, rt_accel_info* out) {
    if (!c || !out) return RT_ERR_INVALID;
    // the accelerator the next dispatch uses: pending updates applied first (a flush may rebuild it)
    if (c->have_scene) {
        if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
        if (const int rc = flush_updates(c)) return rc;
    }
    out->built = c->accel_ok ? 1 : 0;
    out->local_nodes = static_cast<int>(c->accel.lbox.size());
    out->local_leaves = c->accel.local_leaves;
    out->bounded_prims = c->accel.bounded_prims;
    out->always_prims = c->accel.always_prims;
    out->max_stack = c->accel.max_stack;
    out->last_kernel = c->last_kind;
    out->scene_tree = c->accel_ok && c->st_root != kNoChild ? 1 : 0;
    out->scene_nodes = static_cast<int>(c->accel.st.wchild.size() / rta::kWide);
    out->scene_items = static_cast<int>(c->accel.st.item_ref.size());
    out->scene_height = c->accel.st.height;
    out->tree_nested = c->accel.st.nested;
    out->record_bytes = c->accel_ok ? static_cast<int>(std::min<size_t>(c->record_bytes, 0x7fffffff)) : 0;
    return RT_OK;
}

extern "C" int rt_set_tree(rt_ctx* c, int mode) {
    if (!c || (mode != RT_TREE_REFERENCE && mode != RT_TREE_SCENE)) return RT_ERR_INVALID;
    c->tree_mode = mode;
    return RT_OK;
}

extern "C" int rt_debug_anim_rebuilds(rt_ctx* c) { return c ? c->anim_rebuilds : -1; }
extern "C" int rt_debug_refits(rt_ctx* c) { return c ? c->updates_flushed : -1; }
// Diagnostics: how flush_updates launches the refit (RefitArgs: 0 one launch whose box
// roles wait for the record role, 1 two launches, 2 one launch deriving every box from
// the records). Same device state either way.
// out[7]: dirty slots, their largest and total prim range, reference nodes listing an
// entry, refit entries, bytes of the last flush's pinned records, compactions
// Diagnostics: the rebuild a refit asks for runs on a host thread (1, default) or in that
// refit's flush (0). rt_debug_rebuild_state: out[0] a rebuild is running, out[1] rebuilds
// asked for, out[2] rebuilt accelerators swapped in, out[3] the scene tree is suspended.
extern "C" int rt_debug_async_rebuild(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID;
    c->async_rebuild = on ? 1 : 0;
    return RT_OK;
}
extern "C" int rt_debug_rebuild_state(rt_ctx* c, int* out) {
    if (!c || !out) return RT_ERR_INVALID;
    out[0] = c->rebuild ? 1 : 0;
    out[1] = c->anim_rebuilds;
    out[2] = c->async_swaps;
    out[3] = c->st_suspended ? 1 : 0;
    return RT_OK;
}

extern "C" int rt_debug_refit_stats(rt_ctx* c, long long* out) {
    if (!c || !out) return RT_ERR_INVALID;
    out[0] = c->n_dirty;
    out[1] = c->dirty_max;
    out[2] = c->dirty_sum;
    out[3] = c->anim.nodes;
    out[4] = static_cast<long long>(c->refit_ids.size());
    out[5] = c->last_flush_bytes;
    out[6] = c->refit_compactions;
    return RT_OK;
}

// Diagnostics: the device state the refit maintains, read back for checking against a
// plain recomputation (tests/refit_ref.py). which: 0 this context, 1 its brute-force
// sub-context, 2 its Moller-Trumbore one (RT_ERR_INVALID while that does not exist or
// does not hold the current scene). Section -1 applies the pending updates as a dispatch
// applies them (flush_updates) and waits for the stream; the other sections copy the
// state as that left it. Nothing a frame depends on changes. *need gets the section's
// size in bytes; it is copied when cap holds it (dst null: the size only).
// Sections 0-11, device arrays byte for byte: staging_shapes, staging_nodes, packed
// nodes, geo_lin, geo_leaf, mat, prims, anodes, wnodes, titems, lnodes, pbox (empty
// without an accelerator; pbox empty without a refit set). Host facts about topology:
// 12 int info {record stride, mt, cone_cull, local wide records, all wide records, prims,
// S, N, I, titems records, few-leaf count, refit entries, accelerator built}; 13 float
// {origin_lim, mt_z xyz}; 14 wide_slot_table; 15 prim_shape; 16 per shape the class the
// accelerator's boxes stand for (a refit entry's at the build, else as last classified);
// 17 per titems record its reference leaf; 18 per shape its refit entry (-1: none).
extern "C" int rt_debug_accel_dump(rt_ctx* c, int which, int section, void* dst, long long cap, long long* need) {
    if (!c || !c->have_scene || !need || which < 0 || which > 2 || section < -1 || section > 18) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    rt_ctx* x = which == 0 ? c : which == 1 ? c->brute : c->mtc;
    if (!x || !x->have_scene || (which == 1 && c->brute_stale) || (which == 2 && c->mtc_stale)) return RT_ERR_INVALID;
    if (section == -1) {
        // one flush per dump, of the dumped context alone (a sub-context was given the writes when
        // they were made): a second flush may land the rebuild that the first one's refit asked for
        if (const int rc = flush_updates(x)) return rc;
        *need = 0;
    }
    HIP_TRY(sync_stream(c));  // the sub-contexts run on this stream
    if (section == -1) return RT_OK;
    const rta::AccelHost& A = x->accel;
    const bool acc = x->accel_ok;
    const size_t S = x->S, N = x->N, I = x->I, P = acc ? A.prim_shape.size() : 0;
    const size_t rec = A.mt ? kWideRecMt : kWideRec;
    const size_t nlw = acc ? A.wchild.size() / rta::kWide : 0;
    const size_t nsw = acc && A.st.wroot >= 0 ? A.st.wchild.size() / rta::kWide : 0;
    const size_t f4 = sizeof(float4);
    const void* dev = nullptr;
    std::vector<int> hi;
    std::vector<float> hf;
    size_t bytes = 0;
    switch (section) {
        case 0: dev = x->staging_shapes, bytes = S * sizeof(FlatShape); break;
        case 1: dev = x->staging_nodes, bytes = N * sizeof(FlatNode); break;
        case 2: dev = x->nodes, bytes = 2 * N * f4; break;
        case 3: dev = x->geo_lin, bytes = 5 * S * f4; break;
        case 4: dev = x->geo_leaf, bytes = 5 * I * f4; break;
        case 5: dev = x->mat, bytes = 2 * S * f4; break;
        case 6: dev = x->prims, bytes = acc ? 4 * P * f4 : 0; break;
        case 7: dev = x->anodes, bytes = acc ? 4 * N * f4 : 0; break;
        case 8: dev = x->wnodes, bytes = acc ? 8 * N * f4 : 0; break;
        case 9: dev = x->titems, bytes = acc ? 2 * static_cast<size_t>(x->n_titems) * f4 : 0; break;
        case 10: dev = x->lnodes, bytes = acc ? rec * (nlw + nsw) * f4 : 0; break;
        case 11: dev = x->pbox, bytes = acc && x->pbox ? 2 * P * f4 : 0; break;
        case 12:
            hi = {static_cast<int>(rec), A.mt ? 1 : 0, x->cone_cull, static_cast<int>(nlw), static_cast<int>(nlw + nsw),
                  static_cast<int>(P), x->S, x->N, x->I, x->n_titems, x->nfew, static_cast<int>(x->refit_ids.size()),
                  acc ? 1 : 0};
            break;
        case 13: hf = {A.origin_lim, A.mt_z[0], A.mt_z[1], A.mt_z[2]}; break;
        case 14:
            if (acc) hi = rta::wide_slot_table(A);
            break;
        case 15:
            if (acc) hi = A.prim_shape;
            break;
        case 16:
            if (acc && A.shape_cls.size() == S) {
                hi = A.shape_cls;
                for (size_t i = 0; i < x->refit_ids.size() && i < x->anim_cls.size(); ++i)
                    hi[x->refit_ids[i]] = x->anim_cls[i];
            }
            break;
        case 17:
            if (acc) hi = x->host_titem_ref;
            break;
        default: hi = x->refit_of; break;
    }
    if (section >= 12) bytes = section == 13 ? hf.size() * sizeof(float) : hi.size() * sizeof(int);
    *need = static_cast<long long>(bytes);
    if (!dst || bytes == 0) return RT_OK;
    if (cap < static_cast<long long>(bytes)) return RT_ERR_INVALID;
    if (section >= 12) {
        std::memcpy(dst, section == 13 ? static_cast<const void*>(hf.data()) : static_cast<const void*>(hi.data()), bytes);
        return RT_OK;
    }
    if (!dev) return RT_ERR_INVALID;
    HIP_TRY(hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_debug_refit(rt_ctx* c, int mode) {
    if (!c || (mode != -1 && mode != 1 && mode != 2)) return RT_ERR_INVALID;
    c->refit_mode = mode;
    return RT_OK;
}

extern "C" int rt_set_walk(rt_ctx* c, int lane_from_depth) {
    if (!c || lane_from_depth < -1) return RT_ERR_INVALID;
    c->lane_from_depth = lane_from_depth;  // -1: back to the automatic policy (walk_from)
    return RT_OK;
}

// Diagnostics: back-face cone culling on/off (takes effect at the next upload).
extern "C" int rt_debug_cone_cull(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID;
    c->cone_cull = on ? 1 : 0;
    return c->have_scene ? upload_accel(c) : RT_OK;
}

// Diagnostics: cap the stack entries of scene-tree walks (0 = none). Exact at
// any value: a lane that runs out walks the reference tree (lane_walk).
extern "C" int rt_debug_scene_stack(rt_ctx* c, int n) {
    if (!c || n < 0) return RT_ERR_INVALID;
    c->scene_stack = n;
    return RT_OK;
}

// Diagnostics: override the per-lane LDS stack depth of k_accel (0 = computed
// bound). A value below the bound can drop stack entries: timing studies only.
// Diagnostics: shadow walks of bounces >= from walk per lane (-1: the default policy).
extern "C" int rt_debug_shadow_walk(rt_ctx* c, int from) {
    if (!c || from < -1) return RT_ERR_INVALID;
    c->shadow_walk_override = from;
    return RT_OK;
}

// Diagnostics: only waves with at most `lanes` rays alive hand them to the tail kernel.
extern "C" int rt_debug_tail_lanes(rt_ctx* c, int lanes) {
    if (!c || lanes < 0 || lanes > 64) return RT_ERR_INVALID;
    c->tail_max_lanes = lanes;
    return RT_OK;
}

extern "C" int rt_set_tail(rt_ctx* c, int from_bounce) {
    if (!c || from_bounce < RT_TAIL_AUTO) return RT_ERR_INVALID;
    c->tail_from = from_bounce;
    return RT_OK;
}

// Diagnostics: re-derive the cost order every `period` dispatches (1: every one).
extern "C" int rt_debug_sched_period(rt_ctx* c, int period) {
    if (!c || period < 1) return RT_ERR_INVALID;
    c->sched_period = period;
    c->sched_frame = 0;
    return RT_OK;
}

extern "C" int rt_debug_moving(rt_ctx* c, int period, int dilate, int split) {
    if (!c || period < 0 || dilate < 0 || dilate > 64) return RT_ERR_INVALID;
    c->moving_period = period;
    c->moving_dilate = dilate;
    c->moving_split = split ? 1 : 0;
    return RT_OK;
}

// Diagnostics / policy: latency-mode cost frames record the event rt_sync_frame waits for (1, default) or not (0).
extern "C" int rt_debug_frame_event(rt_ctx* c, int on) {
    if (!c || on < 0 || on > 1) return RT_ERR_INVALID;
    c->frame_event = on;
    return RT_OK;
}

extern "C" int rt_debug_cost_dilate(rt_ctx* c, int r) {
    if (!c || r < 0 || r > 64) return RT_ERR_INVALID;
    c->cost_dilate = r;
    return RT_OK;
}

extern "C" int rt_debug_lane_stack(rt_ctx* c, int n) {
    if (!c || n < 0 || n > kMaxStack) return RT_ERR_INVALID;
    c->lane_stack_override = n;
    return RT_OK;
}

// Diagnostics (tools/bench_gbuffer.py): the accelerated geometry-buffer kernel walks per lane
// (walk 1) instead of as packets (0), with `waves` tiles to a block (1, 2 or 4; 0 = default).
// Same planes either way.
extern "C" int rt_debug_gbuffer(rt_ctx* c, int walk, int waves) {
    if (!c || (walk != 0 && walk != 1) || (waves != 0 && waves != 1 && waves != 2 && waves != 4)) return RT_ERR_INVALID;
    c->gbuf_walk = walk;
    c->gbuf_waves = waves;
    return RT_OK;
}

// Diagnostics (tools/bench_ao.py): the accelerated ambient-occlusion kernel walks its rays
// repacked over the wave (form 1) or per hit lane (form 2; 0 = the default form), with `waves`
// tiles to a block (1, 2 or 4; 0 = default). Same planes either way.
extern "C" int rt_debug_ao(rt_ctx* c, int form, int waves) {
    if (!c || form < 0 || form > 2 || (waves != 0 && waves != 1 && waves != 2 && waves != 4)) return RT_ERR_INVALID;
    c->ao_form = form;
    c->ao_waves = waves;
    return RT_OK;
}

// Diagnostics (tools/bench_soft.py): k_soft walks the sample rays of bounces >= 1 repacked
// over the wave (form 1) or per live lane (form 2; 0 = the default form). Same pixels either way.
extern "C" int rt_debug_soft(rt_ctx* c, int form) {
    if (!c || form < 0 || form > 2) return RT_ERR_INVALID;
    c->soft_form = form;
    return RT_OK;
}

// Diagnostics (tools/bench_shade.py): the barycentric k_shade instance with plain walks (1) or
// with the split walks of sparse waves (2); 0 = the default choice. Same pixels either way.
extern "C" int rt_debug_shade(rt_ctx* c, int split) {
    if (!c || split < 0 || split > 2) return RT_ERR_INVALID;
    c->shade_split = split;
    return RT_OK;
}

extern "C" int rt_set_kernel_timing(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID;
    c->timing = on != 0;
    return RT_OK;
}

extern "C" int rt_set_latency_mode(rt_ctx* c, int on) {
    if (!c || on < 0 || on > 1) return RT_ERR_INVALID;
    c->latency_mode = on;
    return RT_OK;
}

extern "C" int rt_set_schedule(rt_ctx* c, int mode) {
    if (!c || mode < RT_SCHED_ROWS || mode > RT_SCHED_COST_XCD) return RT_ERR_INVALID;
    c->schedule = mode;
    c->sched_valid = 0;
    return RT_OK;
}

// Diagnostics: dispatch order of k_accel's tiles (a permutation of [0, n)),
// used when n equals the launch's tile count; n = 0 clears it.
extern "C" int rt_debug_tile_order(rt_ctx* c, const int* order, int n) {
    if (!c || n < 0 || (n > 0 && !order)) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    hipFree(c->tile_order);
    c->tile_order = nullptr;
    c->tile_order_n = 0;
    if (n == 0) return RT_OK;
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= n || seen[order[i]]) return RT_ERR_INVALID;
        seen[order[i]] = 1;
    }
    if (hipMalloc(&c->tile_order, n * sizeof(int)) != hipSuccess) return RT_ERR_NO_MEMORY;
    HIP_TRY(hipMemcpy(c->tile_order, order, n * sizeof(int), hipMemcpyHostToDevice));
    c->tile_order_n = n;
    return RT_OK;
}

// Diagnostics: the current cost order (tile indices, longest first) into out[0, n);
// returns the tiles copied (0 when no order exists yet).
extern "C" int rt_debug_sched_order(rt_ctx* c, int* out, int n) {
    if (!c || n < 0 || (n > 0 && !out)) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    HIP_TRY(sync_stream(c));
    const int k = std::min(n, c->sched_valid);
    if (k > 0 && c->sched_order)
        HIP_TRY(hipMemcpy(out, c->sched_order, static_cast<size_t>(k) * sizeof(int), hipMemcpyDeviceToHost));
    return c->sched_order ? k : 0;
}

// Diagnostics: the tile costs that order was made from, as the last cost-recording
// dispatch wrote them (raw: not the dilated copy of rt_debug_cost_dilate), into
// out[0, n); returns the tiles copied (0 when no order exists yet).
extern "C" int rt_debug_sched_cost(rt_ctx* c, unsigned* out, int n) {
    if (!c || n < 0 || (n > 0 && !out)) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    HIP_TRY(sync_stream(c));
    const int k = std::min(n, c->sched_valid);
    if (k > 0 && c->sched_cost)
        HIP_TRY(hipMemcpy(out, c->sched_cost, static_cast<size_t>(k) * sizeof(unsigned), hipMemcpyDeviceToHost));
    return c->sched_cost ? k : 0;
}

// Diagnostics: the first k tiles of the cost order (the heaviest) each run as `parts`
// waves (1, 2, 4 or 8), one band of 64 / parts pixels per wave; parts = 1: off;
// k = -1: the default policy (kHeavyAutoSlots).
extern "C" int rt_debug_heavy(rt_ctx* c, int k, int parts) {
    if (!c || k < -1 || parts < 1 || parts > 64 || (parts & (parts - 1)) != 0) return RT_ERR_INVALID;
    c->heavy_k = k;
    c->heavy_parts = parts;
    return RT_OK;
}

// Diagnostics: the first k dispatch slots of the cost order (the heaviest tiles) walk
// their camera rays (mode bit 0) and / or the camera rays' shadow rays (bit 1) per lane;
// k = -1: the default policy.
// Diagnostics: a cost-recording dispatch ranks the tiles by their waves' wall time
// (1) or by their lanes' node steps + tests (0); -1: the default policy.
extern "C" int rt_debug_cost_time(rt_ctx* c, int mode) {
    if (!c || mode < -1 || mode > 1) return RT_ERR_INVALID;
    c->cost_time = mode;
    c->sched_valid = 0;
    return RT_OK;
}

extern "C" int rt_debug_lane_k(rt_ctx* c, int k, int mode) {
    if (!c || k < -1 || mode < 0 || mode > 3) return RT_ERR_INVALID;
    c->lane_k = k;
    c->lane_k_mode = mode;
    return RT_OK;
}

// Diagnostics: split per-lane walks (lane_walk_any) of waves with at most max_rays rays
// over groups of at most group lanes (a power of two, 2..64); max_rays = 0 turns it off.
extern "C" int rt_debug_split(rt_ctx* c, int max_rays, int group) {
    if (!c || max_rays < 0 || max_rays > 32 || group < 2 || group > 64 || (group & (group - 1))) return RT_ERR_INVALID;
    c->split_max = max_rays;
    c->split_g = group;
    return RT_OK;
}

// Diagnostics: supersampled frames (rt_set_samples) take the general path -- the sample
// frame into the scratch surface, then k_box_filter -- even where k_accel would reduce the
// samples in its store. Same image either way (tests, tools/bench_ss.py's baseline).
// Diagnostics: frames in a display format render as a float frame into the scratch surface
// followed by the filter kernel's conversion, instead of converting in the render kernel's
// store. Same image either way (tools/bench_formats.py's baseline).
extern "C" int rt_debug_convert_pass(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID;
    c->convert_pass = on != 0;
    return RT_OK;
}

// Diagnostics: the display conversion alone over caller data, so that tests can feed it values
// no frame holds (NaN, infinities, ties, the sRGB thresholds and their neighbours): `rows` compact
// rows of `width` RGBA32F pixels at device pointer src become rows of `format` at dst, by the
// filter kernel's conversion (the render kernels' store_display). Stream-ordered, asynchronous.
extern "C" int rt_debug_convert(rt_ctx* c, const float* src, size_t src_pitch, void* dst, size_t pitch, int width,
                                int rows, int format) {
    if (!c || !src || !dst || width <= 0 || rows <= 0 || rows > 4 * 65535 || format < RT_FORMAT_RGBA8 ||
        format_bytes(format) == 0)
        return RT_ERR_INVALID;
    const size_t px = format_bytes(format), align = format_align(format);
    if (src_pitch < static_cast<size_t>(width) * 16 || src_pitch % 16 != 0 ||
        reinterpret_cast<uintptr_t>(src) % 16 != 0 || pitch < static_cast<size_t>(width) * px || pitch % align != 0 ||
        reinterpret_cast<uintptr_t>(dst) % align != 0)
        return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    hipLaunchKernelGGL((k_box_filter<1, true>), dim3((width + 63) / 64, (rows + 3) / 4), dim3(256), 0, c->stream,
                       reinterpret_cast<const char*>(src), src_pitch, static_cast<char*>(dst), pitch, width, rows, 0, 1,
                       1, rows, format);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_debug_ss_general(rt_ctx* c, int on) {
    if (!c) return RT_ERR_INVALID;
    c->ss_general = on != 0;
    return RT_OK;
}

// Diagnostics (not part of rt_api.h): enable per-tile records for k_accel
// (cap tiles; 0 disables) and read them back (kTileRec u64 per tile, layout
// at kTileRec). Synchronous.
extern "C" int rt_debug_tile_times(rt_ctx* c, int cap, unsigned long long* out) {
    if (!c || cap < 0) return RT_ERR_INVALID;
    if (set_dev(c) != RT_OK) return RT_ERR_DEVICE;
    HIP_TRY(sync_stream(c));
    if (out && c->tile_times && cap > 0) {
        const size_t n = std::min(static_cast<size_t>(cap), c->tile_times_cap);
        HIP_TRY(hipMemcpy(out, c->tile_times, n * kTileRec * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return static_cast<int>(n);
    }
    hipFree(c->tile_times);
    c->tile_times = nullptr;
    c->tile_times_cap = 0;
    if (cap > 0) {
        if (hipMalloc(&c->tile_times, static_cast<size_t>(cap) * kTileRec * sizeof(unsigned long long)) != hipSuccess)
            return RT_ERR_NO_MEMORY;
        c->tile_times_cap = cap;
    }
    return RT_OK;
}
