// accel_pack.h — the device layout of a built accelerator, packed on the host: what
// rt_kernels.hip uploads (upload_built_accel) and what its kernels read (AccelPtrs), as
// one pure function of rta::AccelHost and the host's node records. No HIP: plain C++,
// so the tests' host dump (tests/native/refit_ref.cpp) is the product's own packing.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <vector>

#include "accel.h"
#include "accel_codes.h"
#include "accel_math.h"
#include "host_laps.h"

namespace rta {

// A host array left uninitialised: no serial zeroing pass, its pages are first touched
// by the threads that fill it (config 5's 24 MB of wnodes: 5.4 ms of page faults on one
// thread). Every element is written before the array is read.
template <class T>
struct RawArray {
    std::unique_ptr<T[]> p;
    size_t n = 0;
    void reset(size_t count) {
        p.reset(new T[count]);
        n = count;
    }
    T* data() { return p.get(); }
    const T* data() const { return p.get(); }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
};

struct PackedAccel {
    RawArray<F4> an;         // anodes: 4 per reference node, exact box + children, content box + flags
    std::vector<F4> ln;      // lnodes: `rec` per wide record, the local ones then the scene tree's
    RawArray<F4> wn;         // wnodes: 8 per reference node, both children's exact + content boxes
    RawArray<I4> tl;         // tleaf: per reference leaf its plain range and local root code
    std::vector<F4> ti;      // titems: 2 per record (titem_ref), the leaf's exact box + prim range
    std::vector<int> ps;     // prim_shape, then prim_seq
    std::vector<int> titem_ref;  // per titems record its reference leaf (few-leaf layout: per leaf)
    bool use_st = false;     // the accelerator has a scene tree (titems, titem_ref)
    // -1 until decided: a refused pack leaves what it had decided by then
    int boxes_finite = -1;   // no reference node box holds a NaN
    int nfew = -1;           // > 0: the few-leaf titems layout over nfew reference leaves
    int st_root = kNoChild;  // scene-tree root code
    int rec = kWideRec;      // wide record stride
    size_t nw = 0, nws = 0;  // local and scene-tree wide records
};

// the code of the node whose first record is r (+ base): kPair when it spans two
inline int wide_code(const std::vector<char>& pair, int r, size_t base) {
    return static_cast<int>(kLocal | static_cast<unsigned>(base + r) |
                            (r < static_cast<int>(pair.size()) && pair[r] ? kPair : 0u));
}

// Wide record w of one tree (the local trees, or the scene tree with local = false) as
// record `at` of ln. leaf_of(j): the code of binary leaf j; inner children get wide codes
// from sub_base on.
template <class LeafCode>
void emit_wide(const AccelHost& A, bool cone_cull, std::vector<F4>& ln, size_t w, size_t at, const std::vector<int>& wchild,
               const std::vector<int>& wsub, const std::vector<char>& wpair, const std::vector<Box3>& boxes,
               const std::vector<float>& cones, bool local, const LeafCode& leaf_of, size_t sub_base) {
    const int rec = A.mt ? kWideRecMt : kWideRec;
    float v[kWideRecMt][4];
    for (int s2 = 0; s2 < 4; ++s2) {
        const int j = wchild[kWide * w + s2];
        int code = kNoChild;
        float box[6] = {0, 0, 0, 0, 0, 0}, cone[4] = {0, 0, 0, -4.f}, mtc[kMtPadF] = {0, 0, 0, 0, 0, 0};
        if (j >= 0) {
            const Box3& bx = boxes[j];
            for (int a = 0; a < 3; ++a) {
                box[a] = bx.lo[a];
                box[3 + a] = bx.hi[a];
            }
            for (int a = 0; a < 4; ++a) cone[a] = cones[4 * j + a];
            if (!cone_cull && cone[3] > kNoPrune) cone[3] = A.mt ? 2.f : -4.f;
            if (A.mt && local)
                for (int a = 0; a < kMtPadF; ++a) mtc[a] = A.lmt[kMtPadF * j + a];
            const int sub = wsub[kWide * w + s2];
            code = sub < 0 ? leaf_of(j) : wide_code(wpair, sub, sub_base);
        }
        if (A.mt) {  // per child 16 floats: box, cone, the per-ray padding constants
            float* blk = &v[0][0] + 16 * s2;
            for (int a = 0; a < 6; ++a) blk[a] = box[a];
            for (int a = 0; a < 4; ++a) blk[6 + a] = cone[a];
            for (int a = 0; a < kMtPadF; ++a) blk[10 + a] = mtc[a];
        } else {
            for (int a = 0; a < 6; ++a) v[a][s2] = box[a];
            v[6][s2] = bits_f(j < 0 ? kConeNever : cone_word(cone[0], cone[1], cone[2], cone[3]));
        }
        v[rec - 1][s2] = bits_f(code);
    }
    for (int r = 0; r < rec; ++r) ln[rec * at + r] = F4{v[r][0], v[r][1], v[r][2], v[r][3]};
}

// Packs A (built for `nodes`) with the node records' current exact boxes. False where a
// code cannot hold its index (28 bits of node, 27 of wide record, 28 of item, a local
// leaf's start < 2^22 and count < 64, a prim's rank < 2^29): no accelerator then.
// laps: the caller's "upload" laps, if it keeps any.
inline bool pack_accel(const AccelHost& A, const FlatNode* nodes, int N, bool cone_cull, PackedAccel& out,
                       PhaseLaps* laps = nullptr) {
    if (N >= (1 << 28)) return false;  // codes carry the node index in 28 bits
    // The arrays below are packed on the build threads (parallel_for): each entry is
    // written by one thread from read-only inputs.
    constexpr int kPackChunk = 8192;
    // anodes: every reference node's exact box and content box (the root's entry test).
    RawArray<F4>& an = out.an;
    an.reset(4 * static_cast<size_t>(N));
    std::atomic<int> nan_box{0};
    parallel_for(N, kPackChunk, [&](int k0, int k1) {
        int nan = 0;
        for (int k = k0; k < k1; ++k) {
            const FlatNode& n = nodes[k];
            for (float v : {n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, n.boundsMax.x, n.boundsMax.y, n.boundsMax.z})
                nan |= std::isnan(v) ? 1 : 0;
            const Box3& cb = A.content[k];
            an[4 * k + 0] = F4{n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, bits_f(n.leftChild)};
            an[4 * k + 1] = F4{n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, bits_f(n.rightChild)};
            an[4 * k + 2] = F4{cb.lo[0], cb.lo[1], cb.lo[2], bits_f(A.flags[k])};
            an[4 * k + 3] = F4{cb.hi[0], cb.hi[1], cb.hi[2], 0.f};
        }
        if (nan) nan_box.store(1);
    });
    out.boxes_finite = nan_box.load() ? 0 : 1;
    lap_of(laps, "anodes");
    // lnodes: the wide local nodes (accel.h, build_wide), kWideRec float4 each with
    // quantized cones (kWideRecMt with the MT accelerator's float grazing cones; wide_kids).
    const size_t P = A.prim_shape.size();
    const int rec = out.rec = A.mt ? kWideRecMt : kWideRec;
    std::atomic<bool> codes_ok{true};
    auto leaf_code = [&](int j) -> int {
        const unsigned st = static_cast<unsigned>(-A.la[j] - 1), cnt = static_cast<unsigned>(A.lb[j]);
        if (st >= (1u << 22) || cnt > 63u) codes_ok.store(false);
        return static_cast<int>(kLocal | kLeaf | (st << 6) | cnt);
    };
    // The scene tree's wide nodes (accel.h, SceneTree) follow the local ones;
    // its leaves are item codes (kTopLeaf | kItem | item).
    const SceneTree& T = A.st;
    const bool use_st = out.use_st = T.wroot >= 0;
    const size_t nw = out.nw = A.wchild.size() / kWide;
    const size_t nws = out.nws = use_st ? T.wchild.size() / kWide : 0;
    if (nw + nws >= (1u << 27) || T.item_ref.size() >= (1u << 28)) return false;  // kRecMask, kItem
    std::vector<F4>& ln = out.ln;
    ln = std::vector<F4>(rec * (nw + nws ? nw + nws : 1));
    parallel_for(static_cast<int>(nw), kPackChunk, [&](int w0, int w1) {
        for (size_t w = static_cast<size_t>(w0); w < static_cast<size_t>(w1); ++w)
            emit_wide(A, cone_cull, ln, w, w, A.wchild, A.wsub, A.wpair, A.lbox, A.lcone, true, leaf_code, 0);
    });
    lap_of(laps, "local wide nodes");
    // Items: with <= 8 distinct reference leaves (few-leaf mode, few_mask) a
    // local-leaf code kLocal|kLeaf|kItem|start<<6|leaf<<3|count and titems =
    // the leaves' exact boxes; otherwise kTopLeaf|kItem|item and titems = per
    // item its leaf's exact box + prim range.
    std::vector<int> few;
    if (use_st) {
        for (int k : T.item_ref)
            if (std::find(few.begin(), few.end(), k) == few.end()) {
                few.push_back(k);
                if (few.size() > 8) break;
            }
        if (few.size() > 8) few.clear();
        for (size_t i = 0; i < T.item_ref.size() && !few.empty(); ++i)
            if (T.item_count[i] > 7 || T.item_start[i] >= (1 << 22)) few.clear();
    }
    out.nfew = static_cast<int>(few.size());
    auto item_code = [&](int j) {
        const int i = T.item_of[j];
        if (few.empty()) return static_cast<int>(kTopLeaf | kItem | static_cast<unsigned>(i));
        const unsigned f = static_cast<unsigned>(std::find(few.begin(), few.end(), T.item_ref[i]) - few.begin());
        return static_cast<int>(kLocal | kLeaf | kItem | (static_cast<unsigned>(T.item_start[i]) << 6) | (f << 3) |
                                static_cast<unsigned>(T.item_count[i]));
    };
    std::vector<F4>& ti = out.ti;
    ti = std::vector<F4>(2 * (use_st ? std::max<size_t>(T.item_ref.size(), 1) : 1));
    if (use_st) {
        parallel_for(static_cast<int>(nws), kPackChunk, [&](int w0, int w1) {
            for (size_t w = static_cast<size_t>(w0); w < static_cast<size_t>(w1); ++w)
                emit_wide(A, cone_cull, ln, w, nw + w, T.wchild, T.wsub, T.wpair, T.box, A.st_cone, false, item_code, nw);
        });
        auto put = [&](size_t i, int ref, int start, int count) {
            const FlatNode& n = nodes[ref];
            ti[2 * i] = F4{n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, bits_f(start)};
            ti[2 * i + 1] = F4{n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, bits_f(count)};
        };
        if (!few.empty())
            for (size_t i = 0; i < few.size(); ++i) put(i, few[i], 0, 0);
        else
            for (size_t i = 0; i < T.item_ref.size(); ++i) put(i, T.item_ref[i], T.item_start[i], T.item_count[i]);
        out.titem_ref = few.empty() ? T.item_ref : few;
    }
    lap_of(laps, "scene tree nodes, items");
    // wnodes: per reference inner node both children's exact + content boxes;
    // tleaf: per reference leaf its plain range and local root code.
    RawArray<F4>& wn = out.wn;
    RawArray<I4>& tl = out.tl;
    wn.reset(8 * static_cast<size_t>(N));
    tl.reset(static_cast<size_t>(N));
    auto top_code_of = [&](int k) {
        return nodes[k].leftChild == -1 ? static_cast<int>(kTopLeaf | static_cast<unsigned>(k)) : k;
    };
    parallel_for(N, kPackChunk, [&](int k0, int k1) {
        for (int k = k0; k < k1; ++k) {
            const FlatNode& n = nodes[k];
            if (n.leftChild == -1) {
                const int r = A.local_root[k];
                const int lr = A.wroot[k] >= 0 ? wide_code(A.wpair, A.wroot[k], 0) : (r >= 0 ? leaf_code(r) : kNoChild);
                tl[k] = I4{A.plain_start[k], A.plain_count[k], lr, 0};
                for (int q = 0; q < 8; ++q) wn[8 * static_cast<size_t>(k) + q] = F4{0.f, 0.f, 0.f, 0.f};
                continue;
            }
            tl[k] = I4{0, 0, kNoChild, 0};
            const int ch[2] = {n.leftChild, n.rightChild};
            for (int s2 = 0; s2 < 2; ++s2) {
                const FlatNode& cn = nodes[ch[s2]];
                const Box3& cb = A.content[ch[s2]];
                F4* q = &wn[8 * static_cast<size_t>(k) + 4 * s2];
                q[0] = F4{cn.boundsMin.x, cn.boundsMin.y, cn.boundsMin.z, s2 == 0 ? bits_f(top_code_of(ch[0])) : 0.f};
                q[1] = F4{cn.boundsMax.x, cn.boundsMax.y, cn.boundsMax.z, s2 == 0 ? bits_f(top_code_of(ch[1])) : 0.f};
                q[2] = F4{cb.lo[0], cb.lo[1], cb.lo[2], bits_f(A.flags[ch[s2]] & 8)};
                q[3] = F4{cb.hi[0], cb.hi[1], cb.hi[2], 0.f};
            }
        }
    });
    lap_of(laps, "wnodes, tleaf");
    if (!codes_ok.load()) return false;
    for (size_t i = 0; i < P; ++i)  // PrimRec::st = seq << 2 | type
        if (A.prim_seq[i] < 0 || A.prim_seq[i] >= (1 << 29)) return false;
    std::vector<int>& ps = out.ps;
    ps = std::vector<int>(2 * (P ? P : 1));
    for (size_t i = 0; i < P; ++i) {
        ps[i] = A.prim_shape[i];
        ps[P + i] = A.prim_seq[i];
    }
    lap_of(laps, "prim lists");
    out.st_root = use_st ? wide_code(T.wpair, T.wroot, nw) : kNoChild;
    return true;
}

}  // namespace rta
