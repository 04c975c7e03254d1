// refit_ref.cpp — TEST HARNESS for tests/refit_ref.py: the few product functions the
// plain reference of the refit's device state needs as they are (the conservative
// bound of a record, a triangle's Moller-Trumbore constants, the quantized cone test
// on one word and one direction, the cone word's fields), and a host-built "dump" of
// a freshly built accelerator in the layout of rt_debug_accel_dump, for checking the
// reference without a GPU (tests/test_refit_ref_cpu.py). Not product code.
// Built by the test modules: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared, with accel.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "../../opengl-ray-tracer_amd/csrc/accel.h"
#include "../../opengl-ray-tracer_amd/csrc/accel_math.h"

namespace {

struct F4 {
    float x, y, z, w;
};
float bits_f(int v) {
    float f;
    std::memcpy(&f, &v, sizeof f);
    return f;
}

// the last rr_build's sections, numbered as rt_debug_accel_dump's
std::vector<char> g_sec[19];
template <class T>
void put(int s, const std::vector<T>& v) {
    g_sec[s].assign(reinterpret_cast<const char*>(v.data()), reinterpret_cast<const char*>(v.data()) + v.size() * sizeof(T));
}

}  // namespace

extern "C" {

// class and conservative box (lo xyz, hi xyz; untouched unless BOUNDED) per record
int rr_classify(const FlatShape* s, int n, float origin_lim, int mt, int* cls, float* box) {
    for (int i = 0; i < n; ++i) {
        rta::Box3 b;
        cls[i] = rta::classify(s[i], b, origin_lim, mt != 0);
        if (cls[i] != rta::BOUNDED) continue;
        for (int a = 0; a < 3; ++a) {
            box[6 * i + a] = b.lo[a];
            box[6 * i + 3 + a] = b.hi[a];
        }
    }
    return 0;
}

// per record: whether it is a triangle with MT constants (classify_mt_tight), and
// q = {cr, X, esum, p1 xyz}
int rr_mt_tri(const FlatShape* s, int n, int* ok, double* q) {
    for (int i = 0; i < n; ++i) {
        rta::MtTri t{};
        rta::Box3 b;
        ok[i] = s[i].type == RT_TRIANGLE && rta::classify_mt_tight(s[i], b, 0.0, t) == rta::BOUNDED;
        const double v[6] = {t.cr, t.X, t.esum, t.p1[0], t.p1[1], t.p1[2]};
        for (int a = 0; a < 6; ++a) q[6 * i + a] = ok[i] ? v[a] : 0.0;
    }
    return 0;
}

// out[i]: the word words[i] culls a ray of direction d[3 i ..] (ray_consts' dq, cone_culls_q)
int rr_cone_culls(const int* words, const float* d, int n, unsigned char* out) {
    for (int i = 0; i < n; ++i) {
        const rta::RayC c = rta::ray_consts(0.f, 0.f, 0.f, d[3 * i], d[3 * i + 1], d[3 * i + 2], 1.f);
        out[i] = rta::cone_culls_q(words[i], c.dq) ? 1 : 0;
    }
    return 0;
}

// the cone word's fields: the axis bytes and the threshold byte, signed
int rr_cone_decode(const int* words, int n, int* out) {
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < 4; ++b) out[4 * i + b] = static_cast<signed char>((words[i] >> (8 * b)) & 0xff);
    return 0;
}

// Builds the accelerator on the host (rta::build_accel) and packs it as the renderer
// uploads it; the sections are read with rr_section. The node and leaf codes (.w words
// of the wide records) are left 0: the reference only asks that they do not change.
int rr_build(const FlatShape* shapes, int S, const FlatNode* nodes, int N, const int* idx, int I, int mt) {
    for (auto& v : g_sec) v.clear();
    rta::AccelHost A;
    if (!rta::build_accel(shapes, S, nodes, N, idx, I, 8, 64, A, mt != 0)) return -1;
    const rta::SceneTree& T = A.st;
    const bool use_st = T.wroot >= 0;
    const size_t P = A.prim_shape.size();
    const size_t nlw = A.wchild.size() / rta::kWide, nsw = use_st ? T.wchild.size() / rta::kWide : 0;
    const int rec = mt ? 17 : 8;
    put(0, std::vector<FlatShape>(shapes, shapes + S));
    put(1, std::vector<FlatNode>(nodes, nodes + N));
    std::vector<F4> pk(2 * static_cast<size_t>(N)), an(4 * static_cast<size_t>(N)), wn(8 * static_cast<size_t>(N), F4{0, 0, 0, 0});
    for (int k = 0; k < N; ++k) {
        const FlatNode& n = nodes[k];
        const bool leaf = n.leftChild == -1;
        pk[2 * k] = F4{n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, bits_f(leaf ? -(n.startShapeIdx + 1) : n.leftChild)};
        pk[2 * k + 1] = F4{n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, bits_f(leaf ? n.numShapes : n.rightChild)};
        const rta::Box3& cb = A.content[k];
        an[4 * k + 0] = F4{n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, bits_f(n.leftChild)};
        an[4 * k + 1] = F4{n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, bits_f(n.rightChild)};
        an[4 * k + 2] = F4{cb.lo[0], cb.lo[1], cb.lo[2], bits_f(A.flags[k])};
        an[4 * k + 3] = F4{cb.hi[0], cb.hi[1], cb.hi[2], 0.f};
        if (leaf) continue;
        const int ch[2] = {n.leftChild, n.rightChild};
        for (int s = 0; s < 2; ++s) {
            const FlatNode& cn = nodes[ch[s]];
            const rta::Box3& cc = A.content[ch[s]];
            F4* q = &wn[8 * static_cast<size_t>(k) + 4 * s];
            q[0] = F4{cn.boundsMin.x, cn.boundsMin.y, cn.boundsMin.z, 0.f};
            q[1] = F4{cn.boundsMax.x, cn.boundsMax.y, cn.boundsMax.z, 0.f};
            q[2] = F4{cc.lo[0], cc.lo[1], cc.lo[2], bits_f(A.flags[ch[s]] & 8)};
            q[3] = F4{cc.hi[0], cc.hi[1], cc.hi[2], 0.f};
        }
    }
    put(2, pk);
    put(7, an);
    put(8, wn);
    // wide records: the local ones, then the scene tree's
    std::vector<float> ln(4 * static_cast<size_t>(rec) * (nlw + nsw), 0.f);
    auto emit = [&](size_t at, const int* wchild, const std::vector<rta::Box3>& boxes, const std::vector<float>& cones,
                    bool local) {
        float* r = &ln[4 * static_cast<size_t>(rec) * at];
        for (int s = 0; s < 4; ++s) {
            const int j = wchild[s];
            float box[6] = {0, 0, 0, 0, 0, 0}, cone[4] = {0, 0, 0, -4.f}, k[rta::kMtPadF] = {0, 0, 0, 0, 0, 0};
            if (j >= 0) {
                for (int a = 0; a < 3; ++a) {
                    box[a] = boxes[j].lo[a];
                    box[3 + a] = boxes[j].hi[a];
                }
                for (int a = 0; a < 4; ++a) cone[a] = cones[4 * static_cast<size_t>(j) + a];
                if (mt && local)
                    for (int a = 0; a < rta::kMtPadF; ++a) k[a] = A.lmt[rta::kMtPadF * static_cast<size_t>(j) + a];
            }
            if (mt) {
                float* blk = r + 16 * s;
                for (int a = 0; a < 6; ++a) blk[a] = box[a];
                for (int a = 0; a < 4; ++a) blk[6 + a] = cone[a];
                for (int a = 0; a < rta::kMtPadF; ++a) blk[10 + a] = k[a];
            } else {
                for (int a = 0; a < 6; ++a) r[4 * a + s] = box[a];
                r[4 * 6 + s] = bits_f(j < 0 ? rta::kConeNever : rta::cone_word(cone[0], cone[1], cone[2], cone[3]));
            }
        }
    };
    for (size_t w = 0; w < nlw; ++w) emit(w, &A.wchild[rta::kWide * w], A.lbox, A.lcone, true);
    for (size_t w = 0; w < nsw; ++w) emit(nlw + w, &T.wchild[rta::kWide * w], T.box, A.st_cone, false);
    put(10, ln);
    // scene-tree items: the leaves' exact boxes (few-leaf layout) or one record per item
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
    const std::vector<int> refs = use_st ? (few.empty() ? T.item_ref : few) : std::vector<int>();
    std::vector<F4> ti(2 * refs.size());
    for (size_t i = 0; i < refs.size(); ++i) {
        const FlatNode& n = nodes[refs[i]];
        ti[2 * i] = F4{n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, few.empty() ? bits_f(T.item_start[i]) : 0.f};
        ti[2 * i + 1] = F4{n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, few.empty() ? bits_f(T.item_count[i]) : 0.f};
    }
    put(9, ti);
    put(17, refs);
    put(14, rta::wide_slot_table(A));
    put(15, A.prim_shape);
    put(16, A.shape_cls);
    put(18, std::vector<int>(static_cast<size_t>(S), -1));
    put(12, std::vector<int>{rec, mt ? 1 : 0, 1, static_cast<int>(nlw), static_cast<int>(nlw + nsw), static_cast<int>(P), S, N,
                             I, static_cast<int>(refs.size()), static_cast<int>(few.size()), 0, 1});
    put(13, std::vector<float>{A.origin_lim, A.mt_z[0], A.mt_z[1], A.mt_z[2]});
    return 0;
}

int rr_section(int section, void* dst, long long cap, long long* need) {
    if (section < 0 || section > 18 || !need) return -1;
    *need = static_cast<long long>(g_sec[section].size());
    if (!dst || *need == 0) return 0;
    if (cap < *need) return -1;
    std::memcpy(dst, g_sec[section].data(), g_sec[section].size());
    return 0;
}

}  // extern "C"
