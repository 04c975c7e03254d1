// refit_ref.cpp — TEST HARNESS for tests/refit_ref.py: the few product functions the
// plain reference of the refit's device state needs as they are (the conservative
// bound of a record, a triangle's Moller-Trumbore constants, the quantized cone test
// on one word and one direction, the cone word's fields), and a host-built "dump" of
// a freshly built accelerator in the layout of rt_debug_accel_dump, packed by the
// product's own packer (accel_pack.h), for checking the reference without a GPU
// (tests/test_refit_ref_cpu.py). Not product code.
// Built by the test modules: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared, with accel.cpp.
#include <cstring>
#include <vector>

#include "../../opengl-ray-tracer_amd/csrc/accel.h"
#include "../../opengl-ray-tracer_amd/csrc/accel_math.h"
#include "../../opengl-ray-tracer_amd/csrc/accel_pack.h"

namespace {

// the last rr_build's sections, numbered as rt_debug_accel_dump's
std::vector<char> g_sec[19];
template <class T>
void put(int s, const T* v, size_t n) {
    g_sec[s].assign(reinterpret_cast<const char*>(v), reinterpret_cast<const char*>(v) + n * sizeof(T));
}
template <class T>
void put(int s, const std::vector<T>& v) {
    put(s, v.data(), v.size());
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

// Builds the accelerator on the host (rta::build_accel) and packs it with the renderer's
// own packer (rta::pack_accel, what upload_built_accel copies to the device); the sections
// are read with rr_section. Sections 7-10 and 17 are the packer's arrays, cut to the sizes
// rt_debug_accel_dump reports; the packed node records (2) are restated here.
int rr_build(const FlatShape* shapes, int S, const FlatNode* nodes, int N, const int* idx, int I, int mt) {
    for (auto& v : g_sec) v.clear();
    rta::AccelHost A;
    if (!rta::build_accel(shapes, S, nodes, N, idx, I, rta::kLeafScan, rta::kMaxStack, A, mt != 0)) return -1;
    rta::PackedAccel pk;
    if (!rta::pack_accel(A, nodes, N, true, pk)) return -1;
    put(0, shapes, S);
    put(1, nodes, N);
    std::vector<rta::F4> nd(2 * static_cast<size_t>(N));
    for (int k = 0; k < N; ++k) {
        const FlatNode& n = nodes[k];
        const bool leaf = n.leftChild == -1;
        nd[2 * k] = rta::F4{n.boundsMin.x, n.boundsMin.y, n.boundsMin.z, rta::bits_f(leaf ? -(n.startShapeIdx + 1) : n.leftChild)};
        nd[2 * k + 1] = rta::F4{n.boundsMax.x, n.boundsMax.y, n.boundsMax.z, rta::bits_f(leaf ? n.numShapes : n.rightChild)};
    }
    put(2, nd);
    put(7, pk.an.data(), pk.an.size());
    put(8, pk.wn.data(), pk.wn.size());
    put(9, pk.ti.data(), 2 * pk.titem_ref.size());
    put(10, pk.ln.data(), pk.rec * (pk.nw + pk.nws));
    put(17, pk.titem_ref);
    put(14, rta::wide_slot_table(A));
    put(15, A.prim_shape);
    put(16, A.shape_cls);
    put(18, std::vector<int>(static_cast<size_t>(S), -1));
    put(12, std::vector<int>{pk.rec, mt ? 1 : 0, 1, static_cast<int>(pk.nw), static_cast<int>(pk.nw + pk.nws),
                             static_cast<int>(A.prim_shape.size()), S, N, I, static_cast<int>(pk.titem_ref.size()), pk.nfew, 0, 1});
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
