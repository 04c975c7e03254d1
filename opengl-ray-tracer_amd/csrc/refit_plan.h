// refit_plan.h — the refit's maps, planned on the host: for a scene, its accelerator and
// a refit set (the animated shapes and those rt_update_shapes rewrote), every list that
// k_refit reads (rt_kernels.hip AnimMaps, RefitArgs) and the slot arrays prepare_animation
// uploads, as pure functions in the two steps prepare_animation takes them. No HIP: plain
// C++ (tests/native/refit_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/rt_api.h"
#include "accel.h"
#include "accel_codes.h"
#include "host_laps.h"

namespace rta {

// Where each list starts in RefitPlan::buf (ints). Per refit entry i (CSR: off has
// count + 1 running sums, list the concatenation):
//   slot  : its geo_leaf slots (bvhIndices positions)
//   prim  : its accelerator prim slots
//   wpos  : wide-record slots (4*w + s) of the local and scene-tree nodes above those prims
// Per reference node j that lists an entry (node_ids[j]):
//   node  : the entries it lists (updateBVH's set, leaves + ancestors)
//   wn    : the wnodes child slots (2 * parent + side) that hold its box
//   item  : the scene-tree items (titems records) whose exact box is its box
struct RefitOffsets {
    size_t ids = 0;  // the refit set's shapes
    size_t slot_off = 0, slot_list = 0, prim_off = 0, prim_list = 0, wpos_off = 0, wpos_list = 0;
    size_t node_off = 0, node_list = 0, wn_off = 0, wn_list = 0, item_off = 0, item_list = 0;
    size_t node_ids = 0;    // the reference nodes listing an entry
    size_t ecls = 0;        // per entry: the class the accelerator was built with
    size_t prim_entry = 0;  // per accelerator prim: its shape's refit entry (-1: none)
};

// What the context keeps of a plan beyond the device arrays, rewritten in place.
struct RefitState {
    std::vector<int>& refit_of;     // shape -> refit entry, -1 outside the set
    std::vector<int>& anim_cls;     // per entry: classify() of its build-time record (kept as it was for an empty set)
    std::vector<char>& entry_root;  // per entry: node N-1 lists it
};

struct RefitPlan {
    bool slots = false;            // with an accelerator: RefitSlots is filled
    int n_dirty = 0, n_big = 0, dirty_max = 0;
    long long dirty_sum = 0;
    long long n_direct_slot_reads = 0;  // the slots' refit prims
    long long direct_reads = 0;         // records k_refit's roles read when they derive the boxes themselves
    std::vector<int> buf;  // every int list of AnimMaps, at `o`
    RefitOffsets o;
    int n_nodes = 0;       // node_ids' length
    // per entry, from plan_refit_slots to plan_refit_lists: its reference nodes, geo_leaf slots, prims, wide slots
    std::vector<std::vector<int>> nodes_of, slots_of, prims_of, wpos_of;
};

// The slot refit's arrays (with an accelerator), uploaded and dropped before the lists are built.
struct RefitSlots {
    std::vector<F4> pb;    // per prim its conservative box (lo, hi), empty (inf, -inf) if not BOUNDED
    std::vector<I4> work;  // dirty slots {slot, first prim, end prim, start in dl}, big ones first, + the end
    std::vector<F4> st;    // per dirty slot: the box of its prims outside the set (lo, hi)
    std::vector<int> dl;   // per dirty slot: its prims in the set, in order
};

// The per-shape cache of classify() the slot boxes are built from (AccelHost::shape_cls /
// shape_box as built, then as last classified here): plan_refit classifies the moved
// shapes again, writes them back and clears their moved flag. Its one side effect.
struct ShapeCache {
    std::vector<int>& cls;
    std::vector<Box3>& box;
    std::vector<char>& moved;
};

inline bool st_noprune(const AccelHost& A, int j) { return A.st_cone[4 * static_cast<size_t>(j) + 3] <= kNoPrune; }

// The scene tree's wide slots (after the nw local records) whose boxes have no distance
// bound (kNoPrune): open_inf_slots opens them; the refit leaves them alone.
inline std::vector<int> noprune_slots(const AccelHost& A) {
    const size_t nw = A.wchild.size() / kWide;
    std::vector<int> slots;
    for (size_t q = 0; q < A.st.wchild.size(); ++q)
        if (A.st.wchild[q] >= 0 && st_noprune(A, A.st.wchild[q])) slots.push_back(static_cast<int>(4 * nw + q));
    return slots;
}

// One binary tree over prims (inner a = left, b = right | axis << 30; leaf a = -(start+1),
// b = count) with its wide collapse: per node its wide slot (slot_base + position in
// wchild, -1: none, or skipped), and whether a prim of the refit set lies below it.
// Appends each entry's slots to wpos_of and, if asked, its prims to prims_of.
// which: shape -> refit entry, -1 none.
struct TreeSlots {
    std::vector<int> wpos;
    std::vector<char> dirty;
};
template <class Skip>
TreeSlots slots_above(const std::vector<int>& a, const std::vector<int>& b, const std::vector<int>& wchild, size_t slot_base,
                      const Skip& skip, const std::vector<int>& prim_shape, const std::vector<int>& which,
                      std::vector<std::vector<int>>& wpos_of, std::vector<std::vector<int>>* prims_of = nullptr) {
    const size_t M = a.size(), P = prim_shape.size();
    std::vector<int> leaf(P, -1), parent(M, -1), stamp(M, -1);
    TreeSlots t{std::vector<int>(M, -1), std::vector<char>(M, 0)};
    for (size_t j = 0; j < M; ++j) {
        if (a[j] < 0) {
            const int st = -a[j] - 1;
            for (int q = 0; q < b[j]; ++q) leaf[st + q] = static_cast<int>(j);
        } else {
            parent[a[j]] = static_cast<int>(j);
            parent[b[j] & 0x3fffffff] = static_cast<int>(j);
        }
    }
    for (size_t q = 0; q < wchild.size(); ++q)
        if (wchild[q] >= 0 && !skip(wchild[q])) t.wpos[wchild[q]] = static_cast<int>(slot_base + q);
    for (size_t p = 0; p < P; ++p) {
        const int i = which[prim_shape[p]];
        if (i < 0) continue;
        if (prims_of) (*prims_of)[i].push_back(static_cast<int>(p));
        for (int j = leaf[p]; j >= 0; j = parent[j])
            if (t.wpos[j] >= 0 && stamp[j] != i) {
                stamp[j] = i;
                wpos_of[i].push_back(t.wpos[j]);
                t.dirty[j] = 1;
            }
    }
    return t;
}

// Step 1 for refit_ids over the scene (nodes, idx, host_shapes) and, with accel_ok, its
// accelerator A: `state`, the entries' lists, and the slot arrays. anim_base holds, per
// entry, the record the accelerator's bounds and cones were built from. RT_ERR_BVH if a
// local subtree's prims are not contiguous. laps: the caller's "prepare" laps, if any.
inline int plan_refit_slots(const AccelHost& A, bool accel_ok, const FlatNode* nodes, int N, const int* idx, int S,
                            const std::vector<int>& refit_ids, const std::vector<FlatShape>& anim_base,
                            const FlatShape* host_shapes, ShapeCache cache, RefitState state, RefitPlan& out,
                            RefitSlots& sl, PhaseLaps* laps = nullptr) {
    const int n = static_cast<int>(refit_ids.size());
    state.refit_of.assign(S, -1);
    for (int i = 0; i < n; ++i) state.refit_of[refit_ids[i]] = i;
    state.entry_root.clear();
    if (n == 0) return RT_OK;
    const std::vector<int>& which = state.refit_of;  // shape -> refit entry
    state.anim_cls.assign(n, UNBOUNDED);
    for (int i = 0; i < n; ++i) {
        Box3 b;
        state.anim_cls[i] = classify(anim_base[i], b, A.origin_lim, A.mt);
    }
    // reference nodes listing each shape: the leaves that list it and every node above
    // (CSR: a vector per node took ~6 ms of a config-5 setup)
    std::vector<int> poff(static_cast<size_t>(N) + 1, 0), plist;
    for (int k = 0; k < N; ++k) {
        const FlatNode& nd = nodes[k];
        if (nd.leftChild != -1) {
            ++poff[nd.leftChild + 1];
            if (nd.rightChild != nd.leftChild) ++poff[nd.rightChild + 1];
        }
    }
    for (int k = 0; k < N; ++k) poff[k + 1] += poff[k];
    plist.resize(poff[N]);
    {
        std::vector<int> fill(poff.begin(), poff.end() - 1);
        for (int k = 0; k < N; ++k) {
            const FlatNode& nd = nodes[k];
            if (nd.leftChild != -1) {
                plist[fill[nd.leftChild]++] = k;
                if (nd.rightChild != nd.leftChild) plist[fill[nd.rightChild]++] = k;
            }
        }
    }
    using Lists = std::vector<std::vector<int>>;
    Lists &nodes_of = out.nodes_of = Lists(n), &slots_of = out.slots_of = Lists(n), &prims_of = out.prims_of = Lists(n),
          &wpos_of = out.wpos_of = Lists(n);
    std::vector<int> stamp(N, -1);
    for (int k = 0; k < N; ++k) {
        const FlatNode& nd = nodes[k];
        if (nd.leftChild != -1) continue;
        for (int j = nd.startShapeIdx; j < nd.startShapeIdx + nd.numShapes; ++j) {
            const int i = which[idx[j]];
            if (i < 0) continue;
            slots_of[i].push_back(j);
            nodes_of[i].push_back(k);
        }
    }
    for (int i = 0; i < n; ++i) {
        std::vector<int>& L = nodes_of[i];
        std::vector<int> todo;
        for (int k : L)
            if (stamp[k] != i) {
                stamp[k] = i;
                todo.push_back(k);
            }
        L.clear();
        while (!todo.empty()) {
            const int k = todo.back();
            todo.pop_back();
            L.push_back(k);
            for (int q = poff[k]; q < poff[k + 1]; ++q)
                if (const int p = plist[q]; stamp[p] != i) {
                    stamp[p] = i;
                    todo.push_back(p);
                }
        }
        std::sort(L.begin(), L.end());
    }
    lap_of(laps, "nodes_of");
    state.entry_root.assign(n, 0);
    for (int i = 0; i < n; ++i) state.entry_root[i] = std::binary_search(nodes_of[i].begin(), nodes_of[i].end(), N - 1);
    if (accel_ok) {
        out.slots = true;
        const size_t P = A.prim_shape.size();
        std::vector<I4>& work = sl.work;
        auto add_dirty = [&](const TreeSlots& t, const std::vector<int>& first, const std::vector<int>& end) {
            for (size_t j = 0; j < t.dirty.size(); ++j)
                if (t.dirty[j]) work.push_back(I4{t.wpos[j], first[j], end[j], 0});
        };
        const TreeSlots local = slots_above(A.la, A.lb, A.wchild, 0, [](int) { return false; }, A.prim_shape, which, wpos_of, &prims_of);
        lap_of(laps, "local maps");
        // prim range of every local subtree (contiguous: LocalBuilder emits a subtree's prims together)
        std::vector<int> first, end;
        if (!local_prim_ranges(A, first, end)) return RT_ERR_BVH;
        add_dirty(local, first, end);
        lap_of(laps, "local ranges");
        // The scene tree (accel.h SceneTree), refit like the local trees: its wide
        // nodes follow the local ones in lnodes (global slot 4*nw + q), a subtree's
        // prims are contiguous. Its unbounded part (kNoPrune: boxes are the padded
        // reference-leaf boxes, which grow) goes infinite while the set is animated;
        // the items' exact boxes follow the grown leaves (k_refit).
        const SceneTree& T = A.st;
        if (T.wroot >= 0) {
            const size_t nw = A.wchild.size() / kWide;
            const TreeSlots scene = slots_above(T.a, T.b, T.wchild, 4 * nw, [&](int j) { return st_noprune(A, j); }, A.prim_shape, which, wpos_of);
            scene_prim_ranges(T, first, end);
            add_dirty(scene, first, end);
        }
        lap_of(laps, "scene tree maps");
        std::vector<F4>& pb = sl.pb;
        pb.assign(2 * (P ? P : 1), F4{INFINITY, INFINITY, INFINITY, 0.f});
        // per shape its class and box as last classified (the build's, or here for shapes
        // written since: a host rewriting a different 1 % of config 5 every frame had
        // every shape it ever wrote classified again at each change of the set, 11 ms)
        const bool cached = cache.cls.size() == static_cast<size_t>(S) && cache.moved.size() == cache.cls.size();
        for (size_t p = 0; p < P; ++p) {
            Box3 b;
            const int sh = A.prim_shape[p];
            int cls;
            if (cached && !cache.moved[sh]) {
                cls = cache.cls[sh];
                b = cache.box[sh];
            } else {
                cls = classify(host_shapes[sh], b, A.origin_lim, A.mt);
                if (cached) {
                    cache.cls[sh] = cls;
                    cache.box[sh] = b;
                    cache.moved[sh] = 0;
                }
            }
            if (cls != BOUNDED) {
                pb[2 * p + 1] = F4{-INFINITY, -INFINITY, -INFINITY, 0.f};
                continue;
            }
            pb[2 * p] = F4{b.lo[0], b.lo[1], b.lo[2], 0.f};
            pb[2 * p + 1] = F4{b.hi[0], b.hi[1], b.hi[2], 0.f};
        }
        lap_of(laps, "prim boxes (classify)");
        // slots whose refit list takes a wave more than one step (kBigList) first, one
        // workgroup each; the rest kRefitWaves to a workgroup, one wave each (k_refit)
        {
            std::vector<char> big(work.size(), 0);
            for (size_t q = 0; q < work.size(); ++q) {
                int n_ref = 0;
                for (int p = work[q].y; p < work[q].z; ++p) n_ref += which[A.prim_shape[p]] >= 0;
                big[q] = n_ref > kBigList;
            }
            std::vector<I4> ord;
            for (int pass = 1; pass >= 0; --pass)
                for (size_t q = 0; q < work.size(); ++q)
                    if (big[q] == pass) ord.push_back(work[q]);
            out.n_big = static_cast<int>(std::count(big.begin(), big.end(), 1));
            work.swap(ord);
        }
        // per dirty slot: the box of its prims outside the refit set (they never move
        // while this set stands) and the list of those in it, which k_refit unions per frame
        std::vector<F4>& st = sl.st;
        std::vector<int>& dl = sl.dl;
        st.assign(2 * (work.empty() ? 1 : work.size()), F4{0.f, 0.f, 0.f, 0.f});
        for (size_t q = 0; q < work.size(); ++q) {
            I4& w4 = work[q];
            out.dirty_max = std::max(out.dirty_max, w4.z - w4.y);
            out.dirty_sum += w4.z - w4.y;
            w4.w = static_cast<int>(dl.size());
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int p = w4.y; p < w4.z; ++p) {
                if (which[A.prim_shape[p]] >= 0) {
                    dl.push_back(p);
                    continue;
                }
                const F4 a = pb[2 * static_cast<size_t>(p)], b = pb[2 * static_cast<size_t>(p) + 1];
                lo[0] = std::min(lo[0], a.x), lo[1] = std::min(lo[1], a.y), lo[2] = std::min(lo[2], a.z);
                hi[0] = std::max(hi[0], b.x), hi[1] = std::max(hi[1], b.y), hi[2] = std::max(hi[2], b.z);
            }
            st[2 * q] = F4{lo[0], lo[1], lo[2], 0.f};
            st[2 * q + 1] = F4{hi[0], hi[1], hi[2], 0.f};
        }
        lap_of(laps, "slot static boxes");
        out.n_dirty = static_cast<int>(work.size());
        out.n_direct_slot_reads = static_cast<long long>(dl.size());
        work.push_back(I4{0, 0, 0, static_cast<int>(dl.size())});  // the end of the last list
        if (dl.empty()) dl.push_back(0);
    }
    return RT_OK;
}

// Step 2: the CSR buffer behind AnimMaps, from step 1's entry lists. titem_ref: per titems
// record its reference leaf (empty: none).
inline void plan_refit_lists(const AccelHost& A, bool accel_ok, const FlatNode* nodes, int N, const std::vector<int>& refit_ids,
                             const std::vector<int>& titem_ref, RefitState state, RefitPlan& out) {
    const int n = static_cast<int>(refit_ids.size());
    const auto &nodes_of = out.nodes_of, &slots_of = out.slots_of, &prims_of = out.prims_of, &wpos_of = out.wpos_of;
    // one int array: ids, then (offsets, list) x 6, node ids, classes, prim entries
    std::vector<int>& buf = out.buf;
    buf = refit_ids;
    auto append = [&](const std::vector<std::vector<int>>& lists, size_t& off_at, size_t& list_at) {
        off_at = buf.size();
        int run = 0;
        buf.push_back(0);
        for (const auto& l : lists) buf.push_back(run += static_cast<int>(l.size()));
        list_at = buf.size();
        for (const auto& l : lists) buf.insert(buf.end(), l.begin(), l.end());
    };
    // per reference node, the animated shapes it lists (k_refit's node role)
    std::vector<int> node_ids;
    std::vector<std::vector<int>> lists_of;
    std::vector<int> slot(N, -1);  // reference node -> its place in node_ids
    for (int i = 0; i < n; ++i)
        for (int k : nodes_of[i]) {
            if (slot[k] < 0) {
                slot[k] = static_cast<int>(node_ids.size());
                node_ids.push_back(k);
                lists_of.emplace_back();
            }
            lists_of[slot[k]].push_back(i);
        }
    // per grown node, where its box is copied (k_refit writes them through): the
    // wnodes child slots of its parent(s) and the scene-tree items it gates
    std::vector<std::vector<int>> wn_of(node_ids.size()), items_of(node_ids.size());
    for (int p = 0; p < N; ++p) {
        const FlatNode& nd = nodes[p];
        if (nd.leftChild == -1) continue;
        if (slot[nd.leftChild] >= 0) wn_of[slot[nd.leftChild]].push_back(2 * p);
        if (slot[nd.rightChild] >= 0) wn_of[slot[nd.rightChild]].push_back(2 * p + 1);
    }
    for (size_t i = 0; i < titem_ref.size(); ++i) {
        const int k = titem_ref[i];
        if (k >= 0 && k < N && slot[k] >= 0) items_of[slot[k]].push_back(static_cast<int>(i));
    }
    RefitOffsets& o = out.o;
    append(slots_of, o.slot_off, o.slot_list);
    append(prims_of, o.prim_off, o.prim_list);
    append(wpos_of, o.wpos_off, o.wpos_list);
    append(lists_of, o.node_off, o.node_list);
    out.direct_reads = n + out.n_direct_slot_reads;
    for (const auto& l : lists_of) out.direct_reads += static_cast<long long>(l.size());
    append(wn_of, o.wn_off, o.wn_list);
    append(items_of, o.item_off, o.item_list);
    o.node_ids = buf.size();
    buf.insert(buf.end(), node_ids.begin(), node_ids.end());
    o.ecls = buf.size();
    buf.insert(buf.end(), state.anim_cls.begin(), state.anim_cls.end());
    o.prim_entry = buf.size();
    for (size_t p = 0; p < (accel_ok ? A.prim_shape.size() : 0); ++p) buf.push_back(state.refit_of[A.prim_shape[p]]);
    out.n_nodes = static_cast<int>(node_ids.size());
}

// Both steps (the tests' entry point).
inline int plan_refit(const AccelHost& A, bool accel_ok, const FlatNode* nodes, int N, const int* idx, int S,
                      const std::vector<int>& refit_ids, const std::vector<FlatShape>& anim_base, const FlatShape* host_shapes,
                      ShapeCache cache, RefitState state, const std::vector<int>& titem_ref, RefitPlan& out, RefitSlots& sl) {
    const int rc = plan_refit_slots(A, accel_ok, nodes, N, idx, S, refit_ids, anim_base, host_shapes, cache, state, out, sl);
    if (rc == RT_OK && !refit_ids.empty()) plan_refit_lists(A, accel_ok, nodes, N, refit_ids, titem_ref, state, out);
    return rc;
}

}  // namespace rta
