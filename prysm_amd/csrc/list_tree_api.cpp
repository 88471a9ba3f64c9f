// The device-resident list tree: merkleHash (hash.go:194-239) of a list whose
// levels stay in HBM -- build, update from the changed items only and the
// mk_*list_tree* entry points.  The mk_list_tree handle is
// tree_handle.cpp's, with kListKind.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

struct mk_list_tree : TreeHandle {};

namespace {

// The handle rebuilds instead of climbing when count / MK_LIST_TREE_REBUILD_DIV <= dirty:
// on the 2^24 x 32-B list an update of 2^15 random items (0.865 ms) is the
// largest power of two still cheaper than a build (0.961 ms), 2^16 costs
// 1.572 ms: a dirty fraction of 2^15 / 2^24 = 1/512 (tools/list_tree_probe.py,
// profiles/list_tree/probe.json).
#define MK_LIST_TREE_REBUILD_DIV 512

uint64_t lt_per(uint32_t item_len) { return item_len < 128 ? 128 / item_len : 1; }
uint64_t lt_chunks(uint64_t n, uint32_t item_len) { return ceil_div(n, lt_per(item_len)); }

// nodes of all levels 1 .. D of a tree with room for cap_chunks chunks
uint64_t lt_levels_nodes(uint64_t cap_chunks) {
    uint64_t sum = 0;
    for (uint64_t c = cap_chunks; c > 1;) {
        c = (c + 1) / 2;
        sum += c;
    }
    return sum;
}

uint64_t lt_update_ws(uint64_t k) { return align256(8 * std::max<uint64_t>(k, 1)); }

int lt_check(uint64_t n, uint64_t capacity, uint32_t item_len) {
    if (item_len == 0) return fail(MK_EINVAL, "item_len == 0");
    if (item_len > (1u << 30)) return fail(MK_EINVAL, "item_len %u above 2^30", item_len);
    if (n > capacity)
        return fail(MK_EINVAL, "%llu items > capacity %llu", (unsigned long long)n, (unsigned long long)capacity);
    if (capacity > UINT64_MAX / item_len) return fail(MK_EINVAL, "capacity * item_len overflows");
    return MK_OK;
}

int launch_update(const void* d_items, void* d_levels, const uint64_t* d_idx, uint64_t k_idx, uint64_t n_old,
                  uint64_t n_new, uint64_t capacity, uint32_t item_len, void* d_root32, void* d_ws, hipStream_t st) {
    const uint64_t T = k_idx + (n_new - n_old);
    const mk::ListTreeArgs a =
        list_tree_args(d_items, d_levels, d_idx, k_idx, n_old, n_new, capacity, item_len, d_root32, d_ws);
    HIPCHK(hipMemsetAsync(d_ws, 0, 8 * std::max<uint64_t>(T, 1), st));
    hipLaunchKernelGGL(mk::k_list_tree_update, dim3(std::max<uint64_t>(ceil_div(2 * T, 256), 1)), dim3(256), 0, st, a);
    return launched();
}

// Every level and the root of n items.  One batched launch per level over
// all parents but the last (complete pairs: 2 chunk_bytes-byte messages out
// of the item buffer, then 64-B messages out of the level below; the last
// node of a level is never an input of those), then the right edge -- the
// ragged or padded last node of every level -- by the update kernel run on
// "the last item is dirty".
int dev_build(const void* d_items, uint64_t n, uint64_t capacity, uint32_t item_len, void* d_levels, void* d_root32,
              void* d_ws, hipStream_t st) {
    const uint64_t nch = lt_chunks(n, item_len);
    if (nch <= 1) {  // the top is the raw chunk (0^128 for an empty list): no levels
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)d_items, n * item_len, n,
                           (uint8_t*)d_root32);
        return launched();
    }
    const uint64_t cb = lt_per(item_len) * item_len;
    uint8_t* lv = (uint8_t*)d_levels;
    const uint8_t* in = (const uint8_t*)d_items;
    uint32_t msg = (uint32_t)(2 * cb);
    uint64_t capd = (lt_chunks(capacity, item_len) + 1) / 2;
    for (uint64_t c = nch; c > 1; c = (c + 1) / 2) {
        TRY(dev_hash_batch(in, (c + 1) / 2 - 1, msg, lv, st));
        in = lv;
        lv += 32 * capd;
        capd = (capd + 1) / 2;
        msg = 64;
    }
    return launch_update(d_items, d_levels, nullptr, 0, n - 1, n, capacity, item_len, d_root32, d_ws, st);
}

int dev_update(void* d_items, uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len, void* d_levels,
               const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_root32, void* d_ws,
               hipStream_t st) {
    if (d_values) TRY(list_tree_scatter(d_items, d_idx, k_idx, n_old, n_new - n_old, item_len, d_values, st));
    if (lt_chunks(n_new, item_len) <= 1) {
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)d_items, n_new * item_len,
                           n_new, (uint8_t*)d_root32);
        return launched();
    }
    return launch_update(d_items, d_levels, d_idx, k_idx, n_old, n_new, capacity, item_len, d_root32, d_ws, st);
}

// ---- what the handle (tree_handle.cpp) needs of this kind ----------------------------------
const TreeKind kListKind = {
    "list tree", "items", MK_LIST_TREE_REBUILD_DIV, false, lt_check,
    [](const TreeHandle&, uint64_t) { return lt_update_ws(1); },
    [](const TreeHandle&, uint64_t k) { return lt_update_ws(k); },
    nullptr,
    [](const TreeHandle& t, uint64_t n, hipStream_t st) {
        return dev_build(t.items.p, n, t.cap, t.item_len, t.levels.p, t.root.p, t.ws.p, st);
    },
    [](const TreeHandle& t, uint64_t n_old, uint64_t n_new, const uint64_t* d_idx, uint64_t k_idx,
       const void* d_values, hipStream_t st) {
        return dev_update(t.items.p, n_old, n_new, t.cap, t.item_len, t.levels.p, d_idx, k_idx, d_values, t.root.p,
                          t.ws.p, st);
    },
    MK_TREE_LIST,
    [](const TreeHandle&) -> TreeHandle* { return new (std::nothrow) mk_list_tree(); },
    [](const TreeHandle&, const TreeHandle&) { return true; },
};

}  // namespace

namespace mk::rt {
// what the registry tree (struct_tree_api.cpp) runs over its buffer of 32-B struct roots
int list_tree_build32(const void* d_roots, uint64_t n, uint64_t capacity, void* d_levels, void* d_root32, void* d_ws,
                      hipStream_t st) {
    return dev_build(d_roots, n, capacity, 32, d_levels, d_root32, d_ws, st);
}
int list_tree_update32(const void* d_roots, void* d_levels, const uint64_t* d_idx, uint64_t k_idx, uint64_t n_old,
                       uint64_t n_new, uint64_t capacity, void* d_root32, void* d_ws, hipStream_t st) {
    return launch_update(d_roots, d_levels, d_idx, k_idx, n_old, n_new, capacity, 32, d_root32, d_ws, st);
}

int list_tree_scatter(void* d_items, const uint64_t* d_idx, uint64_t k_idx, uint64_t n_old, uint64_t n_app,
                      uint32_t item_len, const void* d_values, hipStream_t st) {
    if (k_idx + n_app == 0) return MK_OK;
    const bool w8 = item_len % 8 == 0 && ((uintptr_t)d_items % 8) == 0 && ((uintptr_t)d_values % 8) == 0;
    const uint32_t unit = w8 ? 8 : 1;
    const uint64_t threads = (k_idx + n_app) * (item_len / unit);
    hipLaunchKernelGGL(mk::k_list_tree_scatter, dim3(ceil_div(threads, 256)), dim3(256), 0, st, (uint8_t*)d_items,
                       d_idx, k_idx, n_old, n_app, item_len, unit, (const uint8_t*)d_values);
    return launched();
}

// The list tree's part of mk_dev_ssz_trees_update (its stage 0 is list_tree_scatter alone).
// host-checkable arguments of mk_dev_ssz_list_tree_update (no device needed)
int list_tree_check_update(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len, uint64_t k_idx,
                           uint64_t ws_bytes) {
    if (item_len == 0) return fail(MK_EINVAL, "item_len == 0");
    if (n_new < n_old)
        return fail(MK_EINVAL, "n_new %llu < n_old %llu (a list tree does not shrink)", (unsigned long long)n_new,
                    (unsigned long long)n_old);
    TRY(lt_check(n_new, capacity, item_len));
    if (k_idx >= kMaxWork) return fail(MK_EINVAL, "%llu indices in one call", (unsigned long long)k_idx);
    const uint64_t T = k_idx + (n_new - n_old);
    if (T >= kMaxWork) return fail(MK_EINVAL, "%llu dirty items in one call (limit 2^31 - 1)", (unsigned long long)T);
    if (ws_bytes < lt_update_ws(T)) return fail(MK_ENOMEM, "workspace too small");
    return MK_OK;
}

int list_tree_check_ptrs(const void* d_items, uint64_t n, uint64_t capacity, uint32_t item_len, const void* d_levels,
                         const void* d_root32, const void* d_ws) {
    if (!d_root32 || !d_ws || (n && !d_items)) return fail(MK_EINVAL, "null pointer");
    if (lt_chunks(capacity, item_len) > 1 && !d_levels) return fail(MK_EINVAL, "null level array");
    if (((uintptr_t)d_levels % 16) || ((uintptr_t)d_root32 % 4) || ((uintptr_t)d_ws % 8))
        return fail(MK_EINVAL, "level array (16 B), root (4 B) or workspace (8 B) misaligned");
    return MK_OK;
}

// the climb's descriptor (k_list_tree_update, one slice of k_trees_update); d_arrive: zeroed arrival words
mk::ListTreeArgs list_tree_args(const void* d_items, void* d_levels, const uint64_t* d_idx, uint64_t k_idx,
                                uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len, void* d_root32,
                                void* d_arrive) {
    mk::ListTreeArgs a{};
    a.items = (const uint8_t*)d_items;
    a.levels = (uint32_t*)d_levels;
    a.idx = d_idx;
    a.k_idx = k_idx;
    a.n_old = n_old;
    a.n_new = n_new;
    a.cap_chunks = lt_chunks(capacity, item_len);
    a.item_len = item_len;
    a.per = (uint32_t)lt_per(item_len);
    a.arrive = (uint64_t*)d_arrive;
    a.root_out = (uint32_t*)d_root32;
    return a;
}

TreeHandle* list_tree_handle() { return new (std::nothrow) mk_list_tree(); }
const TreeKind& list_tree_kind() { return kListKind; }

// ---- shrinking a resident tree of any kind ------------------------------------
// A shrink rebuilds the levels (from level 0, never from the records) instead
// of climbing when n_new / MK_TREE_SHRINK_REBUILD_DIV <= dirty, dirty the
// suffix [first, n_new).  Its climb has no stage 0 and its dirty values are
// one suffix that shares its ancestors, so the kinds' own divisors (512, 32,
// 256: random indices, stage 0 included) are not its break-even: on 2^20 x
// 32-B items the climb over a suffix of 2^14 costs 0.312 ms, the level build
// 0.340 ms, a suffix of 2^16 0.573 ms -- a dirty share of 2^14 / 2^20 = 1/64,
// the same for the three kinds, whose levels are this one tree
// (tools/tree_shrink_probe.py, profiles/tree_shrink/probe.json).
#define MK_TREE_SHRINK_REBUILD_DIV 64
// Regions of the erase workspace for `moved` values: the climb's arrival words
// (at most max(moved, 1) work items), the moved values, the moved level 0.
namespace {
struct ShrinkWs {
    uint64_t vals, l0, total;
};
ShrinkWs shrink_ws(uint64_t moved, uint32_t item_len, bool level0) {
    ShrinkWs w{};
    w.vals = lt_update_ws(moved);
    w.l0 = w.vals + align256(moved * item_len);
    w.total = w.l0 + (level0 ? align256(32 * moved) : 0);
    return w;
}
uint32_t compact_unit(uint32_t item_len, const void* a, const void* b) {
    for (uint32_t u : {16u, 8u, 4u})
        if (item_len % u == 0 && ((uintptr_t)a % u) == 0 && ((uintptr_t)b % u) == 0) return u;
    return 1;
}
}  // namespace

uint64_t tree_shrink_ws(const TreeKind& K, uint64_t moved, uint32_t item_len) {
    if (item_len == 0 || moved >= kMaxWork) return 0;
    return shrink_ws(moved, item_len, K.level0).total;
}

int tree_shrink_check(const TreeKind& K, uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len,
                      uint64_t k_rm, uint64_t first, uint64_t ws_bytes) {
    TRY(K.check_shape(n_old, capacity, item_len));
    if (k_rm > n_old)
        return fail(MK_EINVAL, "%llu removed indices of %llu %s", (unsigned long long)k_rm, (unsigned long long)n_old,
                    K.noun);
    if (n_new > n_old)
        return fail(MK_EINVAL, "n_new %llu > n_old %llu (an erase does not grow the list)", (unsigned long long)n_new,
                    (unsigned long long)n_old);
    if (k_rm && n_new != n_old - k_rm)
        return fail(MK_EINVAL, "n_new %llu is not n_old %llu less the %llu removed %s", (unsigned long long)n_new,
                    (unsigned long long)n_old, (unsigned long long)k_rm, K.noun);
    if (first > n_new)
        return fail(MK_EINVAL, "first %llu beyond the %llu %s that stay", (unsigned long long)first,
                    (unsigned long long)n_new, K.noun);
    const uint64_t moved = k_rm ? n_new - first : 0;
    if (moved >= kMaxWork)
        return fail(MK_EINVAL, "%llu %s to move in one call (limit 2^31 - 1)", (unsigned long long)moved, K.noun);
    if (ceil_div(moved * std::max<uint32_t>(item_len, 32), 256) >= kMaxWork)
        return fail(MK_EINVAL, "%llu %s of %u bytes to move in one call", (unsigned long long)moved, K.noun, item_len);
    if (ws_bytes < shrink_ws(moved, item_len, K.level0).total) return fail(MK_ENOMEM, "workspace too small");
    return MK_OK;
}

// Values [first, n_new) and their level-0 entries take the survivors' (out of
// place into the workspace, then back: a destination below its source may be
// another block's source), then the tree over level 0 as it stands: nothing of
// a survivor is hashed again.  The climb needs no index list: the dirty values
// are the suffix [from, n_new), which lt_update takes as appended ones, and
// every count, pad and the top level come from n_new alone, so the stale nodes
// to the right of the new end are never read (§5k).
int tree_shrink(const TreeKind& K, void* d_items, uint32_t item_len, void* d_level0, void* d_levels, uint64_t n_old,
                uint64_t n_new, uint64_t capacity, const uint64_t* d_rm, uint64_t k_rm, uint64_t first,
                void* d_root32, void* d_ws, hipStream_t st) {
    (void)n_old;
    const uint64_t moved = k_rm ? n_new - first : 0;
    if (moved) {
        const ShrinkWs w = shrink_ws(moved, item_len, K.level0);
        uint8_t* items = (uint8_t*)d_items + first * item_len;
        uint8_t* l0 = K.level0 ? (uint8_t*)d_level0 + 32 * first : nullptr;
        uint8_t* wv = (uint8_t*)d_ws + w.vals;
        uint8_t* wl = (uint8_t*)d_ws + w.l0;
        mk::CompactArgs a{};
        a.s[0] = {items, wv, item_len, compact_unit(item_len, items, wv)};
        a.s[1] = {l0, wl, 32, compact_unit(32, l0, wl)};
        a.rm = d_rm;
        a.k_rm = k_rm;
        a.first = first;
        a.moved = moved;
        const uint64_t p0 = moved * (item_len / a.s[0].unit), p1 = K.level0 ? moved * (32 / a.s[1].unit) : 0;
        const dim3 grid((uint32_t)ceil_div(std::max(p0, p1), 256), K.level0 ? 2 : 1);
        hipLaunchKernelGGL(mk::k_tree_compact, grid, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        a.s[0].src = wv, a.s[0].dst = items;  // the moved range back in place
        a.s[1].src = wl, a.s[1].dst = l0;
        a.k_rm = 0;
        hipLaunchKernelGGL(mk::k_tree_compact, grid, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
    }
    const void* leaves = K.level0 ? d_level0 : d_items;
    const uint32_t leaf_len = K.level0 ? 32 : item_len;
    if (lt_chunks(n_new, leaf_len) <= 1) {  // no levels: the mix-in over the raw chunk (0^128 when empty)
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)leaves, n_new * leaf_len,
                           n_new, (uint8_t*)d_root32);
        return launched();
    }
    // a truncate: the last value that stays is dirty, as the build's right edge
    const uint64_t from = k_rm ? std::min(first, n_new - 1) : n_new - 1;
    if (n_new / MK_TREE_SHRINK_REBUILD_DIV <= n_new - from)  // the climb does not pay: every level, from level 0
        return dev_build(leaves, n_new, capacity, leaf_len, d_levels, d_root32, d_ws, st);
    return launch_update(leaves, d_levels, nullptr, 0, from, n_new, capacity, leaf_len, d_root32, d_ws, st);
}
}  // namespace mk::rt

extern "C" {

uint64_t mk_ssz_list_tree_levels_bytes(uint64_t capacity, uint32_t item_len) {
    if (item_len == 0) return 0;
    return 32 * lt_levels_nodes(lt_chunks(capacity, item_len));
}

uint64_t mk_ssz_list_tree_build_workspace_bytes(uint64_t n, uint32_t item_len) {
    (void)n;
    (void)item_len;
    return lt_update_ws(1);  // the right edge's one arrival word
}

uint64_t mk_ssz_list_tree_update_workspace_bytes(uint64_t k) { return lt_update_ws(k); }

// The argument checks come before the stream's device is looked up: a bad
// call is MK_EINVAL on any machine.
int mk_dev_ssz_list_tree_build(mk_call* call, const void* d_items, uint64_t n, uint64_t capacity, uint32_t item_len,
                               void* d_levels, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream) {
    Scope S(call);
    int rc = lt_check(n, capacity, item_len);
    if (!rc && ws_bytes < lt_update_ws(1)) rc = fail(MK_ENOMEM, "workspace too small");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = list_tree_check_ptrs(d_items, n, capacity, item_len, d_levels, d_root32, d_ws);
    if (!rc) rc = dev_build(d_items, n, capacity, item_len, d_levels, d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_dev_ssz_list_tree_update(mk_call* call, void* d_items, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                uint32_t item_len, void* d_levels, const uint64_t* d_idx, uint64_t k_idx,
                                const void* d_values, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream) {
    Scope S(call);
    int rc = list_tree_check_update(n_old, n_new, capacity, item_len, k_idx, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = list_tree_check_ptrs(d_items, n_new, capacity, item_len, d_levels, d_root32, d_ws);
    if (!rc && k_idx && (!d_idx || ((uintptr_t)d_idx % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc)
        rc = dev_update(d_items, n_old, n_new, capacity, item_len, d_levels, d_idx, k_idx, d_values, d_root32, d_ws,
                        (hipStream_t)stream);
    return S.done(rc);
}

uint64_t mk_ssz_list_tree_erase_workspace_bytes(uint64_t moved, uint32_t item_len) {
    return tree_shrink_ws(kListKind, moved, item_len);
}

// Every argument check comes before the stream's device is looked up.
int mk_dev_ssz_list_tree_erase(mk_call* call, void* d_items, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                               uint32_t item_len, void* d_levels, const uint64_t* d_rm, uint64_t k_rm, uint64_t first,
                               void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream) {
    Scope S(call);
    int rc = tree_shrink_check(kListKind, n_old, n_new, capacity, item_len, k_rm, first, ws_bytes);
    if (!rc) rc = list_tree_check_ptrs(d_items, n_old, capacity, item_len, d_levels, d_root32, d_ws);
    if (!rc && k_rm && (!d_rm || ((uintptr_t)d_rm % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = tree_shrink(kListKind, d_items, item_len, nullptr, d_levels, n_old, n_new, capacity, d_rm, k_rm, first,
                         d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_list_tree_new(mk_call* call, uint32_t item_len, uint64_t capacity, mk_list_tree** out) {
    Scope S(call);
    if (!out) return S.done(fail(MK_EINVAL, "null pointer"));
    *out = nullptr;
    int rc = lt_check(0, std::max<uint64_t>(capacity, 1), item_len);
    if (!rc) rc = bind_call();
    if (rc) return S.done(rc);
    auto* t = new (std::nothrow) mk_list_tree();
    rc = tree_new(t, kListKind, item_len, capacity);
    if (!rc) *out = t;
    return S.done(rc);
}

void mk_list_tree_free(mk_list_tree* t) { tree_free(t); }

uint64_t mk_list_tree_count(const mk_list_tree* t) { return t ? t->count : 0; }

int mk_list_tree_assign(mk_call* call, mk_list_tree* t, const uint8_t* items, uint64_t n) {
    Scope S(call);
    return S.done(tree_assign(t, items, n));
}

int mk_list_tree_update(mk_call* call, mk_list_tree* t, const uint64_t* idx, const uint8_t* values, uint64_t k) {
    Scope S(call);
    return S.done(tree_update(t, idx, values, k));
}

int mk_list_tree_append(mk_call* call, mk_list_tree* t, const uint8_t* items, uint64_t k) {
    Scope S(call);
    return S.done(tree_append(t, items, k));
}

int mk_list_tree_truncate(mk_call* call, mk_list_tree* t, uint64_t n) {
    Scope S(call);
    return S.done(tree_truncate(t, n));
}

int mk_list_tree_erase(mk_call* call, mk_list_tree* t, const uint64_t* idx, uint64_t k) {
    Scope S(call);
    return S.done(tree_erase(t, idx, k));
}

int mk_list_tree_root(mk_call* call, mk_list_tree* t, uint8_t root[32]) {
    Scope S(call);
    return S.done(tree_root(t, root));
}

int mk_list_tree_items(mk_call* call, mk_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(tree_read(t, first, cnt, out));
}

int mk_list_tree_branches(mk_call* call, mk_list_tree* t, const uint64_t* idx, uint64_t k, uint8_t* values_out,
                          uint8_t* branches_out) {
    Scope S(call);
    return S.done(tree_branches(t, idx, k, values_out, branches_out));
}

int mk_list_tree_clone(mk_call* call, mk_list_tree* src, mk_list_tree** out) {
    Scope S(call);
    TreeHandle* t = nullptr;
    const int rc = out ? tree_clone(src, &t) : fail(MK_EINVAL, "null pointer");
    if (out) *out = static_cast<mk_list_tree*>(t);
    return S.done(rc);
}

int mk_list_tree_copy(mk_call* call, mk_list_tree* dst, mk_list_tree* src) {
    Scope S(call);
    return S.done(tree_copy(dst, src));
}

int mk_list_tree_reserve(mk_call* call, mk_list_tree* t, uint64_t capacity) {
    Scope S(call);
    return S.done(tree_reserve(t, capacity));
}

uint64_t mk_list_tree_capacity(const mk_list_tree* t) { return t ? t->cap : 0; }

int mk_list_tree_audit(mk_call* call, mk_list_tree* t, mk_audit_report* out) {
    Scope S(call);
    return S.done(tree_audit(t, out));
}

int mk_list_tree_diff(mk_call* call, mk_list_tree* a, mk_list_tree* b, uint64_t* idx_out,
                      uint64_t max_out, uint64_t* total, uint64_t* n_a, uint64_t* n_b) {
    Scope S(call);
    return S.done(tree_diff(a, b, idx_out, max_out, total, n_a, n_b));
}

}  // extern "C"
