// The device-resident tree of a list of byte strings: TreeHash of a [][N]byte
// (hash.go:100-107, 118-139, 194-239) whose elements, element digests
// K(le32(elem_len) || e_i) and levels stay in HBM -- build, update from the
// changed elements only and the mk_*bytes_list_tree* entry points (DESIGN.md
// §5f).  The tree over the 32-B digests is the list tree's (list_tree_api.cpp,
// §5d); the mk_bytes_list_tree handle is tree_handle.cpp's, with kBytesKind.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

struct mk_bytes_list_tree : TreeHandle {};  // item_len: the element length, level0: the digests

namespace {

// The handle rebuilds instead of climbing when count / MK_BYTES_TREE_REBUILD_DIV <= dirty:
// on the 2^24 x 32-B list an update of 2^16 random elements (1.599 ms) is the
// largest power of two still cheaper than a build (2.519 ms), 2^17 costs
// 2.930 ms: a dirty share of 2^16 / 2^24 = 1/256 (tools/bytes_tree_probe.py,
// profiles/bytes_tree/probe.json).
#define MK_BYTES_TREE_REBUILD_DIV 256

uint64_t bt_chunks(uint64_t n) { return ceil_div(n, 4); }  // 4 digests per chunk

uint64_t build_ws() { return 256; }  // the right edge's one arrival word
// the list tree's arrival words, one per work item
uint64_t update_ws(uint64_t k) { return align256(8 * std::max<uint64_t>(k, 1)); }

// host-checkable arguments (no device needed)
int check_shape(uint64_t n, uint64_t capacity, uint32_t elem_len) {
    if (elem_len == 0) return fail(MK_EINVAL, "elem_len == 0");
    if (elem_len > (1u << 30)) return fail(MK_EINVAL, "elem_len %u above 2^30", elem_len);
    if (n > capacity)
        return fail(MK_EINVAL, "%llu elements > capacity %llu", (unsigned long long)n, (unsigned long long)capacity);
    if (capacity > UINT64_MAX / std::max<uint32_t>(elem_len, 32))
        return fail(MK_EINVAL, "capacity * elem_len overflows");
    return MK_OK;
}

// every element digest, then every level and the root
int dev_build(const void* d_elems, uint64_t n, uint64_t capacity, uint32_t elem_len, void* d_digests, void* d_levels,
              void* d_root32, void* d_ws, hipStream_t st) {
    TRY(launch_elem_digests(d_elems, n, elem_len, d_digests, st));
    return list_tree_build32(d_digests, n, capacity, d_levels, d_root32, d_ws, st);
}

int dev_update(void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t elem_len, void* d_digests,
               void* d_levels, const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_root32,
               void* d_ws, hipStream_t st) {
    TRY(bytes_tree_stage0(d_elems, n_old, n_new, elem_len, d_digests, d_idx, k_idx, d_values, st));
    if (bt_chunks(n_new) <= 1) {  // one chunk, no levels: the mix-in over the raw chunk of digests
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)d_digests, 32 * n_new, n_new,
                           (uint8_t*)d_root32);
        return launched();
    }
    // the list tree's update (with nothing changed: the root again, from the stored top node)
    return list_tree_update32(d_digests, d_levels, d_idx, k_idx, n_old, n_new, capacity, d_root32, d_ws, st);
}

// ---- what the handle (tree_handle.cpp) needs of this kind ----------------------------------
const TreeKind kBytesKind = {
    "bytes tree", "elements", MK_BYTES_TREE_REBUILD_DIV, true, check_shape,
    [](const TreeHandle&, uint64_t) { return build_ws(); },
    [](const TreeHandle&, uint64_t k) { return update_ws(k); },
    nullptr,
    [](const TreeHandle& t, uint64_t n, hipStream_t st) {
        return dev_build(t.items.p, n, t.cap, t.item_len, t.level0.p, t.levels.p, t.root.p, t.ws.p, st);
    },
    [](const TreeHandle& t, uint64_t n_old, uint64_t n_new, const uint64_t* d_idx, uint64_t k_idx,
       const void* d_values, hipStream_t st) {
        return dev_update(t.items.p, n_old, n_new, t.cap, t.item_len, t.level0.p, t.levels.p, d_idx, k_idx, d_values,
                          t.root.p, t.ws.p, st);
    },
    MK_TREE_BYTES,
    [](const TreeHandle&) -> TreeHandle* { return new (std::nothrow) mk_bytes_list_tree(); },
    [](const TreeHandle&, const TreeHandle&) { return true; },
};

}  // namespace

// the bytes tree's part of mk_dev_ssz_trees_update (tree_many_api.cpp)
namespace mk::rt {
int bytes_tree_check_update(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t elem_len, uint64_t k_idx,
                            uint64_t ws_bytes) {
    if (elem_len == 0) return fail(MK_EINVAL, "elem_len == 0");
    if (n_new < n_old)
        return fail(MK_EINVAL, "n_new %llu < n_old %llu (a bytes tree does not shrink)", (unsigned long long)n_new,
                    (unsigned long long)n_old);
    TRY(check_shape(n_new, capacity, elem_len));
    if (k_idx >= kMaxWork) return fail(MK_EINVAL, "%llu indices in one call", (unsigned long long)k_idx);
    const uint64_t T = k_idx + (n_new - n_old);
    if (T >= kMaxWork)
        return fail(MK_EINVAL, "%llu dirty elements in one call (limit 2^31 - 1)", (unsigned long long)T);
    if (ws_bytes < update_ws(T)) return fail(MK_ENOMEM, "workspace too small");
    return MK_OK;
}

int bytes_tree_check_ptrs(const void* d_elems, uint64_t n, uint64_t capacity, const void* d_digests,
                          const void* d_levels, const void* d_root32, const void* d_ws) {
    if (!d_digests || !d_root32 || !d_ws || (n && !d_elems)) return fail(MK_EINVAL, "null pointer");
    if (bt_chunks(capacity) > 1 && !d_levels) return fail(MK_EINVAL, "null level array");
    if (((uintptr_t)d_digests % 16) || ((uintptr_t)d_levels % 16) || ((uintptr_t)d_root32 % 4) ||
        ((uintptr_t)d_ws % 8))
        return fail(MK_EINVAL, "digests (16 B), level array (16 B), root (4 B) or workspace (8 B) misaligned");
    return MK_OK;
}

// Stage 0 of an update, everything before the climb: the new elements
// scattered in, then level 0 (d_digests) brought up to date -- every digest
// again for a list of one chunk (it has no levels), else the dirty elements'
// digests, read in place and stored into level 0.  (Digest and climb in one
// launch -- the level-1 owner pairs digesting their own elements -- were built
// and measured no faster at any k: DESIGN.md §5f.)
int bytes_tree_stage0(void* d_elems, uint64_t n_old, uint64_t n_new, uint32_t elem_len, void* d_digests,
                      const uint64_t* d_idx, uint64_t k_idx, const void* d_values, hipStream_t st) {
    const uint64_t n_app = n_new - n_old, T = k_idx + n_app;
    if (d_values) TRY(list_tree_scatter(d_elems, d_idx, k_idx, n_old, n_app, elem_len, d_values, st));
    if (bt_chunks(n_new) <= 1) return launch_elem_digests(d_elems, n_new, elem_len, d_digests, st);
    if (T == 0) return MK_OK;  // nothing changed
    const uint32_t fast32 = elem_len == 32 && ((uintptr_t)d_elems % 16) == 0;
    hipLaunchKernelGGL(mk::k_bytes_tree_digest, dim3(ceil_div(T, 256)), dim3(256), 0, st, (const uint8_t*)d_elems,
                       elem_len, fast32, d_idx, k_idx, n_old, n_app, (uint4*)d_digests);
    return launched();
}

TreeHandle* bytes_tree_handle() { return new (std::nothrow) mk_bytes_list_tree(); }
const TreeKind& bytes_tree_kind() { return kBytesKind; }
}  // namespace mk::rt

extern "C" {

uint64_t mk_ssz_bytes_list_tree_build_workspace_bytes(uint64_t n, uint32_t elem_len) {
    (void)n;
    return elem_len ? build_ws() : 0;
}

uint64_t mk_ssz_bytes_list_tree_update_workspace_bytes(uint64_t k, uint32_t elem_len) {
    return elem_len ? update_ws(k) : 0;
}

// The argument checks come before the stream's device is looked up: a bad
// call is MK_EINVAL / MK_ENOMEM on any machine.
int mk_dev_ssz_bytes_list_tree_build(mk_call* call, const void* d_elems, uint64_t n, uint64_t capacity,
                                     uint32_t elem_len, void* d_digests, void* d_levels, void* d_root32, void* d_ws,
                                     uint64_t ws_bytes, void* stream) {
    Scope S(call);
    int rc = check_shape(n, capacity, elem_len);
    if (!rc && ws_bytes < build_ws()) rc = fail(MK_ENOMEM, "workspace too small");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = bytes_tree_check_ptrs(d_elems, n, capacity, d_digests, d_levels, d_root32, d_ws);
    if (!rc)
        rc = dev_build(d_elems, n, capacity, elem_len, d_digests, d_levels, d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_dev_ssz_bytes_list_tree_update(mk_call* call, void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                      uint32_t elem_len, void* d_digests, void* d_levels, const uint64_t* d_idx,
                                      uint64_t k_idx, const void* d_values, void* d_root32, void* d_ws,
                                      uint64_t ws_bytes, void* stream) {
    Scope S(call);
    int rc = bytes_tree_check_update(n_old, n_new, capacity, elem_len, k_idx, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = bytes_tree_check_ptrs(d_elems, n_new, capacity, d_digests, d_levels, d_root32, d_ws);
    if (!rc && k_idx && (!d_idx || ((uintptr_t)d_idx % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc)
        rc = dev_update(d_elems, n_old, n_new, capacity, elem_len, d_digests, d_levels, d_idx, k_idx, d_values,
                        d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

uint64_t mk_ssz_bytes_list_tree_erase_workspace_bytes(uint64_t moved, uint32_t elem_len) {
    return tree_shrink_ws(kBytesKind, moved, elem_len);
}

// The elements and their digests move; no element is digested.  Every
// argument check comes before the stream's device is looked up.
int mk_dev_ssz_bytes_list_tree_erase(mk_call* call, void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                     uint32_t elem_len, void* d_digests, void* d_levels, const uint64_t* d_rm,
                                     uint64_t k_rm, uint64_t first, void* d_root32, void* d_ws, uint64_t ws_bytes,
                                     void* stream) {
    Scope S(call);
    int rc = tree_shrink_check(kBytesKind, n_old, n_new, capacity, elem_len, k_rm, first, ws_bytes);
    if (!rc) rc = bytes_tree_check_ptrs(d_elems, n_old, capacity, d_digests, d_levels, d_root32, d_ws);
    if (!rc && k_rm && (!d_rm || ((uintptr_t)d_rm % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = tree_shrink(kBytesKind, d_elems, elem_len, d_digests, d_levels, n_old, n_new, capacity, d_rm, k_rm, first,
                         d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_bytes_list_tree_new(mk_call* call, uint32_t elem_len, uint64_t capacity, mk_bytes_list_tree** out) {
    Scope S(call);
    if (!out) return S.done(fail(MK_EINVAL, "null pointer"));
    *out = nullptr;
    int rc = check_shape(0, std::max<uint64_t>(capacity, 1), elem_len);
    if (!rc) rc = bind_call();
    if (rc) return S.done(rc);
    auto* t = new (std::nothrow) mk_bytes_list_tree();
    rc = tree_new(t, kBytesKind, elem_len, capacity);
    if (!rc) *out = t;
    return S.done(rc);
}

void mk_bytes_list_tree_free(mk_bytes_list_tree* t) { tree_free(t); }

uint64_t mk_bytes_list_tree_count(const mk_bytes_list_tree* t) { return t ? t->count : 0; }

int mk_bytes_list_tree_assign(mk_call* call, mk_bytes_list_tree* t, const uint8_t* elems, uint64_t n) {
    Scope S(call);
    return S.done(tree_assign(t, elems, n));
}

int mk_bytes_list_tree_update(mk_call* call, mk_bytes_list_tree* t, const uint64_t* idx, const uint8_t* elems,
                              uint64_t k) {
    Scope S(call);
    return S.done(tree_update(t, idx, elems, k));
}

int mk_bytes_list_tree_append(mk_call* call, mk_bytes_list_tree* t, const uint8_t* elems, uint64_t k) {
    Scope S(call);
    return S.done(tree_append(t, elems, k));
}

int mk_bytes_list_tree_truncate(mk_call* call, mk_bytes_list_tree* t, uint64_t n) {
    Scope S(call);
    return S.done(tree_truncate(t, n));
}

int mk_bytes_list_tree_erase(mk_call* call, mk_bytes_list_tree* t, const uint64_t* idx, uint64_t k) {
    Scope S(call);
    return S.done(tree_erase(t, idx, k));
}

int mk_bytes_list_tree_root(mk_call* call, mk_bytes_list_tree* t, uint8_t root[32]) {
    Scope S(call);
    return S.done(tree_root(t, root));
}

int mk_bytes_list_tree_elems(mk_call* call, mk_bytes_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(tree_read(t, first, cnt, out));
}

int mk_bytes_list_tree_branches(mk_call* call, mk_bytes_list_tree* t, const uint64_t* idx, uint64_t k, uint8_t* values_out,
                                uint8_t* branches_out) {
    Scope S(call);
    return S.done(tree_branches(t, idx, k, values_out, branches_out));
}

int mk_bytes_list_tree_clone(mk_call* call, mk_bytes_list_tree* src, mk_bytes_list_tree** out) {
    Scope S(call);
    TreeHandle* t = nullptr;
    const int rc = out ? tree_clone(src, &t) : fail(MK_EINVAL, "null pointer");
    if (out) *out = static_cast<mk_bytes_list_tree*>(t);
    return S.done(rc);
}

int mk_bytes_list_tree_copy(mk_call* call, mk_bytes_list_tree* dst, mk_bytes_list_tree* src) {
    Scope S(call);
    return S.done(tree_copy(dst, src));
}

int mk_bytes_list_tree_reserve(mk_call* call, mk_bytes_list_tree* t, uint64_t capacity) {
    Scope S(call);
    return S.done(tree_reserve(t, capacity));
}

uint64_t mk_bytes_list_tree_capacity(const mk_bytes_list_tree* t) { return t ? t->cap : 0; }

int mk_bytes_list_tree_audit(mk_call* call, mk_bytes_list_tree* t, mk_audit_report* out) {
    Scope S(call);
    return S.done(tree_audit(t, out));
}

int mk_bytes_list_tree_diff(mk_call* call, mk_bytes_list_tree* a, mk_bytes_list_tree* b, uint64_t* idx_out,
                            uint64_t max_out, uint64_t* total, uint64_t* n_a, uint64_t* n_b) {
    Scope S(call);
    return S.done(tree_diff(a, b, idx_out, max_out, total, n_a, n_b));
}

}  // extern "C"
