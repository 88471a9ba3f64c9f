// The device-resident registry tree: TreeHash of a list of flat structs
// (hash.go:118-159, 194-239) whose records, struct roots and levels stay in
// HBM -- build, update from the changed records only and the
// mk_*struct_list_tree* entry points.  The tree over the 32-B
// struct roots is the list tree's (list_tree_api.cpp, §5d); the
// mk_struct_list_tree handle is tree_handle.cpp's, with kStructKind.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

using Layout = mk::rt::StructTreeLayout;

struct mk_struct_list_tree : TreeHandle {  // item_len: the record length, level0: the struct roots
    Layout L{};
};

namespace {

// The handle rebuilds instead of climbing when count / MK_STRUCT_TREE_REBUILD_DIV
// <= dirty: on 2^20 ValidatorRecords an update of 2^15 random records is the
// largest power of two still cheaper than a build (0.68 against 0.75 ms; 2^16
// costs 1.07 ms): a dirty share of 2^15 / 2^20 = 1/32 (tools/struct_tree_probe.py,
// profiles/struct_tree/probe.json).
#define MK_STRUCT_TREE_REBUILD_DIV 32

uint64_t st_chunks(uint64_t n) { return ceil_div(n, 4); }  // 4 struct roots per chunk

uint64_t msg_bytes(const Layout& L, uint64_t n) { return L.fused ? 0 : align256(n * L.sp.msg_len); }

uint64_t build_ws(const Layout& L, uint64_t n) { return msg_bytes(L, n) + 256; }

// Regions of the update workspace for k work items (kq = max(k, 4): a list of
// up to 4 records is re-hashed whole): the list tree's arrival words, the
// gathered records, their struct messages, their roots.
struct UpdateWs {
    uint64_t arrive, gath, msg, roots, total;
};
UpdateWs update_ws(const Layout& L, uint64_t k) {
    const uint64_t kq = std::max<uint64_t>(k, 4);
    UpdateWs w{};
    w.arrive = 0;
    w.gath = align256(8 * kq);
    w.msg = w.gath + align256(kq * L.ext);
    w.roots = w.msg + msg_bytes(L, kq);
    w.total = w.roots + align256(32 * kq);
    return w;
}

// host-checkable arguments (no device needed)
int check_shape(uint64_t n, uint64_t capacity, uint32_t record_len) {
    if (record_len == 0) return fail(MK_EINVAL, "record_len == 0");
    if (n > capacity)
        return fail(MK_EINVAL, "%llu records > capacity %llu", (unsigned long long)n, (unsigned long long)capacity);
    if (capacity > UINT64_MAX / std::max<uint32_t>(record_len, 32))
        return fail(MK_EINVAL, "capacity * record_len overflows");
    return MK_OK;
}

// every struct root, then every level and the root
int dev_build(const Layout& L, const void* d_records, uint64_t n, uint64_t capacity, void* d_roots, void* d_levels,
              void* d_root32, void* d_ws, hipStream_t st) {
    TRY(struct_launch_roots(d_records, n, L.sp, d_ws, d_roots, st));
    return list_tree_build32(d_roots, n, capacity, d_levels, d_root32, (uint8_t*)d_ws + msg_bytes(L, n), st);
}

int dev_update(const Layout& L, void* d_records, uint64_t n_old, uint64_t n_new, uint64_t capacity, void* d_roots,
               void* d_levels, const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_root32,
               void* d_ws, hipStream_t st) {
    const UpdateWs w = update_ws(L, k_idx + (n_new - n_old));
    TRY(struct_tree_stage0(L, d_records, n_old, n_new, d_roots, d_idx, k_idx, d_values, (uint8_t*)d_ws + w.gath, st));
    if (st_chunks(n_new) <= 1) {  // one chunk, no levels: the mix-in over the raw chunk of roots
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)d_roots, 32 * n_new, n_new,
                           (uint8_t*)d_root32);
        return launched();
    }
    // the list tree's update (with nothing changed: the root again, from the stored top node)
    return list_tree_update32(d_roots, d_levels, d_idx, k_idx, n_old, n_new, capacity, d_root32,
                              (uint8_t*)d_ws + w.arrive, st);
}

// ---- what the handle (tree_handle.cpp) needs of this kind ----------------------------------
const Layout& layout_of(const TreeHandle& t) { return static_cast<const mk_struct_list_tree&>(t).L; }

const TreeKind kStructKind = {
    "registry tree", "records", MK_STRUCT_TREE_REBUILD_DIV, true, check_shape,
    [](const TreeHandle& t, uint64_t n) { return build_ws(layout_of(t), n); },
    [](const TreeHandle& t, uint64_t k) { return update_ws(layout_of(t), k).total; },
    [](const TreeHandle& t, const uint8_t* records, uint64_t n) {
        return mk::check_var_lengths(layout_of(t).sp, records, n);
    },
    [](const TreeHandle& t, uint64_t n, hipStream_t st) {
        return dev_build(layout_of(t), t.items.p, n, t.cap, t.level0.p, t.levels.p, t.root.p, t.ws.p, st);
    },
    [](const TreeHandle& t, uint64_t n_old, uint64_t n_new, const uint64_t* d_idx, uint64_t k_idx,
       const void* d_values, hipStream_t st) {
        return dev_update(layout_of(t), t.items.p, n_old, n_new, t.cap, t.level0.p, t.levels.p, d_idx, k_idx,
                          d_values, t.root.p, t.ws.p, st);
    },
    MK_TREE_STRUCT,
    [](const TreeHandle& t) { return struct_tree_handle(layout_of(t)); },
    [](const TreeHandle& a, const TreeHandle& b) {  // the parsed spec keeps every entry as it was given, zeros behind
        const mk::HostSpec &x = layout_of(a).sp, &y = layout_of(b).sp;
        return x.nfields == y.nfields && !std::memcmp(x.kind, y.kind, sizeof x.kind) &&
               !std::memcmp(x.off, y.off, sizeof x.off) && !std::memcmp(x.len, y.len, sizeof x.len);
    },
};

}  // namespace

// the registry tree's part of mk_dev_ssz_trees_update (tree_many_api.cpp)
namespace mk::rt {
int struct_tree_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, StructTreeLayout& L) {
    TRY(struct_make_spec(fields, nfields, record_len, L.sp));
    L.fused = struct_fused_layout(L.sp);
    uint32_t ext = 4;
    for (uint32_t f = 0; f < L.sp.nfields; ++f) {
        if (L.sp.kind[f] == MK_FIELD_STRUCT) continue;  // no bytes of its own
        const uint32_t slot = L.sp.kind[f] == MK_FIELD_VARBYTES ? 4 + L.sp.len[f] : L.sp.len[f];
        ext = std::max(ext, (L.sp.off[f] + slot + 3) & ~3u);
    }
    if (L.sp.lists) ext = L.sp.ext;  // a list's slot, and item fields at offsets inside the cell: the parser's figure
    L.ext = ext;
    return MK_OK;
}

uint64_t struct_tree_update_ws(const StructTreeLayout& L, uint64_t k, uint64_t* arrive_bytes) {
    const UpdateWs w = update_ws(L, k);
    *arrive_bytes = w.gath;
    return w.total;
}

int struct_tree_check_update(const StructTreeLayout& L, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                             uint64_t k_idx, uint64_t ws_bytes) {
    if (L.sp.rec_len == 0) return fail(MK_EINVAL, "record_len == 0");
    if (n_new < n_old)
        return fail(MK_EINVAL, "n_new %llu < n_old %llu (a registry tree does not shrink)",
                    (unsigned long long)n_new, (unsigned long long)n_old);
    TRY(check_shape(n_new, capacity, L.sp.rec_len));
    if (k_idx >= kMaxWork) return fail(MK_EINVAL, "%llu indices in one call", (unsigned long long)k_idx);
    const uint64_t T = k_idx + (n_new - n_old);
    if (T >= kMaxWork)
        return fail(MK_EINVAL, "%llu dirty records in one call (limit 2^31 - 1)", (unsigned long long)T);
    if (ws_bytes < update_ws(L, T).total) return fail(MK_ENOMEM, "workspace too small");
    return MK_OK;
}

int struct_tree_check_ptrs(const void* d_records, uint64_t n, uint64_t capacity, const void* d_roots,
                           const void* d_levels, const void* d_root32, const void* d_ws) {
    if (!d_roots || !d_root32 || !d_ws || (n && !d_records)) return fail(MK_EINVAL, "null pointer");
    if (st_chunks(capacity) > 1 && !d_levels) return fail(MK_EINVAL, "null level array");
    if (((uintptr_t)d_records % 4) || ((uintptr_t)d_roots % 16) || ((uintptr_t)d_levels % 16) ||
        ((uintptr_t)d_root32 % 4) || ((uintptr_t)d_ws % 8))
        return fail(MK_EINVAL, "records (4 B), roots (16 B), level array (16 B), root (4 B) or workspace (8 B) "
                               "misaligned");
    return MK_OK;
}

// Stage 0 of an update, everything before the climb: the new records scattered
// in, then level 0 (d_roots) brought up to date -- every root again for a list
// of one chunk (it has no levels), else the dirty records side by side, their
// roots by the struct-roots launch, the roots scattered into level 0.
// `d_scratch`: the update workspace from UpdateWs::gath on.
// (One fused launch -- struct root, arrival count per window, climb -- was
// built and measured slower than this at every k: DESIGN.md §5e.)
int struct_tree_stage0(const StructTreeLayout& L, void* d_records, uint64_t n_old, uint64_t n_new, void* d_roots,
                       const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_scratch, hipStream_t st) {
    const uint64_t n_app = n_new - n_old, T = k_idx + n_app;
    const UpdateWs w = update_ws(L, T);
    uint8_t* gath = (uint8_t*)d_scratch;
    uint8_t* msg = gath + (w.msg - w.gath);
    uint8_t* roots = gath + (w.roots - w.gath);
    if (d_values) TRY(list_tree_scatter(d_records, d_idx, k_idx, n_old, n_app, L.sp.rec_len, d_values, st));
    if (st_chunks(n_new) <= 1) return struct_launch_roots(d_records, n_new, L.sp, msg, d_roots, st);
    if (T == 0) return MK_OK;  // nothing changed
    mk::HostSpec sp = L.sp;
    const void* src = d_values;  // holds them in work-item order already
    if (!src) {
        hipLaunchKernelGGL(mk::k_struct_tree_gather, dim3(ceil_div(T * (L.ext / 4), 256)), dim3(256), 0, st,
                           (const uint8_t*)d_records, d_idx, k_idx, n_old, n_app, L.sp.rec_len, L.ext, gath);
        HIPCHK(hipGetLastError());
        src = gath;
        sp.rec_len = sp.prog.rec_len = sp.lprog.rec_len = L.ext;
    }
    TRY(struct_launch_roots(src, T, sp, msg, roots, st));
    return list_tree_scatter(d_roots, d_idx, k_idx, n_old, n_app, 32, roots, st);
}

// The struct-roots launch of struct_tree_stage0 alone, for the batched stage 0
// of several trees (tree_many_api.cpp), which has scattered d_values (non-null)
// into d_records on this stream and scatters the new roots itself: a list of
// one chunk gets every root again straight into d_roots (*d_new_roots = null),
// a longer one the roots of its T work items from d_values into the scratch
// (*d_new_roots: T x 32 B in work-item order; null when T == 0).
int struct_tree_stage0_roots(const StructTreeLayout& L, const void* d_records, uint64_t n_new, uint64_t T,
                             const void* d_values, void* d_roots, void* d_scratch, const void** d_new_roots,
                             hipStream_t st) {
    const UpdateWs w = update_ws(L, T);
    uint8_t* gath = (uint8_t*)d_scratch;
    uint8_t* msg = gath + (w.msg - w.gath);
    uint8_t* roots = gath + (w.roots - w.gath);
    *d_new_roots = nullptr;
    if (st_chunks(n_new) <= 1) return struct_launch_roots(d_records, n_new, L.sp, msg, d_roots, st);
    if (T == 0) return MK_OK;
    TRY(struct_launch_roots(d_values, T, L.sp, msg, roots, st));
    *d_new_roots = roots;
    return MK_OK;
}

TreeHandle* struct_tree_handle(const StructTreeLayout& L) {
    auto* t = new (std::nothrow) mk_struct_list_tree();
    if (t) t->L = L;
    return t;
}
const TreeKind& struct_tree_kind() { return kStructKind; }
const StructTreeLayout* struct_tree_layout_of(const TreeHandle& t) { return &layout_of(t); }
}  // namespace mk::rt

extern "C" {

uint64_t mk_ssz_struct_list_tree_build_workspace_bytes(uint64_t n, const mk_field* fields, uint32_t nfields) {
    Scope S(nullptr, false);
    Layout L;
    if (struct_tree_layout(fields, nfields, 0, L) != MK_OK) return 0;
    return build_ws(L, n);
}

uint64_t mk_ssz_struct_list_tree_update_workspace_bytes(uint64_t k, const mk_field* fields, uint32_t nfields) {
    Scope S(nullptr, false);
    Layout L;
    if (struct_tree_layout(fields, nfields, 0, L) != MK_OK) return 0;
    return update_ws(L, k).total;
}

// The argument checks come before the stream's device is looked up: a bad
// call is MK_EINVAL / MK_ENOMEM on any machine.
int mk_dev_ssz_struct_list_tree_build(mk_call* call, const void* d_records, uint64_t n, uint64_t capacity,
                                      uint32_t record_len, const mk_field* fields, uint32_t nfields, void* d_roots,
                                      void* d_levels, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream) {
    Scope S(call);
    Layout L;
    int rc = struct_tree_layout(fields, nfields, record_len, L);
    if (!rc) rc = check_shape(n, capacity, record_len);
    if (!rc && ws_bytes < build_ws(L, n)) rc = fail(MK_ENOMEM, "workspace too small");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = struct_tree_check_ptrs(d_records, n, capacity, d_roots, d_levels, d_root32, d_ws);
    if (!rc) rc = dev_build(L, d_records, n, capacity, d_roots, d_levels, d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_dev_ssz_struct_list_tree_update(mk_call* call, void* d_records, uint64_t n_old, uint64_t n_new,
                                       uint64_t capacity, uint32_t record_len, const mk_field* fields,
                                       uint32_t nfields, void* d_roots, void* d_levels, const uint64_t* d_idx,
                                       uint64_t k_idx, const void* d_values, void* d_root32, void* d_ws,
                                       uint64_t ws_bytes, void* stream) {
    Scope S(call);
    Layout L;
    int rc = struct_tree_layout(fields, nfields, record_len, L);
    if (!rc) rc = struct_tree_check_update(L, n_old, n_new, capacity, k_idx, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = struct_tree_check_ptrs(d_records, n_new, capacity, d_roots, d_levels, d_root32, d_ws);
    if (!rc && k_idx && (!d_idx || ((uintptr_t)d_idx % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc && ((uintptr_t)d_values % 4)) rc = fail(MK_EINVAL, "new records not 4-byte aligned");
    if (!rc)
        rc = dev_update(L, d_records, n_old, n_new, capacity, d_roots, d_levels, d_idx, k_idx, d_values, d_root32,
                        d_ws, (hipStream_t)stream);
    return S.done(rc);
}

uint64_t mk_ssz_struct_list_tree_erase_workspace_bytes(uint64_t moved, uint32_t record_len) {
    return tree_shrink_ws(kStructKind, moved, record_len);
}

// The records and their struct roots move; no record is hashed.  Every
// argument check comes before the stream's device is looked up.
int mk_dev_ssz_struct_list_tree_erase(mk_call* call, void* d_records, uint64_t n_old, uint64_t n_new,
                                      uint64_t capacity, uint32_t record_len, const mk_field* fields,
                                      uint32_t nfields, void* d_roots, void* d_levels, const uint64_t* d_rm,
                                      uint64_t k_rm, uint64_t first, void* d_root32, void* d_ws, uint64_t ws_bytes,
                                      void* stream) {
    Scope S(call);
    Layout L;
    int rc = struct_tree_layout(fields, nfields, record_len, L);
    if (!rc) rc = tree_shrink_check(kStructKind, n_old, n_new, capacity, record_len, k_rm, first, ws_bytes);
    if (!rc) rc = struct_tree_check_ptrs(d_records, n_old, capacity, d_roots, d_levels, d_root32, d_ws);
    if (!rc && k_rm && (!d_rm || ((uintptr_t)d_rm % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = tree_shrink(kStructKind, d_records, record_len, d_roots, d_levels, n_old, n_new, capacity, d_rm, k_rm,
                         first, d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_struct_list_tree_new(mk_call* call, uint32_t record_len, const mk_field* fields, uint32_t nfields,
                            uint64_t capacity, mk_struct_list_tree** out) {
    Scope S(call);
    if (!out) return S.done(fail(MK_EINVAL, "null pointer"));
    *out = nullptr;
    Layout L;
    int rc = struct_tree_layout(fields, nfields, record_len, L);
    if (!rc) rc = check_shape(0, std::max<uint64_t>(capacity, 1), record_len);
    if (!rc) rc = bind_call();
    if (rc) return S.done(rc);
    auto* t = new (std::nothrow) mk_struct_list_tree();
    if (t) t->L = L;
    rc = tree_new(t, kStructKind, record_len, capacity);
    if (!rc) *out = t;
    return S.done(rc);
}

void mk_struct_list_tree_free(mk_struct_list_tree* t) { tree_free(t); }

uint64_t mk_struct_list_tree_count(const mk_struct_list_tree* t) { return t ? t->count : 0; }

int mk_struct_list_tree_assign(mk_call* call, mk_struct_list_tree* t, const uint8_t* records, uint64_t n) {
    Scope S(call);
    return S.done(tree_assign(t, records, n));
}

int mk_struct_list_tree_update(mk_call* call, mk_struct_list_tree* t, const uint64_t* idx, const uint8_t* records,
                               uint64_t k) {
    Scope S(call);
    return S.done(tree_update(t, idx, records, k));
}

int mk_struct_list_tree_append(mk_call* call, mk_struct_list_tree* t, const uint8_t* records, uint64_t k) {
    Scope S(call);
    return S.done(tree_append(t, records, k));
}

int mk_struct_list_tree_truncate(mk_call* call, mk_struct_list_tree* t, uint64_t n) {
    Scope S(call);
    return S.done(tree_truncate(t, n));
}

int mk_struct_list_tree_erase(mk_call* call, mk_struct_list_tree* t, const uint64_t* idx, uint64_t k) {
    Scope S(call);
    return S.done(tree_erase(t, idx, k));
}

int mk_struct_list_tree_root(mk_call* call, mk_struct_list_tree* t, uint8_t root[32]) {
    Scope S(call);
    return S.done(tree_root(t, root));
}

int mk_struct_list_tree_records(mk_call* call, mk_struct_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(tree_read(t, first, cnt, out));
}

int mk_struct_list_tree_branches(mk_call* call, mk_struct_list_tree* t, const uint64_t* idx, uint64_t k,
                                 uint8_t* values_out, uint8_t* branches_out) {
    Scope S(call);
    return S.done(tree_branches(t, idx, k, values_out, branches_out));
}

int mk_struct_list_tree_verify_repeat_hash(mk_call* call, mk_struct_list_tree* t, uint32_t commit_off,
                                           uint32_t layers_off, const uint64_t* idx, const uint8_t* reveals,
                                           uint64_t m, uint32_t max_layers, uint8_t* ok) {
    Scope S(call);
    return S.done(tree_verify_repeat_hash(t, commit_off, layers_off, idx, reveals, m, max_layers, ok));
}

int mk_struct_list_tree_clone(mk_call* call, mk_struct_list_tree* src, mk_struct_list_tree** out) {
    Scope S(call);
    TreeHandle* t = nullptr;
    const int rc = out ? tree_clone(src, &t) : fail(MK_EINVAL, "null pointer");
    if (out) *out = static_cast<mk_struct_list_tree*>(t);
    return S.done(rc);
}

int mk_struct_list_tree_copy(mk_call* call, mk_struct_list_tree* dst, mk_struct_list_tree* src) {
    Scope S(call);
    return S.done(tree_copy(dst, src));
}

int mk_struct_list_tree_reserve(mk_call* call, mk_struct_list_tree* t, uint64_t capacity) {
    Scope S(call);
    return S.done(tree_reserve(t, capacity));
}

uint64_t mk_struct_list_tree_capacity(const mk_struct_list_tree* t) { return t ? t->cap : 0; }

int mk_struct_list_tree_audit(mk_call* call, mk_struct_list_tree* t, mk_audit_report* out) {
    Scope S(call);
    return S.done(tree_audit(t, out));
}

int mk_struct_list_tree_diff(mk_call* call, mk_struct_list_tree* a, mk_struct_list_tree* b, uint64_t* idx_out,
                             uint64_t max_out, uint64_t* total, uint64_t* n_a, uint64_t* n_b) {
    Scope S(call);
    return S.done(tree_diff(a, b, idx_out, max_out, total, n_a, n_b));
}

}  // extern "C"
