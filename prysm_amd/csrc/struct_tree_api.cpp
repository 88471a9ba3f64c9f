// The device-resident registry tree: TreeHash of a list of flat structs
// (hash.go:118-159, 194-239) whose records, struct roots and levels stay in
// HBM -- build, update from the changed records only, the mk_struct_list_tree
// handle and the mk_*struct_list_tree* entry points.  The tree
// over the 32-B struct roots is the list tree's (list_tree_api.cpp, §5d).
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

// ---- registry tree handle ----------------------------------------------------------------
using Layout = mk::rt::StructTreeLayout;

struct mk_struct_list_tree {
    std::mutex mu;
    int dev = 0;
    Layout L{};
    uint64_t cap = 0, count = 0;  // records
    DevBuf recs, roots, levels, root, idx, vals, ws;
};

namespace {

// The handle rebuilds instead of climbing when count / kRebuildDiv <= dirty:
// on 2^20 ValidatorRecords an update of 2^15 random records is the largest
// power of two still cheaper than a build (0.68 against 0.75 ms; 2^16 costs
// 1.07 ms): a dirty share of 2^15 / 2^20 = 1/32 (tools/struct_tree_probe.py,
// profiles/struct_tree/probe.json).
#define MK_STRUCT_TREE_REBUILD_DIV 32
constexpr uint64_t kRebuildDiv = MK_STRUCT_TREE_REBUILD_DIV;
constexpr uint64_t kMaxWork = 1ull << 31;  // work items of one update launch

uint64_t st_chunks(uint64_t n) { return ceil_div(n, 4); }  // 4 struct roots per chunk

int st_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, Layout& L) {
    TRY(struct_make_spec(fields, nfields, record_len, L.sp));
    L.fused = struct_fused_layout(L.sp);
    uint32_t ext = 4;
    for (uint32_t f = 0; f < L.sp.nfields; ++f) {
        if (L.sp.kind[f] == MK_FIELD_STRUCT) continue;  // no bytes of its own
        const uint32_t slot = L.sp.kind[f] == MK_FIELD_VARBYTES ? 4 + L.sp.len[f] : L.sp.len[f];
        ext = std::max(ext, (L.sp.off[f] + slot + 3) & ~3u);
    }
    L.ext = ext;
    return MK_OK;
}

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

int check_update(const Layout& L, uint64_t n_old, uint64_t n_new, uint64_t capacity, uint64_t k_idx,
                 uint64_t ws_bytes) {
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

int check_ptrs(const void* d_records, uint64_t n, uint64_t capacity, const void* d_roots, const void* d_levels,
               const void* d_root32, const void* d_ws) {
    if (!d_roots || !d_root32 || !d_ws || (n && !d_records)) return fail(MK_EINVAL, "null pointer");
    if (st_chunks(capacity) > 1 && !d_levels) return fail(MK_EINVAL, "null level array");
    if (((uintptr_t)d_records % 4) || ((uintptr_t)d_roots % 16) || ((uintptr_t)d_levels % 16) ||
        ((uintptr_t)d_root32 % 4) || ((uintptr_t)d_ws % 8))
        return fail(MK_EINVAL, "records (4 B), roots (16 B), level array (16 B), root (4 B) or workspace (8 B) "
                               "misaligned");
    return MK_OK;
}

// every struct root, then every level and the root
int dev_build(const Layout& L, const void* d_records, uint64_t n, uint64_t capacity, void* d_roots, void* d_levels,
              void* d_root32, void* d_ws, hipStream_t st) {
    TRY(struct_launch_roots(d_records, n, L.sp, d_ws, d_roots, st));
    return list_tree_build32(d_roots, n, capacity, d_levels, d_root32, (uint8_t*)d_ws + msg_bytes(L, n), st);
}

// Stage 0 of an update, everything before the climb: the new records scattered
// in, then level 0 (d_roots) brought up to date -- every root again for a list
// of one chunk (it has no levels), else the dirty records side by side, their
// roots by the struct-roots launch, the roots scattered into level 0.
// `scratch`: the update workspace from UpdateWs::gath on.
// (One fused launch -- struct root, arrival count per window, climb -- was
// built and measured slower than this at every k: DESIGN.md §5e.)
int stage0(const Layout& L, void* d_records, uint64_t n_old, uint64_t n_new, void* d_roots, const uint64_t* d_idx,
           uint64_t k_idx, const void* d_values, uint8_t* scratch, hipStream_t st) {
    const uint64_t n_app = n_new - n_old, T = k_idx + n_app;
    const UpdateWs w = update_ws(L, T);
    uint8_t* gath = scratch;
    uint8_t* msg = scratch + (w.msg - w.gath);
    uint8_t* roots = scratch + (w.roots - w.gath);
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
        sp.rec_len = sp.prog.rec_len = L.ext;
    }
    TRY(struct_launch_roots(src, T, sp, msg, roots, st));
    return list_tree_scatter(d_roots, d_idx, k_idx, n_old, n_app, 32, roots, st);
}

int dev_update(const Layout& L, void* d_records, uint64_t n_old, uint64_t n_new, uint64_t capacity, void* d_roots,
               void* d_levels, const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_root32,
               void* d_ws, hipStream_t st) {
    const UpdateWs w = update_ws(L, k_idx + (n_new - n_old));
    TRY(stage0(L, d_records, n_old, n_new, d_roots, d_idx, k_idx, d_values, (uint8_t*)d_ws + w.gath, st));
    if (st_chunks(n_new) <= 1) {  // one chunk, no levels: the mix-in over the raw chunk of roots
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)d_roots, 32 * n_new, n_new,
                           (uint8_t*)d_root32);
        return launched();
    }
    // the list tree's update (with nothing changed: the root again, from the stored top node)
    return list_tree_update32(d_roots, d_levels, d_idx, k_idx, n_old, n_new, capacity, d_root32,
                              (uint8_t*)d_ws + w.arrive, st);
}

// ---- handle ------------------------------------------------------------------------------
int tree_alloc(mk_struct_list_tree* t, uint64_t cap) {
    TRY(check_shape(0, cap, t->L.sp.rec_len));
    TRY(grow(t->recs, cap * t->L.sp.rec_len + 16));
    TRY(grow(t->roots, 32 * cap + 16));
    TRY(grow(t->levels, mk_ssz_list_tree_levels_bytes(cap, 32)));
    t->cap = cap;
    return MK_OK;
}

// all roots, levels and the root of the records already in t->recs
int tree_rebuild(mk_struct_list_tree* t, uint64_t n, hipStream_t st) {
    TRY(grow(t->ws, build_ws(t->L, n)));
    return dev_build(t->L, t->recs.p, n, t->cap, t->roots.p, t->levels.p, t->root.p, t->ws.p, st);
}

bool rebuild_pays(uint64_t dirty, uint64_t count) { return dirty && count / kRebuildDiv <= dirty; }

int tree_assign(mk_struct_list_tree* t, const uint8_t* records, uint64_t n) {
    if (!t || (n && !records)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(mk::check_var_lengths(t->L.sp, records, n));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    if (n > t->cap) TRY(tree_alloc(t, n));
    if (n) HIPCHK(hipMemcpyAsync(t->recs.p, records, n * t->L.sp.rec_len, hipMemcpyHostToDevice, st));
    TRY(tree_rebuild(t, n, st));
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffer is released after this
    t->count = n;
    return MK_OK;
}

int tree_update(mk_struct_list_tree* t, const uint64_t* idx, const uint8_t* records, uint64_t k) {
    if (!t || (k && (!idx || !records))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= t->count)
            return fail(MK_EINVAL, "index %llu beyond %llu records", (unsigned long long)idx[i],
                        (unsigned long long)t->count);
    if (k == 0) return MK_OK;
    TRY(mk::check_var_lengths(t->L.sp, records, k));
    // list[idx[j]] = records[j] in sequence: ascending indices, the last value of a repeated one
    std::vector<uint64_t> order(k);
    for (uint64_t i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return idx[a] < idx[b]; });
    const uint32_t R = t->L.sp.rec_len;
    std::vector<uint64_t> sidx;
    std::vector<uint8_t> svals;
    sidx.reserve(k);
    svals.reserve(k * R);
    for (uint64_t i = 0; i < k; ++i) {
        if (i + 1 < k && idx[order[i + 1]] == idx[order[i]]) continue;
        sidx.push_back(idx[order[i]]);
        svals.insert(svals.end(), records + order[i] * R, records + (order[i] + 1) * R);
    }
    const uint64_t m = sidx.size();
    if (m >= kMaxWork) return fail(MK_EINVAL, "%llu dirty records in one call", (unsigned long long)m);
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(grow(t->idx, 8 * m));
    TRY(grow(t->vals, m * R + 16));
    HIPCHK(hipMemcpyAsync(t->idx.p, sidx.data(), 8 * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t->vals.p, svals.data(), m * R, hipMemcpyHostToDevice, st));
    if (rebuild_pays(m, t->count)) {
        TRY(list_tree_scatter(t->recs.p, (const uint64_t*)t->idx.p, m, t->count, 0, R, t->vals.p, st));
        TRY(tree_rebuild(t, t->count, st));
    } else {
        TRY(grow(t->ws, update_ws(t->L, m).total));
        TRY(dev_update(t->L, t->recs.p, t->count, t->count, t->cap, t->roots.p, t->levels.p,
                       (const uint64_t*)t->idx.p, m, t->vals.p, t->root.p, t->ws.p, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // sidx / svals are released after this
    return MK_OK;
}

int tree_append(mk_struct_list_tree* t, const uint8_t* records, uint64_t k) {
    if (!t || (k && !records)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (k == 0) return MK_OK;
    if (k >= kMaxWork || t->count + k < k)
        return fail(MK_EINVAL, "%llu records in one append", (unsigned long long)k);
    TRY(mk::check_var_lengths(t->L.sp, records, k));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint32_t R = t->L.sp.rec_len;
    const uint64_t n_new = t->count + k;
    bool rebuild = rebuild_pays(k, n_new);
    if (n_new > t->cap) {  // the layout depends on the capacity: double it, move the records, rebuild
        const uint64_t ncap = std::max(2 * t->cap, n_new);
        TRY(check_shape(n_new, ncap, R));
        DevBuf nr;
        TRY(grow(nr, ncap * R + 16));
        if (t->count) HIPCHK(hipMemcpyAsync(nr.p, t->recs.p, t->count * R, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(t->recs.p);
        t->recs = nr;
        TRY(grow(t->roots, 32 * ncap + 16));  // every root is computed again below
        TRY(grow(t->levels, mk_ssz_list_tree_levels_bytes(ncap, 32)));
        t->cap = ncap;
        rebuild = true;
    }
    HIPCHK(hipMemcpyAsync((uint8_t*)t->recs.p + t->count * R, records, k * R, hipMemcpyHostToDevice, st));
    if (rebuild) {
        TRY(tree_rebuild(t, n_new, st));
    } else {
        TRY(grow(t->ws, update_ws(t->L, k).total));
        TRY(dev_update(t->L, t->recs.p, t->count, n_new, t->cap, t->roots.p, t->levels.p, nullptr, 0, nullptr,
                       t->root.p, t->ws.p, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffer is released after this
    t->count = n_new;
    return MK_OK;
}

int tree_root(mk_struct_list_tree* t, uint8_t* root) {
    if (!t || !root) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(bind_dev(t->dev));
    HIPCHK(hipMemcpyAsync(root, t->root.p, 32, hipMemcpyDeviceToHost, ctx()->stream));
    HIPCHK(hipStreamSynchronize(ctx()->stream));
    return MK_OK;
}

int tree_records(mk_struct_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    if (!t || (cnt && !out)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (first > t->count || cnt > t->count - first)
        return fail(MK_EINVAL, "records [%llu, +%llu) beyond %llu records", (unsigned long long)first,
                    (unsigned long long)cnt, (unsigned long long)t->count);
    if (!cnt) return MK_OK;
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint32_t R = t->L.sp.rec_len;
    HIPCHK(hipMemcpyAsync(out, (const uint8_t*)t->recs.p + first * R, cnt * R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

}  // namespace

// the registry tree's part of mk_dev_ssz_trees_update (tree_many_api.cpp)
namespace mk::rt {
int struct_tree_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, StructTreeLayout& L) {
    return st_layout(fields, nfields, record_len, L);
}
uint64_t struct_tree_update_ws(const StructTreeLayout& L, uint64_t k, uint64_t* arrive_bytes) {
    const UpdateWs w = update_ws(L, k);
    *arrive_bytes = w.gath;
    return w.total;
}
int struct_tree_check_update(const StructTreeLayout& L, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                             uint64_t k_idx, uint64_t ws_bytes) {
    if (L.sp.rec_len == 0) return fail(MK_EINVAL, "record_len == 0");
    return check_update(L, n_old, n_new, capacity, k_idx, ws_bytes);
}
int struct_tree_check_ptrs(const void* d_records, uint64_t n, uint64_t capacity, const void* d_roots,
                           const void* d_levels, const void* d_root32, const void* d_ws) {
    return check_ptrs(d_records, n, capacity, d_roots, d_levels, d_root32, d_ws);
}
int struct_tree_stage0(const StructTreeLayout& L, void* d_records, uint64_t n_old, uint64_t n_new, void* d_roots,
                       const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_scratch, hipStream_t st) {
    return stage0(L, d_records, n_old, n_new, d_roots, d_idx, k_idx, d_values, (uint8_t*)d_scratch, st);
}
}  // namespace mk::rt

extern "C" {

uint64_t mk_ssz_struct_list_tree_build_workspace_bytes(uint64_t n, const mk_field* fields, uint32_t nfields) {
    Scope S(nullptr, false);
    Layout L;
    if (st_layout(fields, nfields, 0, L) != MK_OK) return 0;
    return build_ws(L, n);
}

uint64_t mk_ssz_struct_list_tree_update_workspace_bytes(uint64_t k, const mk_field* fields, uint32_t nfields) {
    Scope S(nullptr, false);
    Layout L;
    if (st_layout(fields, nfields, 0, L) != MK_OK) return 0;
    return update_ws(L, k).total;
}

// The argument checks come before the stream's device is looked up: a bad
// call is MK_EINVAL / MK_ENOMEM on any machine.
int mk_dev_ssz_struct_list_tree_build(mk_call* call, const void* d_records, uint64_t n, uint64_t capacity,
                                      uint32_t record_len, const mk_field* fields, uint32_t nfields, void* d_roots,
                                      void* d_levels, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream) {
    Scope S(call);
    Layout L;
    int rc = st_layout(fields, nfields, record_len, L);
    if (!rc) rc = check_shape(n, capacity, record_len);
    if (!rc && ws_bytes < build_ws(L, n)) rc = fail(MK_ENOMEM, "workspace too small");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = check_ptrs(d_records, n, capacity, d_roots, d_levels, d_root32, d_ws);
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
    int rc = st_layout(fields, nfields, record_len, L);
    if (!rc && record_len == 0) rc = fail(MK_EINVAL, "record_len == 0");
    if (!rc) rc = check_update(L, n_old, n_new, capacity, k_idx, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = check_ptrs(d_records, n_new, capacity, d_roots, d_levels, d_root32, d_ws);
    if (!rc && k_idx && (!d_idx || ((uintptr_t)d_idx % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc && ((uintptr_t)d_values % 4)) rc = fail(MK_EINVAL, "new records not 4-byte aligned");
    if (!rc)
        rc = dev_update(L, d_records, n_old, n_new, capacity, d_roots, d_levels, d_idx, k_idx, d_values, d_root32,
                        d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_struct_list_tree_new(mk_call* call, uint32_t record_len, const mk_field* fields, uint32_t nfields,
                            uint64_t capacity, mk_struct_list_tree** out) {
    Scope S(call);
    if (!out) return S.done(fail(MK_EINVAL, "null pointer"));
    *out = nullptr;
    Layout L;
    int rc = st_layout(fields, nfields, record_len, L);
    if (!rc) rc = check_shape(0, std::max<uint64_t>(capacity, 1), record_len);
    if (!rc) rc = bind_call();
    if (rc) return S.done(rc);
    auto* t = new (std::nothrow) mk_struct_list_tree();
    if (!t) return S.done(fail(MK_ENOMEM, "registry tree allocation failed"));
    t->dev = t_bound;
    t->L = L;
    rc = tree_alloc(t, std::max<uint64_t>(capacity, 1));
    if (!rc) rc = grow(t->root, 32);
    if (!rc) rc = tree_rebuild(t, 0, ctx()->stream);  // merkleHash([])
    if (!rc && hipStreamSynchronize(ctx()->stream) != hipSuccess) rc = fail(MK_EHIP, "hipStreamSynchronize failed");
    if (rc) {
        mk_struct_list_tree_free(t);
        return S.done(rc);
    }
    *out = t;
    return S.done(MK_OK);
}

void mk_struct_list_tree_free(mk_struct_list_tree* t) {
    if (!t) return;
    int saved = -1;
    const bool restore = hipGetDevice(&saved) == hipSuccess;
    (void)hipSetDevice(t->dev);
    for (DevBuf* b : {&t->recs, &t->roots, &t->levels, &t->root, &t->idx, &t->vals, &t->ws})
        if (b->p) (void)hipFree(b->p);
    if (restore) (void)hipSetDevice(saved);
    delete t;
}

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

int mk_struct_list_tree_root(mk_call* call, mk_struct_list_tree* t, uint8_t root[32]) {
    Scope S(call);
    return S.done(tree_root(t, root));
}

int mk_struct_list_tree_records(mk_call* call, mk_struct_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(tree_records(t, first, cnt, out));
}

}  // extern "C"
