// The device-resident tree of a list of byte strings: TreeHash of a [][N]byte
// (hash.go:100-107, 118-139, 194-239) whose elements, element digests
// K(le32(elem_len) || e_i) and levels stay in HBM -- build, update from the
// changed elements only, the mk_bytes_list_tree handle and the
// mk_*bytes_list_tree* entry points.  The tree over the 32-B
// digests is the list tree's (list_tree_api.cpp, §5d).
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

// ---- bytes tree handle -------------------------------------------------------------------
struct mk_bytes_list_tree {
    std::mutex mu;
    int dev = 0;
    uint32_t elem_len = 0;
    uint64_t cap = 0, count = 0;  // elements
    DevBuf elems, digs, levels, root, idx, vals, ws;
};

namespace {

// The handle rebuilds instead of climbing when count / kRebuildDiv <= dirty:
// on the 2^24 x 32-B list an update of 2^16 random elements (1.599 ms) is the
// largest power of two still cheaper than a build (2.519 ms), 2^17 costs
// 2.930 ms: a dirty share of 2^16 / 2^24 = 1/256 (tools/bytes_tree_probe.py,
// profiles/bytes_tree/probe.json).
#define MK_BYTES_TREE_REBUILD_DIV 256
constexpr uint64_t kRebuildDiv = MK_BYTES_TREE_REBUILD_DIV;
constexpr uint64_t kMaxWork = 1ull << 31;  // work items of one update launch

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

int check_update(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t elem_len, uint64_t k_idx,
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

int check_ptrs(const void* d_elems, uint64_t n, uint64_t capacity, const void* d_digests, const void* d_levels,
               const void* d_root32, const void* d_ws) {
    if (!d_digests || !d_root32 || !d_ws || (n && !d_elems)) return fail(MK_EINVAL, "null pointer");
    if (bt_chunks(capacity) > 1 && !d_levels) return fail(MK_EINVAL, "null level array");
    if (((uintptr_t)d_digests % 16) || ((uintptr_t)d_levels % 16) || ((uintptr_t)d_root32 % 4) ||
        ((uintptr_t)d_ws % 8))
        return fail(MK_EINVAL, "digests (16 B), level array (16 B), root (4 B) or workspace (8 B) misaligned");
    return MK_OK;
}

// every element digest, then every level and the root
int dev_build(const void* d_elems, uint64_t n, uint64_t capacity, uint32_t elem_len, void* d_digests, void* d_levels,
              void* d_root32, void* d_ws, hipStream_t st) {
    TRY(launch_elem_digests(d_elems, n, elem_len, d_digests, st));
    return list_tree_build32(d_digests, n, capacity, d_levels, d_root32, d_ws, st);
}

// Stage 0 of an update, everything before the climb: the new elements
// scattered in, then level 0 (d_digests) brought up to date -- every digest
// again for a list of one chunk (it has no levels), else the dirty elements'
// digests, read in place and stored into level 0.  (Digest and climb in one
// launch -- the level-1 owner pairs digesting their own elements -- were built
// and measured no faster at any k: DESIGN.md §5f.)
int stage0(void* d_elems, uint64_t n_old, uint64_t n_new, uint32_t elem_len, void* d_digests, const uint64_t* d_idx,
           uint64_t k_idx, const void* d_values, hipStream_t st) {
    const uint64_t n_app = n_new - n_old, T = k_idx + n_app;
    if (d_values) TRY(list_tree_scatter(d_elems, d_idx, k_idx, n_old, n_app, elem_len, d_values, st));
    if (bt_chunks(n_new) <= 1) return launch_elem_digests(d_elems, n_new, elem_len, d_digests, st);
    if (T == 0) return MK_OK;  // nothing changed
    const uint32_t fast32 = elem_len == 32 && ((uintptr_t)d_elems % 16) == 0;
    hipLaunchKernelGGL(mk::k_bytes_tree_digest, dim3(ceil_div(T, 256)), dim3(256), 0, st, (const uint8_t*)d_elems,
                       elem_len, fast32, d_idx, k_idx, n_old, n_app, (uint4*)d_digests);
    return launched();
}

int dev_update(void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t elem_len, void* d_digests,
               void* d_levels, const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_root32,
               void* d_ws, hipStream_t st) {
    TRY(stage0(d_elems, n_old, n_new, elem_len, d_digests, d_idx, k_idx, d_values, st));
    if (bt_chunks(n_new) <= 1) {  // one chunk, no levels: the mix-in over the raw chunk of digests
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, (const uint8_t*)d_digests, 32 * n_new, n_new,
                           (uint8_t*)d_root32);
        return launched();
    }
    // the list tree's update (with nothing changed: the root again, from the stored top node)
    return list_tree_update32(d_digests, d_levels, d_idx, k_idx, n_old, n_new, capacity, d_root32, d_ws, st);
}

// ---- handle ------------------------------------------------------------------------------
int tree_alloc(mk_bytes_list_tree* t, uint64_t cap) {
    TRY(check_shape(0, cap, t->elem_len));
    TRY(grow(t->elems, cap * t->elem_len + 16));
    TRY(grow(t->digs, 32 * cap + 16));
    TRY(grow(t->levels, mk_ssz_list_tree_levels_bytes(cap, 32)));
    t->cap = cap;
    return MK_OK;
}

// all digests, levels and the root of the elements already in t->elems
int tree_rebuild(mk_bytes_list_tree* t, uint64_t n, hipStream_t st) {
    TRY(grow(t->ws, build_ws()));
    return dev_build(t->elems.p, n, t->cap, t->elem_len, t->digs.p, t->levels.p, t->root.p, t->ws.p, st);
}

bool rebuild_pays(uint64_t dirty, uint64_t count) { return dirty && count / kRebuildDiv <= dirty; }

int tree_assign(mk_bytes_list_tree* t, const uint8_t* elems, uint64_t n) {
    if (!t || (n && !elems)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    if (n > t->cap) TRY(tree_alloc(t, n));
    if (n) HIPCHK(hipMemcpyAsync(t->elems.p, elems, n * t->elem_len, hipMemcpyHostToDevice, st));
    TRY(tree_rebuild(t, n, st));
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffer is released after this
    t->count = n;
    return MK_OK;
}

int tree_update(mk_bytes_list_tree* t, const uint64_t* idx, const uint8_t* elems, uint64_t k) {
    if (!t || (k && (!idx || !elems))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= t->count)
            return fail(MK_EINVAL, "index %llu beyond %llu elements", (unsigned long long)idx[i],
                        (unsigned long long)t->count);
    if (k == 0) return MK_OK;
    // list[idx[j]] = elems[j] in sequence: ascending indices, the last value of a repeated one
    std::vector<uint64_t> order(k);
    for (uint64_t i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return idx[a] < idx[b]; });
    const uint32_t L = t->elem_len;
    std::vector<uint64_t> sidx;
    std::vector<uint8_t> svals;
    sidx.reserve(k);
    svals.reserve(k * L);
    for (uint64_t i = 0; i < k; ++i) {
        if (i + 1 < k && idx[order[i + 1]] == idx[order[i]]) continue;
        sidx.push_back(idx[order[i]]);
        svals.insert(svals.end(), elems + order[i] * L, elems + (order[i] + 1) * L);
    }
    const uint64_t m = sidx.size();
    if (m >= kMaxWork) return fail(MK_EINVAL, "%llu dirty elements in one call", (unsigned long long)m);
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(grow(t->idx, 8 * m));
    TRY(grow(t->vals, m * L + 16));
    HIPCHK(hipMemcpyAsync(t->idx.p, sidx.data(), 8 * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t->vals.p, svals.data(), m * L, hipMemcpyHostToDevice, st));
    if (rebuild_pays(m, t->count)) {
        TRY(list_tree_scatter(t->elems.p, (const uint64_t*)t->idx.p, m, t->count, 0, L, t->vals.p, st));
        TRY(tree_rebuild(t, t->count, st));
    } else {
        TRY(grow(t->ws, update_ws(m)));
        TRY(dev_update(t->elems.p, t->count, t->count, t->cap, L, t->digs.p, t->levels.p, (const uint64_t*)t->idx.p,
                       m, t->vals.p, t->root.p, t->ws.p, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // sidx / svals are released after this
    return MK_OK;
}

int tree_append(mk_bytes_list_tree* t, const uint8_t* elems, uint64_t k) {
    if (!t || (k && !elems)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (k == 0) return MK_OK;
    if (k >= kMaxWork || t->count + k < k)
        return fail(MK_EINVAL, "%llu elements in one append", (unsigned long long)k);
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint32_t L = t->elem_len;
    const uint64_t n_new = t->count + k;
    bool rebuild = rebuild_pays(k, n_new);
    if (n_new > t->cap) {  // the layout depends on the capacity: double it, move the elements, rebuild
        const uint64_t ncap = std::max(2 * t->cap, n_new);
        TRY(check_shape(n_new, ncap, L));
        DevBuf ne;
        TRY(grow(ne, ncap * L + 16));
        if (t->count) HIPCHK(hipMemcpyAsync(ne.p, t->elems.p, t->count * L, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(t->elems.p);
        t->elems = ne;
        TRY(grow(t->digs, 32 * ncap + 16));  // every digest is computed again below
        TRY(grow(t->levels, mk_ssz_list_tree_levels_bytes(ncap, 32)));
        t->cap = ncap;
        rebuild = true;
    }
    HIPCHK(hipMemcpyAsync((uint8_t*)t->elems.p + t->count * L, elems, k * L, hipMemcpyHostToDevice, st));
    if (rebuild) {
        TRY(tree_rebuild(t, n_new, st));
    } else {
        TRY(grow(t->ws, update_ws(k)));
        TRY(dev_update(t->elems.p, t->count, n_new, t->cap, L, t->digs.p, t->levels.p, nullptr, 0, nullptr, t->root.p,
                       t->ws.p, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffer is released after this
    t->count = n_new;
    return MK_OK;
}

int tree_root(mk_bytes_list_tree* t, uint8_t* root) {
    if (!t || !root) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(bind_dev(t->dev));
    HIPCHK(hipMemcpyAsync(root, t->root.p, 32, hipMemcpyDeviceToHost, ctx()->stream));
    HIPCHK(hipStreamSynchronize(ctx()->stream));
    return MK_OK;
}

int tree_elems(mk_bytes_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    if (!t || (cnt && !out)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (first > t->count || cnt > t->count - first)
        return fail(MK_EINVAL, "elements [%llu, +%llu) beyond %llu elements", (unsigned long long)first,
                    (unsigned long long)cnt, (unsigned long long)t->count);
    if (!cnt) return MK_OK;
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint32_t L = t->elem_len;
    HIPCHK(hipMemcpyAsync(out, (const uint8_t*)t->elems.p + first * L, cnt * L, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

}  // namespace

// the bytes tree's part of mk_dev_ssz_trees_update (tree_many_api.cpp)
namespace mk::rt {
int bytes_tree_check_update(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t elem_len, uint64_t k_idx,
                            uint64_t ws_bytes) {
    return check_update(n_old, n_new, capacity, elem_len, k_idx, ws_bytes);
}
int bytes_tree_check_ptrs(const void* d_elems, uint64_t n, uint64_t capacity, const void* d_digests,
                          const void* d_levels, const void* d_root32, const void* d_ws) {
    return check_ptrs(d_elems, n, capacity, d_digests, d_levels, d_root32, d_ws);
}
int bytes_tree_stage0(void* d_elems, uint64_t n_old, uint64_t n_new, uint32_t elem_len, void* d_digests,
                      const uint64_t* d_idx, uint64_t k_idx, const void* d_values, hipStream_t st) {
    return stage0(d_elems, n_old, n_new, elem_len, d_digests, d_idx, k_idx, d_values, st);
}
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
    if (!rc) rc = check_ptrs(d_elems, n, capacity, d_digests, d_levels, d_root32, d_ws);
    if (!rc)
        rc = dev_build(d_elems, n, capacity, elem_len, d_digests, d_levels, d_root32, d_ws, (hipStream_t)stream);
    return S.done(rc);
}

int mk_dev_ssz_bytes_list_tree_update(mk_call* call, void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                      uint32_t elem_len, void* d_digests, void* d_levels, const uint64_t* d_idx,
                                      uint64_t k_idx, const void* d_values, void* d_root32, void* d_ws,
                                      uint64_t ws_bytes, void* stream) {
    Scope S(call);
    int rc = check_update(n_old, n_new, capacity, elem_len, k_idx, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = check_ptrs(d_elems, n_new, capacity, d_digests, d_levels, d_root32, d_ws);
    if (!rc && k_idx && (!d_idx || ((uintptr_t)d_idx % 8))) rc = fail(MK_EINVAL, "null or misaligned index array");
    if (!rc)
        rc = dev_update(d_elems, n_old, n_new, capacity, elem_len, d_digests, d_levels, d_idx, k_idx, d_values,
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
    if (!t) return S.done(fail(MK_ENOMEM, "bytes tree allocation failed"));
    t->dev = t_bound;
    t->elem_len = elem_len;
    rc = tree_alloc(t, std::max<uint64_t>(capacity, 1));
    if (!rc) rc = grow(t->root, 32);
    if (!rc) rc = tree_rebuild(t, 0, ctx()->stream);  // merkleHash([])
    if (!rc && hipStreamSynchronize(ctx()->stream) != hipSuccess) rc = fail(MK_EHIP, "hipStreamSynchronize failed");
    if (rc) {
        mk_bytes_list_tree_free(t);
        return S.done(rc);
    }
    *out = t;
    return S.done(MK_OK);
}

void mk_bytes_list_tree_free(mk_bytes_list_tree* t) {
    if (!t) return;
    int saved = -1;
    const bool restore = hipGetDevice(&saved) == hipSuccess;
    (void)hipSetDevice(t->dev);
    for (DevBuf* b : {&t->elems, &t->digs, &t->levels, &t->root, &t->idx, &t->vals, &t->ws})
        if (b->p) (void)hipFree(b->p);
    if (restore) (void)hipSetDevice(saved);
    delete t;
}

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

int mk_bytes_list_tree_root(mk_call* call, mk_bytes_list_tree* t, uint8_t root[32]) {
    Scope S(call);
    return S.done(tree_root(t, root));
}

int mk_bytes_list_tree_elems(mk_call* call, mk_bytes_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(tree_elems(t, first, cnt, out));
}

}  // extern "C"
