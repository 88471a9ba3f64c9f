// The host handle of a device-resident tree, once for the three kinds
// (mk_list_tree §5d, mk_struct_list_tree §5e, mk_bytes_list_tree §5f): the
// list, its level 0 and its levels in HBM, assign / update / append / root /
// read-back under one mutex.  What a kind does differently is its TreeKind
// (runtime.hpp), defined in list_tree_api, struct_tree_api, bytes_tree_api.
#include <functional>

#include "list_branch.hpp"
#include "runtime.hpp"

using namespace mk;

namespace mk::rt {
namespace {

// level 0 and the levels for `cap` items (the item buffer is the caller's: an append has to move it)
int grow_levels(TreeHandle* t, uint64_t cap) {
    if (t->kind->level0) TRY(grow(t->level0, 32 * cap + 16));  // every entry is computed again by the rebuild
    return grow(t->levels, mk_ssz_list_tree_levels_bytes(cap, t->kind->level0 ? 32 : t->item_len));
}

int alloc(TreeHandle* t, uint64_t cap) {
    TRY(t->kind->check_shape(0, cap, t->item_len));
    TRY(grow(t->items, cap * t->item_len + 16));
    TRY(grow_levels(t, cap));
    t->cap = cap;
    return MK_OK;
}

// level 0, all levels and the root of the items already in t->items
int rebuild(TreeHandle* t, uint64_t n, hipStream_t st) {
    TRY(grow(t->ws, t->kind->build_ws(*t, n)));
    return t->kind->dev_build(*t, n, st);
}

bool rebuild_pays(const TreeHandle* t, uint64_t dirty, uint64_t count) {
    return dirty && count / t->kind->rebuild_div <= dirty;
}

int check_values(const TreeHandle* t, const uint8_t* values, uint64_t n) {
    return t->kind->check_values ? t->kind->check_values(*t, values, n) : MK_OK;
}

}  // namespace

int tree_new(TreeHandle* t, const TreeKind& kind, uint32_t item_len, uint64_t capacity) {
    if (!t) return fail(MK_ENOMEM, "%s allocation failed", kind.name);
    t->kind = &kind;
    t->dev = t_bound;
    t->item_len = item_len;
    int rc = alloc(t, std::max<uint64_t>(capacity, 1));
    if (!rc) rc = grow(t->root, 32);
    if (!rc) rc = rebuild(t, 0, ctx()->stream);  // merkleHash([])
    if (!rc && hipStreamSynchronize(ctx()->stream) != hipSuccess) rc = fail(MK_EHIP, "hipStreamSynchronize failed");
    if (rc) tree_free(t);
    return rc;
}

void tree_free(TreeHandle* t) {
    if (!t) return;
    int saved = -1;
    const bool restore = hipGetDevice(&saved) == hipSuccess;
    (void)hipSetDevice(t->dev);
    for (DevBuf* b : {&t->items, &t->level0, &t->levels, &t->root, &t->idx, &t->vals, &t->ws})
        if (b->p) (void)hipFree(b->p);
    if (restore) (void)hipSetDevice(saved);
    delete t;
}

int tree_assign(TreeHandle* t, const uint8_t* values, uint64_t n) {
    if (!t || (n && !values)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(check_values(t, values, n));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    if (n > t->cap) TRY(alloc(t, n));
    if (n) HIPCHK(hipMemcpyAsync(t->items.p, values, n * t->item_len, hipMemcpyHostToDevice, st));
    TRY(rebuild(t, n, st));
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffer is released after this
    t->count = n;
    return MK_OK;
}

int tree_update(TreeHandle* t, const uint64_t* idx, const uint8_t* values, uint64_t k) {
    if (!t || (k && (!idx || !values))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    const char* noun = t->kind->noun;
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= t->count)
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[i],
                        (unsigned long long)t->count, noun);
    if (k == 0) return MK_OK;
    TRY(check_values(t, values, k));
    // list[idx[j]] = values[j] in sequence: ascending indices, the last value of a repeated one
    std::vector<uint64_t> order(k);
    for (uint64_t i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return idx[a] < idx[b]; });
    const uint32_t L = t->item_len;
    std::vector<uint64_t> sidx;
    std::vector<uint8_t> svals;
    sidx.reserve(k);
    svals.reserve(k * L);
    for (uint64_t i = 0; i < k; ++i) {
        if (i + 1 < k && idx[order[i + 1]] == idx[order[i]]) continue;
        sidx.push_back(idx[order[i]]);
        svals.insert(svals.end(), values + order[i] * L, values + (order[i] + 1) * L);
    }
    const uint64_t m = sidx.size();
    if (m >= kMaxWork) return fail(MK_EINVAL, "%llu dirty %s in one call", (unsigned long long)m, noun);
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(grow(t->idx, 8 * m));
    TRY(grow(t->vals, m * L + 16));
    HIPCHK(hipMemcpyAsync(t->idx.p, sidx.data(), 8 * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t->vals.p, svals.data(), m * L, hipMemcpyHostToDevice, st));
    if (rebuild_pays(t, m, t->count)) {
        TRY(list_tree_scatter(t->items.p, (const uint64_t*)t->idx.p, m, t->count, 0, L, t->vals.p, st));
        TRY(rebuild(t, t->count, st));
    } else {
        TRY(grow(t->ws, t->kind->update_ws(*t, m)));
        TRY(t->kind->dev_update(*t, t->count, t->count, (const uint64_t*)t->idx.p, m, t->vals.p, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // sidx / svals are released after this
    return MK_OK;
}

int tree_append(TreeHandle* t, const uint8_t* values, uint64_t k) {
    if (!t || (k && !values)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (k == 0) return MK_OK;
    if (k >= kMaxWork || t->count + k < k)
        return fail(MK_EINVAL, "%llu %s in one append", (unsigned long long)k, t->kind->noun);
    TRY(check_values(t, values, k));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint32_t L = t->item_len;
    const uint64_t n_new = t->count + k;
    bool rebuild_all = rebuild_pays(t, k, n_new);
    if (n_new > t->cap) {  // the layout depends on the capacity: double it, move the items, rebuild
        const uint64_t ncap = std::max(2 * t->cap, n_new);
        TRY(t->kind->check_shape(n_new, ncap, L));
        DevBuf ni;
        TRY(grow(ni, ncap * L + 16));
        if (t->count) HIPCHK(hipMemcpyAsync(ni.p, t->items.p, t->count * L, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(t->items.p);
        t->items = ni;
        TRY(grow_levels(t, ncap));
        t->cap = ncap;
        rebuild_all = true;
    }
    HIPCHK(hipMemcpyAsync((uint8_t*)t->items.p + t->count * L, values, k * L, hipMemcpyHostToDevice, st));
    if (rebuild_all) {
        TRY(rebuild(t, n_new, st));
    } else {
        TRY(grow(t->ws, t->kind->update_ws(*t, k)));
        TRY(t->kind->dev_update(*t, t->count, n_new, nullptr, 0, nullptr, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffer is released after this
    t->count = n_new;
    return MK_OK;
}

int tree_write_through_build(TreeHandle* t, uint64_t n_old, uint64_t n_new, uint64_t new_cap, const uint64_t* d_idx,
                             uint64_t k_idx, const void* d_values, hipStream_t st) {
    const uint32_t L = t->item_len;
    if (new_cap > t->cap) {  // as tree_append: the layout depends on the capacity
        TRY(t->kind->check_shape(n_new, new_cap, L));
        DevBuf ni;
        TRY(grow(ni, new_cap * L + 16));
        if (n_old) HIPCHK(hipMemcpyAsync(ni.p, t->items.p, n_old * L, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(t->items.p);
        t->items = ni;
        TRY(grow_levels(t, new_cap));
        t->cap = new_cap;
    }
    TRY(list_tree_scatter(t->items.p, d_idx, k_idx, n_old, n_new - n_old, L, d_values, st));
    return rebuild(t, n_new, st);
}

namespace {
// the shrink on the handle's own buffers (under its lock); rm: k_rm sorted indices (host), uploaded into t->idx
int shrink(TreeHandle* t, uint64_t n_new, const uint64_t* rm, uint64_t k_rm, uint64_t first, hipStream_t st) {
    const uint32_t L = t->item_len;
    const uint64_t need = tree_shrink_ws(*t->kind, k_rm ? n_new - first : 0, L);
    TRY(grow(t->ws, need));
    TRY(tree_shrink_check(*t->kind, t->count, n_new, t->cap, L, k_rm, first, t->ws.cap));
    if (k_rm) {
        TRY(grow(t->idx, 8 * k_rm));
        HIPCHK(hipMemcpyAsync(t->idx.p, rm, 8 * k_rm, hipMemcpyHostToDevice, st));
    }
    TRY(tree_shrink(*t->kind, t->items.p, L, t->level0.p, t->levels.p, t->count, n_new, t->cap,
                    (const uint64_t*)t->idx.p, k_rm, first, t->root.p, t->ws.p, st));
    HIPCHK(hipStreamSynchronize(st));  // rm is released after this
    t->count = n_new;
    return MK_OK;
}
}  // namespace

int tree_truncate(TreeHandle* t, uint64_t n) {
    if (!t) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (n > t->count)
        return fail(MK_EINVAL, "truncate to %llu of %llu %s", (unsigned long long)n, (unsigned long long)t->count,
                    t->kind->noun);
    if (n == t->count) return MK_OK;
    TRY(bind_dev(t->dev));
    return shrink(t, n, nullptr, 0, n, ctx()->stream);
}

int tree_erase(TreeHandle* t, const uint64_t* idx, uint64_t k) {
    if (!t || (k && !idx)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= t->count)
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[i],
                        (unsigned long long)t->count, t->kind->noun);
    if (k == 0) return MK_OK;
    std::vector<uint64_t> rm(idx, idx + k);
    std::sort(rm.begin(), rm.end());
    rm.erase(std::unique(rm.begin(), rm.end()), rm.end());
    const uint64_t m = rm.size(), n_new = t->count - m;
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    if (rm[0] + m == t->count) return shrink(t, n_new, nullptr, 0, n_new, st);  // a suffix: nothing moves
    return shrink(t, n_new, rm.data(), m, rm[0], st);
}

int tree_root(TreeHandle* t, uint8_t* root) {
    if (!t || !root) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(bind_dev(t->dev));
    HIPCHK(hipMemcpyAsync(root, t->root.p, 32, hipMemcpyDeviceToHost, ctx()->stream));
    HIPCHK(hipStreamSynchronize(ctx()->stream));
    return MK_OK;
}

int tree_read(TreeHandle* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    if (!t || (cnt && !out)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (first > t->count || cnt > t->count - first)
        return fail(MK_EINVAL, "%s [%llu, +%llu) beyond %llu %s", t->kind->noun, (unsigned long long)first,
                    (unsigned long long)cnt, (unsigned long long)t->count, t->kind->noun);
    if (!cnt) return MK_OK;
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint32_t L = t->item_len;
    HIPCHK(hipMemcpyAsync(out, (const uint8_t*)t->items.p + first * L, cnt * L, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// The proofs of k values: the indices up, one gather launch
// over level 0 and the levels, the records back.  A value lies in its
// record's window, so the k level-0 values are copied out of the records on
// the host: no second read-back.
int tree_branches(TreeHandle* t, const uint64_t* idx, uint64_t k, uint8_t* values_out, uint8_t* branches_out) {
    if (!t || (k && (!idx || !values_out || !branches_out))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= t->count)
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[i],
                        (unsigned long long)t->count, t->kind->noun);
    if (k == 0) return MK_OK;
    const uint32_t L = t->kind->level0 ? 32 : t->item_len;  // a leaf: the item, or its 32-B root / digest
    const uint64_t stride = mk_ssz_list_branch_bytes(t->count, L);
    if (!stride) return fail(MK_EINVAL, "item_len %u above %u: no proof record", L, kBranchItemMax);
    if (k >= kMaxWork) return fail(MK_EINVAL, "%llu proofs in one call (limit 2^31 - 1)", (unsigned long long)k);
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const void* leaves = t->kind->level0 ? t->level0.p : t->items.p;
    TRY(grow(t->idx, 8 * k));
    TRY(grow(t->ws, stride * k));
    TRY(list_branches_check(leaves, t->count, t->cap, L, t->levels.p, (const uint64_t*)t->idx.p, k, t->ws.p));
    HIPCHK(hipMemcpyAsync(t->idx.p, idx, 8 * k, hipMemcpyHostToDevice, st));
    TRY(list_branches_launch(leaves, t->count, t->cap, L, t->levels.p, (const uint64_t*)t->idx.p, k, t->ws.p, st));
    HIPCHK(hipMemcpyAsync(branches_out, t->ws.p, stride * k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // idx is released after this
    const BranchShape b = branch_shape(t->count, t->cap, L);
    for (uint64_t g = 0; g < k; ++g)
        std::memcpy(values_out + g * L, branches_out + g * stride + branch_item_pos(b, idx[g]), L);
    return MK_OK;
}

// ---- clone, copy, reserve ---------------------------------------------------------
// One operation under the three: the live part of a tree moved from the layout
// of one capacity into buffers laid out for another by the copy launch
// (tree_copy_api.cpp).  Nothing is uploaded and nothing is hashed.
bool tree_same_shape(const TreeHandle& a, const TreeHandle& b) {
    return a.kind == b.kind && a.item_len == b.item_len && a.kind->same_layout(a, b);
}

void tree_bufs_free(TreeBufs& b) {
    for (DevBuf* d : {&b.items, &b.level0, &b.levels, &b.root}) {
        if (d->p) (void)hipFree(d->p);
        *d = DevBuf{};
    }
}

// the sizes of alloc() / grow_levels() above
int tree_bufs_alloc(const TreeHandle& like, uint64_t cap, bool with_root, TreeBufs& b) {
    const uint32_t L = like.item_len;
    int rc = like.kind->check_shape(0, cap, L);
    if (!rc) rc = grow(b.items, cap * L + 16);
    if (!rc && like.kind->level0) rc = grow(b.level0, 32 * cap + 16);
    if (!rc) rc = grow(b.levels, mk_ssz_list_tree_levels_bytes(cap, like.kind->level0 ? 32 : L));
    if (!rc && with_root) rc = grow(b.root, 32);
    if (rc) tree_bufs_free(b);
    return rc;
}

void tree_bufs_install(TreeHandle* t, TreeBufs& b, uint64_t cap) {
    TreeBufs old;
    old.items = t->items, old.level0 = t->level0, old.levels = t->levels;
    t->items = b.items, t->level0 = b.level0, t->levels = b.levels;
    if (b.root.p) {
        old.root = t->root;
        t->root = b.root;
    }
    t->cap = cap;
    b = TreeBufs{};
    tree_bufs_free(old);
}

int tree_new_like(const TreeHandle& src, TreeHandle** out) {
    TreeHandle* t = src.kind->make_like(src);
    if (!t) return fail(MK_ENOMEM, "%s allocation failed", src.kind->name);
    t->kind = src.kind;
    t->dev = src.dev;
    t->item_len = src.item_len;
    TreeBufs b;
    const int rc = tree_bufs_alloc(src, src.cap, true, b);
    if (rc) {
        tree_free(t);
        return rc;
    }
    tree_bufs_install(t, b, src.cap);
    *out = t;
    return MK_OK;
}

mk_tree_copy tree_copy_desc(const TreeHandle& src, const TreeHandle& dst, const TreeBufs* nb, uint64_t dst_cap) {
    mk_tree_copy c{};
    c.kind = src.kind->id;
    c.item_len = src.item_len;
    c.n = src.count;
    c.src_capacity = src.cap;
    c.dst_capacity = dst_cap;
    const bool l0 = src.kind->level0;
    c.d_src_items = src.items.p, c.d_src_level0 = l0 ? src.level0.p : nullptr, c.d_src_levels = src.levels.p;
    c.d_src_root32 = src.root.p;
    c.d_dst_items = nb ? nb->items.p : dst.items.p;
    c.d_dst_level0 = !l0 ? nullptr : nb ? nb->level0.p : dst.level0.p;
    c.d_dst_levels = nb ? nb->levels.p : dst.levels.p;
    c.d_dst_root32 = nb && nb->root.p ? nb->root.p : dst.root.p;
    return c;
}

namespace {
// one tree's copy: the checks, the launch, the synchronise
int copy_one(const mk_tree_copy& c, hipStream_t st) {
    TRY(trees_copy_check(&c, 1, nullptr, nullptr));
    TRY(trees_copy_launch(&c, 1, nullptr, nullptr, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}
}  // namespace

int tree_clone(TreeHandle* src, TreeHandle** out) {
    if (!src || !out) return fail(MK_EINVAL, "null pointer");
    *out = nullptr;
    std::lock_guard<std::mutex> tl(src->mu);
    TRY(bind_dev(src->dev));
    TreeHandle* t = nullptr;
    TRY(tree_new_like(*src, &t));
    const int rc = copy_one(tree_copy_desc(*src, *t, nullptr, t->cap), ctx()->stream);
    if (rc) {
        tree_free(t);
        return rc;
    }
    t->count = src->count;
    *out = t;
    return MK_OK;
}

int tree_copy(TreeHandle* dst, TreeHandle* src) {
    if (!dst || !src) return fail(MK_EINVAL, "null pointer");
    if (dst == src) return MK_OK;
    // Both handles' mutexes, always the one at the lower address first: two
    // threads copying a <- b and b <- a take them in the same order.
    std::mutex *first = &dst->mu, *second = &src->mu;
    if (std::less<std::mutex*>()(second, first)) std::swap(first, second);
    std::lock_guard<std::mutex> l1(*first);
    std::lock_guard<std::mutex> l2(*second);
    if (!tree_same_shape(*dst, *src))
        return fail(MK_EINVAL, "a copy between a %s of %u-byte %s and a %s of %u-byte %s, or of another layout",
                    dst->kind->name, dst->item_len, dst->kind->noun, src->kind->name, src->item_len, src->kind->noun);
    if (dst->dev != src->dev) return fail(MK_EINVAL, "the trees live on devices %d and %d", dst->dev, src->dev);
    TRY(bind_dev(src->dev));
    const bool regrow = src->count > dst->cap;  // else dst keeps its capacity
    TreeBufs nb;
    if (regrow) TRY(tree_bufs_alloc(*src, src->cap, false, nb));  // before anything is enqueued: a failure leaves dst as it was
    const uint64_t cap = regrow ? src->cap : dst->cap;
    const int rc = copy_one(tree_copy_desc(*src, *dst, regrow ? &nb : nullptr, cap), ctx()->stream);
    if (rc) {
        tree_bufs_free(nb);
        return rc;
    }
    if (regrow) tree_bufs_install(dst, nb, cap);
    dst->count = src->count;
    return MK_OK;
}

int tree_reserve(TreeHandle* t, uint64_t capacity) {
    if (!t) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (capacity <= t->cap) return MK_OK;
    TRY(t->kind->check_shape(t->count, capacity, t->item_len));
    TRY(bind_dev(t->dev));
    TreeBufs nb;  // a root of its own: no destination range of the copy may be one of its sources
    TRY(tree_bufs_alloc(*t, capacity, true, nb));
    const int rc = copy_one(tree_copy_desc(*t, *t, &nb, capacity), ctx()->stream);
    if (rc) {
        tree_bufs_free(nb);
        return rc;
    }
    tree_bufs_install(t, nb, capacity);
    return MK_OK;
}

// ---- audit ------------------------------------------------------------------------
mk_tree_audit tree_audit_desc(const TreeHandle& t, uint32_t container_off) {
    mk_tree_audit a{};
    a.kind = t.kind->id;
    a.item_len = t.item_len;
    a.d_items = t.items.p;
    a.d_level0 = t.kind->level0 ? t.level0.p : nullptr;
    a.d_levels = t.levels.p;
    a.d_root32 = t.root.p;
    a.n = t.count;
    a.capacity = t.cap;
    a.container_off = container_off;
    return a;
}

// The handle's workspace holds the two reports (its front, 256 bytes) and the
// level-0 piece behind them: the chain of tree_audit_api.cpp, one read-back.
int tree_audit(TreeHandle* t, mk_audit_report* out) {
    if (!t || !out) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    const mk_tree_audit a = tree_audit_desc(*t, MK_NO_CONTAINER);
    const StructTreeLayout* L = t->kind->id == MK_TREE_STRUCT ? struct_tree_layout_of(*t) : nullptr;
    AuditCall c;
    TRY(trees_audit_prepare(&a, 1, &L, 0, c));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(grow(t->ws, 256 + c.ws));
    uint8_t* ws = (uint8_t*)t->ws.p;
    TRY(trees_audit_check(&a, 1, c, nullptr, 0, nullptr, ws, ws + 256, c.ws));
    TRY(trees_audit_launch(&a, 1, c, nullptr, 0, nullptr, ws, ws + 256, st));
    mk_audit_report both[2];
    HIPCHK(hipMemcpyAsync(both, ws, sizeof both, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = both[0];
    return MK_OK;
}

// ---- diff -------------------------------------------------------------------------
mk_tree_diff tree_diff_desc(const TreeHandle& a, const TreeHandle& b, uint64_t* d_idx_out, uint64_t max_out) {
    mk_tree_diff d{};
    d.kind = a.kind->id;
    d.item_len = a.item_len;
    const bool l0 = a.kind->level0;
    d.d_a_items = a.items.p, d.d_a_level0 = l0 ? a.level0.p : nullptr, d.d_a_levels = a.levels.p;
    d.d_b_items = b.items.p, d.d_b_level0 = l0 ? b.level0.p : nullptr, d.d_b_levels = b.levels.p;
    d.n_a = a.count, d.capacity_a = a.cap;
    d.n_b = b.count, d.capacity_b = b.cap;
    d.d_idx_out = max_out ? d_idx_out : nullptr;
    d.max_out = max_out;
    return d;
}

void tree_diff_sort(uint64_t* slots, uint64_t total, uint64_t max_out) {
    std::sort(slots, slots + std::min(total, max_out));
}

// a's workspace holds the report (its front, 16 bytes) and the max_out slots
// behind it: one launch, one read-back of both.
int tree_diff(TreeHandle* a, TreeHandle* b, uint64_t* idx_out, uint64_t max_out, uint64_t* total, uint64_t* n_a,
              uint64_t* n_b) {
    if (!a || !b || !total || !n_a || !n_b || (max_out && !idx_out)) return fail(MK_EINVAL, "null pointer");
    if (max_out >= (1ull << 60)) return fail(MK_EINVAL, "max_out * 8 overflows");
    if (a == b) {
        std::lock_guard<std::mutex> tl(a->mu);
        *total = 0;
        *n_a = *n_b = a->count;
        return MK_OK;
    }
    // both handles' mutexes, the one at the lower address first (as tree_copy)
    std::mutex *first = &a->mu, *second = &b->mu;
    if (std::less<std::mutex*>()(second, first)) std::swap(first, second);
    std::lock_guard<std::mutex> l1(*first);
    std::lock_guard<std::mutex> l2(*second);
    if (!tree_same_shape(*a, *b))
        return fail(MK_EINVAL, "a diff between a %s of %u-byte %s and a %s of %u-byte %s, or of another layout",
                    a->kind->name, a->item_len, a->kind->noun, b->kind->name, b->item_len, b->kind->noun);
    if (a->dev != b->dev) return fail(MK_EINVAL, "the trees live on devices %d and %d", a->dev, b->dev);
    TRY(bind_dev(a->dev));
    hipStream_t st = ctx()->stream;
    TRY(grow(a->ws, 16 + 8 * max_out));
    uint8_t* ws = (uint8_t*)a->ws.p;
    const mk_tree_diff d = tree_diff_desc(*a, *b, (uint64_t*)(ws + 16), max_out);
    TRY(trees_diff_check(&d, 1, ws));
    TRY(trees_diff_launch(&d, 1, ws, st));
    std::vector<uint64_t> back(2 + max_out);
    HIPCHK(hipMemcpyAsync(back.data(), ws, 8 * back.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *total = back[0];
    *n_a = a->count;
    *n_b = b->count;
    tree_diff_sort(back.data() + 2, back[0], max_out);
    if (max_out) std::memcpy(idx_out, back.data() + 2, 8 * std::min(back[0], max_out));
    return MK_OK;
}

}  // namespace mk::rt
