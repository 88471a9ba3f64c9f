// The resident deposit trie rolled back, compared, audited, cloned, copied and
// grown on the device (the rules: trie_admin.hpp): the
// mk_dev_deposit_trie_truncate / _fork_point / _audit / _copy entry points and
// the handle forms over mk_trie.  Every argument check comes before the
// stream's device is looked up; no entry allocates, uploads or synchronises in
// its device form.
#include <functional>

#include "runtime.hpp"
#include "trie_admin.hpp"
#include "trie_handle.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

constexpr uint64_t kTrieAdminGridMax = 2048;  // workgroups: 8 per CU, the rest by grid stride

int check_shape(uint64_t cap, uint64_t count, uint32_t depth) {
    if (depth == 0 || depth > kTrieDepthMax) return fail(MK_EINVAL, "depth %u out of range (1..63)", depth);
    if (count > cap)
        return fail(MK_EINVAL, "count %llu > capacity %llu", (unsigned long long)count, (unsigned long long)cap);
    if (count > (1ull << depth))
        return fail(MK_EINVAL, "%llu deposits do not fit a depth-%u trie", (unsigned long long)count, depth);
    return MK_OK;
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) != 0; }

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

// ---- roll back ------------------------------------------------------------------------------------
int truncate_check(const void* d_levels, uint64_t cap, uint64_t count, uint64_t c, uint32_t depth,
                   const void* d_root32) {
    TRY(check_shape(cap, count, depth));
    if (c > count)
        return fail(MK_EINVAL, "roll back to %llu beyond %llu deposits", (unsigned long long)c,
                    (unsigned long long)count);
    if (!d_root32 || (cap && !d_levels)) return fail(MK_EINVAL, "null pointer");
    if (misaligned(d_levels, 16) || misaligned(d_root32, 16)) return fail(MK_EINVAL, "levels or root misaligned (16 B)");
    return MK_OK;
}

int truncate_launch(void* d_levels, uint64_t cap, uint64_t count, uint64_t c, uint32_t depth, void* d_root32,
                    hipStream_t st) {
    hipLaunchKernelGGL(mk::k_trie_truncate, dim3(1), dim3(64), 0, st, (uint4*)d_levels, cap, count, c, depth,
                       (uint4*)d_root32);
    return launched();
}

// ---- fork point -----------------------------------------------------------------------------------
int fork_check(const void* a, uint64_t cap_a, uint64_t count_a, const void* b, uint64_t cap_b, uint64_t count_b,
               uint32_t depth, const void* d_out8) {
    TRY(check_shape(cap_a, count_a, depth));
    TRY(check_shape(cap_b, count_b, depth));
    if (!d_out8 || (count_a && count_b && (!a || !b))) return fail(MK_EINVAL, "null pointer");
    if (misaligned(a, 16) || misaligned(b, 16)) return fail(MK_EINVAL, "levels misaligned (16 B)");
    if (misaligned(d_out8, 8)) return fail(MK_EINVAL, "output misaligned (8 B)");
    return MK_OK;
}

int fork_launch(const void* a, uint64_t cap_a, uint64_t count_a, const void* b, uint64_t cap_b, uint64_t count_b,
                uint32_t depth, void* d_out8, hipStream_t st) {
    hipLaunchKernelGGL(mk::k_trie_fork_point, dim3(1), dim3(64), 0, st, (const uint4*)a, cap_a, count_a,
                       (const uint4*)b, cap_b, count_b, depth, (uint64_t*)d_out8);
    return launched();
}

// ---- audit ----------------------------------------------------------------------------------------
int audit_check(const void* d_levels, uint64_t cap, uint64_t count, uint32_t depth, const void* d_root32,
                const void* d_report) {
    TRY(check_shape(cap, count, depth));
    if (!d_root32 || !d_report || (count && !d_levels)) return fail(MK_EINVAL, "null pointer");
    if (misaligned(d_levels, 16) || misaligned(d_root32, 16)) return fail(MK_EINVAL, "levels or root misaligned (16 B)");
    if (misaligned(d_report, 8)) return fail(MK_EINVAL, "report misaligned (8 B)");
    // count <= 2^63 and every level above the first has at most half the nodes: no overflow
    if (count > kMaxWork || ta_audit_items(count, depth) > kMaxWork)
        return fail(MK_EINVAL, "more than 2^31 work items in one audit (%llu deposits)", (unsigned long long)count);
    return MK_OK;
}

// the report cleared, the one launch over every node, the key unpacked: a linear chain
int audit_launch(const void* d_levels, uint64_t cap, uint64_t count, uint32_t depth, const void* d_root32,
                 void* d_report, hipStream_t st) {
    mk::AuditReport* rep = (mk::AuditReport*)d_report;
    hipLaunchKernelGGL(mk::k_audit_reports, dim3(1), dim3(64), 0, st, rep, 1u, 0u);
    TRY(launched());
    const uint64_t items = ta_audit_items(count, depth);
    const uint64_t grid = std::min<uint64_t>(ceil_div(items, mk::kAuditThreads), kTrieAdminGridMax);
    hipLaunchKernelGGL(mk::k_trie_audit, dim3((uint32_t)grid), dim3(mk::kAuditThreads), 0, st, (const uint4*)d_levels,
                       cap, count, depth, (const uint4*)d_root32, rep);
    TRY(launched());
    hipLaunchKernelGGL(mk::k_audit_reports, dim3(1), dim3(64), 0, st, rep, 1u, 1u);
    return launched();
}

// ---- copy -----------------------------------------------------------------------------------------
int copy_check(const void* src, uint64_t cap_src, uint64_t count, const void* dst, uint64_t cap_dst, uint32_t depth,
               const void* src_root, const void* dst_root) {
    TRY(check_shape(cap_src, count, depth));
    TRY(check_shape(cap_dst, count, depth));
    if ((count && (!src || !dst)) || !src_root != !dst_root) return fail(MK_EINVAL, "null pointer");
    if (misaligned(src, 16) || misaligned(dst, 16) || misaligned(src_root, 16) || misaligned(dst_root, 16))
        return fail(MK_EINVAL, "levels or root misaligned (16 B)");
    const uint64_t sb = mk_deposit_trie_levels_bytes(cap_src, depth), db = mk_deposit_trie_levels_bytes(cap_dst, depth);
    if (overlap(src, sb, dst, db) || overlap(src_root, 32, dst_root, 32) || overlap(src, sb, dst_root, 32) ||
        overlap(src_root, 32, dst, db) || overlap(dst, db, dst_root, 32))
        return fail(MK_EINVAL, "the source and the destination of a copy overlap");
    return MK_OK;
}

int copy_launch(const void* src, uint64_t cap_src, uint64_t count, void* dst, uint64_t cap_dst, uint32_t depth,
                const void* src_root, void* dst_root, hipStream_t st) {
    const uint64_t pieces = ta_copy_first(count, depth + 1) + (src_root ? 2 : 0);
    if (pieces == 0) return MK_OK;
    const uint64_t grid = std::min<uint64_t>(ceil_div(pieces, mk::kCopyThreads), kTrieAdminGridMax);
    hipLaunchKernelGGL(mk::k_trie_copy, dim3((uint32_t)grid), dim3(mk::kCopyThreads), 0, st, (const uint4*)src, cap_src,
                       count, (uint4*)dst, cap_dst, depth, (const uint4*)src_root, (uint4*)dst_root);
    return launched();
}

template <class Check, class Launch>
int dev_form(mk_call* call, void* stream, const Check& check, const Launch& launch) {
    Scope S(call);
    int rc = check();
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = launch();
    return S.done(rc);
}

// ---- the handle -----------------------------------------------------------------------------------
int trie_truncate(mk_trie* t, uint64_t n) {
    if (!t) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    TRY(truncate_check(t->levels.p, t->cap, t->count, n, t->depth, t->root.p));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(truncate_launch(t->levels.p, t->cap, t->count, n, t->depth, t->root.p, st));
    HIPCHK(hipStreamSynchronize(st));
    t->count = n;
    return MK_OK;
}

int trie_fork_point(mk_trie* a, mk_trie* b, uint64_t* out) {
    if (!a || !b || !out) return fail(MK_EINVAL, "null pointer");
    if (a == b) {
        std::lock_guard<std::mutex> tl(a->mu);
        *out = a->count;
        return MK_OK;
    }
    // both handles' mutexes, the one at the lower address first
    std::mutex *first = &a->mu, *second = &b->mu;
    if (std::less<std::mutex*>()(second, first)) std::swap(first, second);
    std::lock_guard<std::mutex> l1(*first);
    std::lock_guard<std::mutex> l2(*second);
    if (a->depth != b->depth) return fail(MK_EINVAL, "tries of depth %u and %u", a->depth, b->depth);
    if (a->dev != b->dev) return fail(MK_EINVAL, "the tries live on devices %d and %d", a->dev, b->dev);
    TRY(fork_check(a->levels.p, a->cap, a->count, b->levels.p, b->cap, b->count, a->depth, a->branch.p));
    TRY(bind_dev(a->dev));
    hipStream_t st = ctx()->stream;
    TRY(fork_launch(a->levels.p, a->cap, a->count, b->levels.p, b->cap, b->count, a->depth, a->branch.p, st));
    HIPCHK(hipMemcpyAsync(out, a->branch.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int trie_audit(mk_trie* t, mk_audit_report* out) {
    if (!t || !out) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (t->count == 0) {  // the handle's root reads 0^32 without a device word behind it (trie_root)
        *out = mk_audit_report{0, ~0ull, MK_AUDIT_NONE, 0};
        return MK_OK;
    }
    TRY(audit_check(t->levels.p, t->cap, t->count, t->depth, t->root.p, t->branch.p));
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(audit_launch(t->levels.p, t->cap, t->count, t->depth, t->root.p, t->branch.p, st));
    HIPCHK(hipMemcpyAsync(out, t->branch.p, sizeof *out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// src's live nodes into a fresh level array of `cap` leaves (and src's root into `root`, when given); the
// caller holds src's lock with the device bound and installs or frees nl
int copy_into_new(mk_trie* src, uint64_t cap, DevBuf& nl, void* root) {
    TRY(grow(nl, mk_deposit_trie_levels_bytes(cap, src->depth)));
    hipStream_t st = ctx()->stream;
    const void* sroot = root && src->count ? src->root.p : nullptr;
    int rc = copy_check(src->levels.p, src->cap, src->count, nl.p, cap, src->depth, sroot, sroot ? root : nullptr);
    if (!rc) rc = copy_launch(src->levels.p, src->cap, src->count, nl.p, cap, src->depth, sroot, sroot ? root : nullptr, st);
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(MK_EHIP, "hipStreamSynchronize failed");
    if (rc) {
        (void)hipFree(nl.p);
        nl = DevBuf{};
    }
    return rc;
}

int trie_clone(mk_trie* src, mk_trie** out) {
    if (!src || !out) return fail(MK_EINVAL, "null pointer");
    *out = nullptr;
    std::lock_guard<std::mutex> tl(src->mu);
    TRY(bind_dev(src->dev));
    auto* t = new (std::nothrow) mk_trie();
    if (!t) return fail(MK_ENOMEM, "trie allocation failed");
    t->dev = src->dev;
    t->depth = src->depth;
    t->cap = src->cap;
    int rc = grow(t->root, 32);
    if (!rc) rc = grow(t->branch, 32 * (size_t)t->depth);
    if (!rc) rc = copy_into_new(src, t->cap, t->levels, t->root.p);
    if (rc) {
        mk_deposit_trie_free(t);
        return rc;
    }
    t->count = src->count;
    *out = t;
    return MK_OK;
}

int trie_copy(mk_trie* dst, mk_trie* src) {
    if (!dst || !src) return fail(MK_EINVAL, "null pointer");
    if (dst == src) return MK_OK;
    std::mutex *first = &dst->mu, *second = &src->mu;
    if (std::less<std::mutex*>()(second, first)) std::swap(first, second);
    std::lock_guard<std::mutex> l1(*first);
    std::lock_guard<std::mutex> l2(*second);
    if (dst->depth != src->depth) return fail(MK_EINVAL, "tries of depth %u and %u", dst->depth, src->depth);
    if (dst->dev != src->dev) return fail(MK_EINVAL, "the tries live on devices %d and %d", dst->dev, src->dev);
    TRY(bind_dev(src->dev));
    hipStream_t st = ctx()->stream;
    if (src->count > dst->cap) {  // dst grows to src's capacity; a failure leaves it as it was
        DevBuf nl;
        TRY(copy_into_new(src, src->cap, nl, dst->root.p));
        (void)hipFree(dst->levels.p);
        dst->levels = nl;
        dst->cap = src->cap;
    } else {
        const void* sroot = src->count ? src->root.p : nullptr;
        TRY(copy_check(src->levels.p, src->cap, src->count, dst->levels.p, dst->cap, src->depth, sroot,
                       sroot ? dst->root.p : nullptr));
        TRY(copy_launch(src->levels.p, src->cap, src->count, dst->levels.p, dst->cap, src->depth, sroot,
                        sroot ? dst->root.p : nullptr, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    dst->count = src->count;
    return MK_OK;
}

int trie_reserve(mk_trie* t, uint64_t capacity) {
    if (!t) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (t->depth < 63 && capacity > (1ull << t->depth))
        return fail(MK_EINVAL, "capacity %llu beyond a depth-%u trie", (unsigned long long)capacity, t->depth);
    if (capacity <= t->cap) return MK_OK;
    TRY(bind_dev(t->dev));
    DevBuf nl;
    TRY(copy_into_new(t, capacity, nl, nullptr));  // the root stays where it is
    (void)hipFree(t->levels.p);
    t->levels = nl;
    t->cap = capacity;
    return MK_OK;
}

}  // namespace

extern "C" {

int mk_dev_deposit_trie_truncate(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, uint64_t new_count,
                                 uint32_t depth, void* d_root32, void* stream) {
    return dev_form(
        call, stream, [&] { return truncate_check(d_levels, capacity, count, new_count, depth, d_root32); },
        [&] { return truncate_launch(d_levels, capacity, count, new_count, depth, d_root32, (hipStream_t)stream); });
}

int mk_dev_deposit_trie_fork_point(mk_call* call, const void* d_levels_a, uint64_t capacity_a, uint64_t count_a,
                                   const void* d_levels_b, uint64_t capacity_b, uint64_t count_b, uint32_t depth,
                                   void* d_out8, void* stream) {
    return dev_form(
        call, stream,
        [&] { return fork_check(d_levels_a, capacity_a, count_a, d_levels_b, capacity_b, count_b, depth, d_out8); },
        [&] {
            return fork_launch(d_levels_a, capacity_a, count_a, d_levels_b, capacity_b, count_b, depth, d_out8,
                               (hipStream_t)stream);
        });
}

int mk_dev_deposit_trie_audit(mk_call* call, const void* d_levels, uint64_t capacity, uint64_t count, uint32_t depth,
                              const void* d_root32, void* d_report, void* stream) {
    return dev_form(
        call, stream, [&] { return audit_check(d_levels, capacity, count, depth, d_root32, d_report); },
        [&] { return audit_launch(d_levels, capacity, count, depth, d_root32, d_report, (hipStream_t)stream); });
}

int mk_dev_deposit_trie_copy(mk_call* call, const void* d_src_levels, uint64_t src_capacity, uint64_t count,
                             void* d_dst_levels, uint64_t dst_capacity, uint32_t depth, const void* d_src_root32,
                             void* d_dst_root32, void* stream) {
    return dev_form(
        call, stream,
        [&] {
            return copy_check(d_src_levels, src_capacity, count, d_dst_levels, dst_capacity, depth, d_src_root32,
                              d_dst_root32);
        },
        [&] {
            return copy_launch(d_src_levels, src_capacity, count, d_dst_levels, dst_capacity, depth, d_src_root32,
                               d_dst_root32, (hipStream_t)stream);
        });
}

int mk_deposit_trie_truncate(mk_call* call, mk_trie* t, uint64_t n) {
    Scope S(call);
    return S.done(trie_truncate(t, n));
}

int mk_deposit_trie_fork_point(mk_call* call, mk_trie* a, mk_trie* b, uint64_t* out) {
    Scope S(call);
    return S.done(trie_fork_point(a, b, out));
}

int mk_deposit_trie_audit(mk_call* call, mk_trie* t, mk_audit_report* out) {
    Scope S(call);
    return S.done(trie_audit(t, out));
}

int mk_deposit_trie_clone(mk_call* call, mk_trie* src, mk_trie** out) {
    Scope S(call);
    return S.done(trie_clone(src, out));
}

int mk_deposit_trie_copy(mk_call* call, mk_trie* dst, mk_trie* src) {
    Scope S(call);
    return S.done(trie_copy(dst, src));
}

int mk_deposit_trie_reserve(mk_call* call, mk_trie* t, uint64_t capacity) {
    Scope S(call);
    return S.done(trie_reserve(t, capacity));
}

uint64_t mk_deposit_trie_capacity(const mk_trie* t) { return t ? t->cap : 0; }

}  // extern "C"
