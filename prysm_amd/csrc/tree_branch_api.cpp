// Merkle proofs out of the resident list trees and their batched verifier
// (DESIGN.md §5l): the device entry points over a tree's level 0 and levels,
// the verifier from device and from host buffers.  The handle calls
// (mk_*_tree_branches, mk_tree_set_branches) are tree_handle.cpp's and
// tree_set_api.cpp's; the index arithmetic is list_branch.hpp's.
#include "list_branch.hpp"
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

constexpr uint64_t kListBranchGridMax = 2048;  // workgroups: 8 per CU, the rest by grid stride

int check_item_len(uint32_t item_len) {
    if (item_len == 0) return fail(MK_EINVAL, "item_len == 0");
    if (item_len > kBranchItemMax)
        return fail(MK_EINVAL, "item_len %u above %u: no proof record (a window of 2 x item_len)", item_len,
                    kBranchItemMax);
    return MK_OK;
}

int check_k(uint64_t k) {
    if (k >= kMaxWork) return fail(MK_EINVAL, "%llu proofs in one call (limit 2^31 - 1)", (unsigned long long)k);
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int list_branches_check(const void* d_level0, uint64_t n, uint64_t capacity, uint32_t item_len, const void* d_levels,
                        const uint64_t* d_idx, uint64_t k, const void* d_branches) {
    TRY(check_item_len(item_len));
    if (n > capacity)
        return fail(MK_EINVAL, "%llu items > capacity %llu", (unsigned long long)n, (unsigned long long)capacity);
    if (capacity > UINT64_MAX / item_len) return fail(MK_EINVAL, "capacity * item_len overflows");
    TRY(check_k(k));
    if (k && (!d_idx || !d_branches)) return fail(MK_EINVAL, "null pointer");
    if (n && !d_level0) return fail(MK_EINVAL, "null level 0");
    if (branch_shape(n, capacity, item_len).D > 1 && !d_levels) return fail(MK_EINVAL, "null level array");
    if (((uintptr_t)d_levels | (uintptr_t)d_branches) % 16 || (uintptr_t)d_idx % 8)
        return fail(MK_EINVAL, "levels and branches need 16-B alignment, indices 8-B");
    return MK_OK;
}

int list_branches_launch(const void* d_level0, uint64_t n, uint64_t capacity, uint32_t item_len, const void* d_levels,
                         const uint64_t* d_idx, uint64_t k, void* d_branches, hipStream_t st) {
    if (k == 0) return MK_OK;
    const uint64_t grid = std::min<uint64_t>(ceil_div(k, mk::kBranchWaves), kListBranchGridMax);
    hipLaunchKernelGGL(mk::k_list_tree_branches, dim3(grid), dim3(64 * mk::kBranchWaves), 0, st,
                       (const uint8_t*)d_level0, (const uint4*)d_levels, n, capacity, item_len, d_idx, k,
                       (uint4*)d_branches);
    return launched();
}

}  // namespace mk::rt

namespace {

// what can be said of a verify call without a device; the pointers are the device or the host ones
int verify_check(const void* values, const void* idx, uint64_t k, uint32_t item_len, const void* branches,
                 const void* roots, uint32_t root_stride, const void* container, uint32_t container_len,
                 uint32_t container_off, const void* ok) {
    TRY(check_item_len(item_len));
    TRY(check_k(k));
    if (root_stride != 0 && root_stride != 32)
        return fail(MK_EINVAL, "root_stride %u (0: one root for the batch, 32: one per proof)", root_stride);
    if (container) {
        if (container_len > MK_CONTAINER_MAX)
            return fail(MK_EINVAL, "container of %u bytes (limit %d)", container_len, MK_CONTAINER_MAX);
        if ((uint64_t)container_off + 32 > container_len)
            return fail(MK_EINVAL, "root at offset %u beyond the %u-byte container", container_off, container_len);
    }
    if (k && (!values || !idx || !branches || !roots || !ok)) return fail(MK_EINVAL, "null pointer");
    return MK_OK;
}

int verify_launch(const void* d_values, const uint64_t* d_idx, uint64_t k, uint64_t n, uint32_t item_len,
                  const void* d_branches, const void* d_roots, uint32_t root_stride, const void* d_container,
                  uint32_t container_len, uint32_t container_off, void* d_ok, hipStream_t st) {
    if (k == 0) return MK_OK;
    hipLaunchKernelGGL(mk::k_verify_list_branches, dim3(ceil_div(k, 256)), dim3(256), 0, st, (const uint8_t*)d_values,
                       d_idx, k, n, item_len, (const uint8_t*)d_branches, (const uint8_t*)d_roots, root_stride,
                       (const uint8_t*)d_container, container_len, container_off, (uint8_t*)d_ok);
    return launched();
}

int host_verify_list_branches(const uint8_t* values, const uint64_t* idx, uint64_t k, uint64_t n, uint32_t item_len,
                              const uint8_t* branches, const uint8_t* roots, uint32_t root_stride,
                              const uint8_t* container, uint32_t container_len, uint32_t container_off, uint8_t* ok) {
    TRY(verify_check(values, idx, k, item_len, branches, roots, root_stride, container, container_len, container_off,
                     ok));
    if (n > UINT64_MAX / item_len) return fail(MK_EINVAL, "n * item_len overflows");
    TRY(bind_call());
    if (k == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    const size_t stride = mk_ssz_list_branch_bytes(n, item_len);
    const size_t bb = stride * k, rb = align256(root_stride ? 32 * k : 32), cb = container ? align256(container_len) : 0;
    const size_t vb = (size_t)item_len * k;
    // in: [branches | roots | container | values], aux: the indices
    TRY(grow(c->in, bb + rb + cb + vb + 16));
    TRY(grow(c->aux, 8 * k));
    TRY(grow(c->out, k));
    uint8_t* d_br = (uint8_t*)c->in.p;
    uint8_t* d_roots = d_br + bb;
    uint8_t* d_cont = d_roots + rb;
    uint8_t* d_vals = d_cont + cb;
    HIPCHK(hipMemcpyAsync(d_br, branches, bb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_roots, roots, root_stride ? 32 * k : 32, hipMemcpyHostToDevice, st));
    if (container && container_len)
        HIPCHK(hipMemcpyAsync(d_cont, container, container_len, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_vals, values, vb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->aux.p, idx, 8 * k, hipMemcpyHostToDevice, st));
    TRY(verify_launch(d_vals, (const uint64_t*)c->aux.p, k, n, item_len, d_br, d_roots, root_stride,
                      container ? d_cont : nullptr, container_len, container_off, c->out.p, st));
    HIPCHK(hipMemcpyAsync(ok, c->out.p, k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the caller's buffers are released after this
    return MK_OK;
}

}  // namespace

extern "C" {

uint64_t mk_ssz_list_branch_bytes(uint64_t n, uint32_t item_len) {
    if (item_len == 0 || item_len > kBranchItemMax) return 0;
    return branch_record_bytes(branch_shape(n, n, item_len));
}

// Every argument check comes before the stream's device is looked up: a bad
// call is MK_EINVAL on any machine.  One launch, nothing allocated, no
// synchronise: capturable.
int mk_dev_ssz_list_tree_branches(mk_call* call, const void* d_level0, uint64_t n, uint64_t capacity,
                                  uint32_t item_len, const void* d_levels, const uint64_t* d_idx, uint64_t k,
                                  void* d_branches, void* stream) {
    Scope S(call);
    int rc = list_branches_check(d_level0, n, capacity, item_len, d_levels, d_idx, k, d_branches);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = list_branches_launch(d_level0, n, capacity, item_len, d_levels, d_idx, k, d_branches,
                                  (hipStream_t)stream);
    return S.done(rc);
}

int mk_dev_verify_list_branches(mk_call* call, const void* d_values, const uint64_t* d_idx, uint64_t k, uint64_t n,
                                uint32_t item_len, const void* d_branches, const void* d_roots, uint32_t root_stride,
                                const void* d_container, uint32_t container_len, uint32_t container_off, void* d_ok,
                                void* stream) {
    Scope S(call);
    int rc = verify_check(d_values, d_idx, k, item_len, d_branches, d_roots, root_stride, d_container, container_len,
                          container_off, d_ok);
    if (!rc && n > UINT64_MAX / item_len) rc = fail(MK_EINVAL, "n * item_len overflows");
    if (!rc && (((uintptr_t)d_branches % 16) || ((uintptr_t)d_roots % 4) || ((uintptr_t)d_idx % 8)))
        rc = fail(MK_EINVAL, "branches need 16-B alignment, indices 8-B, roots 4-B");
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = verify_launch(d_values, d_idx, k, n, item_len, d_branches, d_roots, root_stride, d_container,
                           container_len, container_off, d_ok, (hipStream_t)stream);
    return S.done(rc);
}

int mk_verify_list_branches(mk_call* call, const uint8_t* values, const uint64_t* idx, uint64_t k, uint64_t n,
                            uint32_t item_len, const uint8_t* branches, const uint8_t* roots, uint32_t root_stride,
                            const uint8_t* container, uint32_t container_len, uint32_t container_off, uint8_t* ok) {
    Scope S(call);
    return S.done(host_verify_list_branches(values, idx, k, n, item_len, branches, roots, root_stride, container,
                                            container_len, container_off, ok));
}

}  // extern "C"
