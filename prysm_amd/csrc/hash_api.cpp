// Batched Keccak-256: the launch selection and the mk_hash* entry points.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

int host_hash_batch(const uint8_t* in, uint64_t n, uint32_t msg_len, uint8_t* out) {
    if (n && !in && msg_len) return fail(MK_EINVAL, "null input");
    if (n && !out) return fail(MK_EINVAL, "null output");
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t inb = n * (size_t)msg_len;
    TRY(grow(c->in, inb));
    TRY(grow(c->out, 32 * n));
    hipStream_t st = c->stream;
    if (inb) HIPCHK(hipMemcpyAsync(c->in.p, in, inb, hipMemcpyHostToDevice, st));
    TRY(dev_hash_batch(c->in.p, n, msg_len, c->out.p, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int host_hash_var(const uint8_t* in, const uint64_t* offs, uint64_t n, uint8_t* out) {
    if (n && (!offs || !out)) return fail(MK_EINVAL, "null pointer");
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t inb = offs[n] - offs[0];
    TRY(grow(c->in, inb));
    TRY(grow(c->aux, 8 * (n + 1)));
    TRY(grow(c->out, 32 * n));
    hipStream_t st = c->stream;
    std::vector<uint64_t> rel(offs, offs + n + 1);
    for (auto& o : rel) o -= offs[0];
    if (inb) HIPCHK(hipMemcpyAsync(c->in.p, in + offs[0], inb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->aux.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
    TRY(dev_hash_var(c->in.p, (const uint64_t*)c->aux.p, n, c->out.p, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int dev_hash_batch(const void* d_in, uint64_t n, uint32_t msg_len, void* d_out, hipStream_t st) {
    if (n == 0) return MK_OK;
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    if (!d_out || (!d_in && msg_len)) return fail(MK_EINVAL, "null pointer");
    const uint64_t grid = ceil_div(n, 256);
    if (msg_len == 64 && ((uintptr_t)d_in % 16) == 0 && ((uintptr_t)d_out % 16) == 0) {
        if (n >= (1u << 18))  // phase-locked (a partial last group included)
            hipLaunchKernelGGL(mk::k_keccak64_lock,
                               dim3(std::min<uint64_t>(ceil_div(n, mk::kLockThreads), lock_grid_cap(st))),
                               dim3(mk::kLockThreads), 0, st, (const uint4*)d_in, n, (uint4*)d_out);
        else
            hipLaunchKernelGGL(mk::k_keccak64, dim3(grid), dim3(256), 0, st, (const uint4*)d_in, n, (uint4*)d_out);
    } else if (msg_len == 280 && ((uintptr_t)d_in % 8) == 0 && ((uintptr_t)d_out % 16) == 0) {
        hipLaunchKernelGGL((mk::k_keccak_rec<35>), dim3(std::min<uint64_t>(ceil_div(n, mk::kRecThreads), mk::kRecGridMax)),
                           dim3(mk::kRecThreads), 0, st, (const uint2*)d_in, n, (uint4*)d_out);
    } else if (msg_len % 8 == 0 && msg_len > 0 && ((uintptr_t)d_in % 8) == 0 && ((uintptr_t)d_out % 16) == 0) {
        hipLaunchKernelGGL(mk::k_keccak_words, dim3(grid), dim3(256), 0, st, (const uint2*)d_in, n, msg_len / 8,
                           (uint4*)d_out);
    } else {
        hipLaunchKernelGGL(mk::k_keccak_fixed, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_in, n, msg_len,
                           (uint4*)d_out);
    }
    return launched();
}

int dev_hash_var(const void* d_in, const uint64_t* d_offs, uint64_t n, void* d_out, hipStream_t st) {
    if (n == 0) return MK_OK;
    if (!d_offs || !d_out) return fail(MK_EINVAL, "null pointer");
    hipLaunchKernelGGL(mk::k_keccak_var, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const uint8_t*)d_in, d_offs, n,
                       (uint4*)d_out);
    return launched();
}

// Uniform message length of offs[0..n] (relative), or -1.
int64_t uniform_len(const uint64_t* offs, uint64_t n) {
    const uint64_t len0 = offs[1] - offs[0];
    for (uint64_t i = 1; i < n; ++i)
        if (offs[i + 1] - offs[i] != len0) return -1;
    return len0 <= UINT32_MAX ? (int64_t)len0 : -1;
}

}  // namespace mk::rt

extern "C" {

int mk_dev_hash_batch(mk_call* call, const void* d_in, uint64_t n, uint32_t msg_len, void* d_out, void* stream) {
    return dev_entry(call, stream, [&] { return dev_hash_batch(d_in, n, msg_len, d_out, (hipStream_t)stream); });
}

int mk_dev_hash_batch_var(mk_call* call, const void* d_in, const uint64_t* d_offs, uint64_t n, void* d_out,
                          void* stream) {
    return dev_entry(call, stream, [&] { return dev_hash_var(d_in, d_offs, n, d_out, (hipStream_t)stream); });
}

int mk_hash_batch(mk_call* call, const uint8_t* in, uint64_t n, uint32_t msg_len, uint8_t* out) {
    Scope S(call);
    return S.done(host_hash_batch(in, n, msg_len, out));
}

int mk_hash_batch_var(mk_call* call, const uint8_t* in, const uint64_t* offs, uint64_t n, uint8_t* out) {
    Scope S(call);
    return S.done(host_hash_var(in, offs, n, out));
}

int mk_hash(mk_call* call, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    Scope S(call);
    if (len && !data) return S.done(fail(MK_EINVAL, "null input"));
    if (len > UINT32_MAX) {
        uint64_t offs[2] = {0, len};
        return S.done(host_hash_var(data, offs, 1, out));
    }
    static const uint8_t empty = 0;
    return S.done(host_hash_batch(len ? data : &empty, 1, (uint32_t)len, out));
}

}  // extern "C"
