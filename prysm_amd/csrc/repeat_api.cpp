// hashutil.RepeatHash in batches: the launch selection and the mk_*repeat_hash*, mk_*hash_onion
// entry points; the kernels are kernels_repeat.hip.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace mk::rt {

// what every entry checks before anything else: the cap, the form, the size of one launch
int repeat_check_call(uint64_t n, uint32_t max_layers, uint32_t form) {
    if (max_layers > MK_REPEAT_MAX_LAYERS)
        return fail(MK_EINVAL, "max_layers %u above MK_REPEAT_MAX_LAYERS (%u)", max_layers, MK_REPEAT_MAX_LAYERS);
    if (form != MK_REPEAT_AUTO && form != MK_REPEAT_LANE && form != MK_REPEAT_WAVE)
        return fail(MK_EINVAL, "unknown form %u", form);
    if (n >= kMaxWork) return fail(MK_EINVAL, "%llu chains in one call (limit 2^31 - 1)", (unsigned long long)n);
    return MK_OK;
}

int repeat_check_offsets(uint64_t stride, uint32_t commit_off, uint32_t layers_off, const char* what) {
    if ((uint64_t)commit_off + 32 > stride)
        return fail(MK_EINVAL, "commit_off %u + 32 beyond the %s %llu", commit_off, what, (unsigned long long)stride);
    if ((uint64_t)layers_off + 8 > stride)
        return fail(MK_EINVAL, "layers_off %u + 8 beyond the %s %llu", layers_off, what, (unsigned long long)stride);
    return MK_OK;
}

int repeat_check_indices(const uint64_t* idx, uint64_t m, uint64_t count, const char* noun) {
    for (uint64_t j = 0; j < m; ++j)
        if (idx[j] >= count)
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[j], (unsigned long long)count,
                        noun);
    return MK_OK;
}

}  // namespace mk::rt

namespace {

// MK_REPEAT_AUTO: one chain per wave up to this many chains, one per GPU lane above.  The largest probed count at
// which the forced wave form is not the slower one: at 16 layers it takes 0.79 of the lane form's time at 4,096
// chains and 1.39 at 8,192 (`crossing_l16` of profiles/repeat_hash/probe.json, tools/repeat_hash_probe.py;
// DESIGN.md §5s).
constexpr uint64_t kRepeatWaveMax = 4096;



bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// one launch of a.n >= 1 chains; the arguments are checked
template <int MODE>
int launch(const RepeatArgs& a, uint32_t form, hipStream_t st) {
    const bool wave = form == MK_REPEAT_WAVE || (form == MK_REPEAT_AUTO && a.n <= kRepeatWaveMax);
    if (wave)
        hipLaunchKernelGGL((mk::k_repeat_wave<MODE>), dim3((uint32_t)ceil_div(a.n, mk::kRepeatWaves)),
                           dim3(mk::kRepeatThreads), 0, st, a);
    else
        hipLaunchKernelGGL((mk::k_repeat_lane<MODE>), dim3((uint32_t)ceil_div(a.n, mk::kRepeatThreads)),
                           dim3(mk::kRepeatThreads), 0, st, a);
    return launched();
}

int dev_chain(const void* d_seeds, const uint32_t* d_layers, uint64_t n, uint32_t max_layers, uint32_t form,
              void* d_out, uint32_t* d_status, hipStream_t st) {
    RepeatArgs a{};
    a.seeds = (const uint8_t*)d_seeds, a.layers = d_layers, a.out = (uint8_t*)d_out, a.status = d_status;
    a.n = n, a.max_layers = max_layers;
    a.io16 = al16(d_seeds) && al16(d_out);
    return launch<kRepeatChain>(a, form, st);
}

int dev_onion(const void* d_seeds, uint64_t n, uint32_t layers, uint32_t form, void* d_out, hipStream_t st) {
    RepeatArgs a{};
    a.seeds = (const uint8_t*)d_seeds, a.out = (uint8_t*)d_out;
    a.n = n, a.max_layers = layers;
    a.io16 = al16(d_seeds) && al16(d_out);
    return launch<kRepeatOnion>(a, form, st);
}

int dev_verify(const void* d_records, uint64_t n_records, uint64_t stride, uint32_t commit_off, uint32_t layers_off,
               const uint64_t* d_idx, const void* d_reveals, uint64_t m, uint32_t max_layers, uint32_t form,
               uint8_t* d_ok, hipStream_t st) {
    RepeatArgs a{};
    a.seeds = (const uint8_t*)d_reveals, a.out = d_ok, a.records = (const uint8_t*)d_records, a.idx = d_idx;
    a.n = m, a.n_records = n_records, a.stride = stride;
    a.commit_off = commit_off, a.layers_off = layers_off, a.max_layers = max_layers;
    a.io16 = al16(d_reveals);
    a.rec4 = ((uintptr_t)d_records % 4) == 0 && stride % 4 == 0 && commit_off % 4 == 0 && layers_off % 4 == 0;
    return launch<kRepeatVerify>(a, form, st);
}

int host_chain(const uint8_t* seeds, const uint32_t* layers, uint64_t n, uint32_t max_layers, uint8_t* out) {
    TRY(repeat_check_call(n, max_layers, MK_REPEAT_AUTO));
    if (n && (!seeds || !layers || !out)) return fail(MK_EINVAL, "null pointer");
    for (uint64_t i = 0; i < n; ++i)
        if (layers[i] > max_layers)
            return fail(MK_EINVAL, "layers[%llu] = %u above max_layers %u", (unsigned long long)i, layers[i],
                        max_layers);
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    TRY(grow(c->in, 32 * n));
    TRY(grow(c->aux, 4 * n));
    TRY(grow(c->out, 32 * n));
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(c->in.p, seeds, 32 * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->aux.p, layers, 4 * n, hipMemcpyHostToDevice, st));
    TRY(dev_chain(c->in.p, (const uint32_t*)c->aux.p, n, max_layers, MK_REPEAT_AUTO, c->out.p, nullptr, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int host_onion(const uint8_t* seeds, uint64_t n, uint32_t layers, uint8_t* out) {
    TRY(repeat_check_call(n, layers, MK_REPEAT_AUTO));
    if (n && (!seeds || !out)) return fail(MK_EINVAL, "null pointer");
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t outb = 32 * n * ((size_t)layers + 1);
    TRY(grow(c->in, 32 * n));
    TRY(grow(c->out, outb));
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(c->in.p, seeds, 32 * n, hipMemcpyHostToDevice, st));
    TRY(dev_onion(c->in.p, n, layers, MK_REPEAT_AUTO, c->out.p, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, outb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}


int host_verify(const uint8_t* records, uint64_t n_records, uint64_t stride, uint32_t commit_off, uint32_t layers_off,
                const uint64_t* idx, const uint8_t* reveals, uint64_t m, uint32_t max_layers, uint8_t* ok) {
    TRY(repeat_check_call(m, max_layers, MK_REPEAT_AUTO));
    if (m && (!idx || !reveals || !ok || (n_records && !records))) return fail(MK_EINVAL, "null pointer");
    TRY(repeat_check_offsets(stride, commit_off, layers_off, "stride"));
    if (n_records > UINT64_MAX / stride) return fail(MK_EINVAL, "n_records * stride overflows");
    TRY(repeat_check_indices(idx, m, n_records, "records"));
    TRY(bind_call());
    if (m == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t recb = n_records * stride;
    TRY(grow(c->in, recb));
    TRY(grow(c->aux, 8 * m));
    TRY(grow(c->ws, 32 * m));
    TRY(grow(c->out, m));
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(c->in.p, records, recb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->aux.p, idx, 8 * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->ws.p, reveals, 32 * m, hipMemcpyHostToDevice, st));
    TRY(dev_verify(c->in.p, n_records, stride, commit_off, layers_off, (const uint64_t*)c->aux.p, c->ws.p, m,
                   max_layers, MK_REPEAT_AUTO, (uint8_t*)c->out.p, st));
    HIPCHK(hipMemcpyAsync(ok, c->out.p, m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int tree_verify_repeat_hash(TreeHandle* t, uint32_t commit_off, uint32_t layers_off, const uint64_t* idx,
                            const uint8_t* reveals, uint64_t m, uint32_t max_layers, uint8_t* ok) {
    if (!t || (m && (!idx || !reveals || !ok))) return fail(MK_EINVAL, "null pointer");
    TRY(repeat_check_call(m, max_layers, MK_REPEAT_AUTO));
    std::lock_guard<std::mutex> tl(t->mu);
    if (t->kind->id != MK_TREE_STRUCT)
        return fail(MK_EINVAL, "a %s has no records: the verify takes a struct list tree", t->kind->name);
    TRY(repeat_check_offsets(t->item_len, commit_off, layers_off, "record length"));
    TRY(repeat_check_indices(idx, m, t->count, t->kind->noun));
    if (m == 0) return MK_OK;
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(grow(t->idx, 8 * m));
    TRY(grow(t->ws, 33 * m));  // the reveals, then the verdicts
    uint8_t* d_ok = (uint8_t*)t->ws.p + 32 * m;
    HIPCHK(hipMemcpyAsync(t->idx.p, idx, 8 * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t->ws.p, reveals, 32 * m, hipMemcpyHostToDevice, st));
    TRY(dev_verify(t->items.p, t->count, t->item_len, commit_off, layers_off, (const uint64_t*)t->idx.p, t->ws.p, m,
                   max_layers, MK_REPEAT_AUTO, d_ok, st));
    HIPCHK(hipMemcpyAsync(ok, d_ok, m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // idx and the reveals are released after this
    return MK_OK;
}

}  // namespace mk::rt

extern "C" {

int mk_dev_repeat_hash(mk_call* call, const void* d_seeds, const uint32_t* d_layers, uint64_t n, uint32_t max_layers,
                       uint32_t form, void* d_out, uint32_t* d_status, void* stream) {
    return dev_entry(call, stream, [&] {
        TRY(repeat_check_call(n, max_layers, form));
        if (n == 0) return (int)MK_OK;
        if (!d_seeds || !d_layers || !d_out || !d_status) return fail(MK_EINVAL, "null pointer");
        if ((uintptr_t)d_layers % 4 || (uintptr_t)d_status % 4)
            return fail(MK_EINVAL, "d_layers and d_status must be 4-byte aligned");
        return dev_chain(d_seeds, d_layers, n, max_layers, form, d_out, d_status, (hipStream_t)stream);
    });
}

int mk_dev_hash_onion(mk_call* call, const void* d_seeds, uint64_t n, uint32_t layers, uint32_t form, void* d_out,
                      void* stream) {
    return dev_entry(call, stream, [&] {
        TRY(repeat_check_call(n, layers, form));
        if (n == 0) return (int)MK_OK;
        if (!d_seeds || !d_out) return fail(MK_EINVAL, "null pointer");
        return dev_onion(d_seeds, n, layers, form, d_out, (hipStream_t)stream);
    });
}

int mk_dev_verify_repeat_hash(mk_call* call, const void* d_records, uint64_t n_records, uint64_t stride,
                              uint32_t commit_off, uint32_t layers_off, const uint64_t* d_idx, const void* d_reveals,
                              uint64_t m, uint32_t max_layers, uint32_t form, uint8_t* d_ok, void* stream) {
    return dev_entry(call, stream, [&] {
        TRY(repeat_check_call(m, max_layers, form));
        TRY(repeat_check_offsets(stride, commit_off, layers_off, "stride"));
        if (n_records > UINT64_MAX / stride) return fail(MK_EINVAL, "n_records * stride overflows");
        if (m == 0) return (int)MK_OK;
        if (!d_idx || !d_reveals || !d_ok || (n_records && !d_records)) return fail(MK_EINVAL, "null pointer");
        if ((uintptr_t)d_idx % 8) return fail(MK_EINVAL, "d_idx must be 8-byte aligned");
        return dev_verify(d_records, n_records, stride, commit_off, layers_off, d_idx, d_reveals, m, max_layers, form,
                          d_ok, (hipStream_t)stream);
    });
}

int mk_repeat_hash_batch(mk_call* call, const uint8_t* seeds, const uint32_t* layers, uint64_t n, uint32_t max_layers,
                         uint8_t* out) {
    Scope S(call);
    return S.done(host_chain(seeds, layers, n, max_layers, out));
}

int mk_repeat_hash(mk_call* call, const uint8_t data[32], uint64_t num_times, uint8_t out[32]) {
    Scope S(call);
    if (!data || !out) return S.done(fail(MK_EINVAL, "null pointer"));
    if (num_times > MK_REPEAT_MAX_LAYERS)
        return S.done(fail(MK_EINVAL, "num_times %llu above MK_REPEAT_MAX_LAYERS (%u)", (unsigned long long)num_times,
                           MK_REPEAT_MAX_LAYERS));
    const uint32_t layers = (uint32_t)num_times;
    return S.done(host_chain(data, &layers, 1, MK_REPEAT_MAX_LAYERS, out));
}

int mk_hash_onion(mk_call* call, const uint8_t* seeds, uint64_t n, uint32_t layers, uint8_t* out) {
    Scope S(call);
    return S.done(host_onion(seeds, n, layers, out));
}

int mk_verify_repeat_hash(mk_call* call, const uint8_t* records, uint64_t n_records, uint64_t stride,
                          uint32_t commit_off, uint32_t layers_off, const uint64_t* idx, const uint8_t* reveals,
                          uint64_t m, uint32_t max_layers, uint8_t* ok) {
    Scope S(call);
    return S.done(host_verify(records, n_records, stride, commit_off, layers_off, idx, reveals, m, max_layers, ok));
}

}  // extern "C"
