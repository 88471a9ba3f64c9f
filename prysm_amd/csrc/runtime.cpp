// The device context of the C ABI: devices, streams, buffers, the per-call
// scope's binding, small uploads, the test hooks and the profiling records.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

std::mutex g_mu;  // g_ndev, g_ctx
int g_ndev = -1;
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;

}  // namespace

namespace mk::rt {

std::vector<DevCtx*> g_ctx;
thread_local int t_bound = -1;

int grow(DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return MK_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) return fail(MK_ENOMEM, "hipMalloc(%zu) failed", bytes);
    b.cap = bytes;
    return MK_OK;
}

int probe_devices() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ndev >= 0) return g_ndev;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    int good = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) break;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;  // gfx950 only
        ++good;
    }
    g_ndev = good;
    g_ctx.resize(good, nullptr);
    return g_ndev;
}

// Makes `dev` the thread's current device and creates its context once.
int bind_dev(int dev) {
    if (probe_devices() <= 0) return fail(MK_ENODEV, "no gfx950 device visible");
    if (dev < 0 || dev >= g_ndev) return fail(MK_ENODEV, "device %d out of range (%d visible)", dev, g_ndev);
    HIPCHK(hipSetDevice(dev));
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_ctx[dev]) {
        auto* c = new DevCtx();
        // side/copy streams at the highest priority: a default-priority
        // stream can share the caller's hardware queue (GPU_MAX_HW_QUEUES=4)
        // and then runs after, not beside, the work it should overlap
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) hi = lo = 0;
        bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, hi) == hipSuccess &&
                  hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&c->join, hipEventDisableTiming) == hipSuccess &&
                  hipStreamCreateWithPriority(&c->copy, hipStreamNonBlocking, hi) == hipSuccess &&
                  hipEventCreateWithFlags(&c->h2d, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < 2; ++i)
            ok = hipEventCreateWithFlags(&c->region_ev[i], hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < SmallStage::kSlots; ++i)
            ok = hipEventCreateWithFlags(&c->small.ev[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            delete c;
            return fail(MK_EHIP, "stream/event creation failed on device %d", dev);
        }
        g_ctx[dev] = c;
    }
    t_bound = dev;
    return MK_OK;
}

// The device a call runs on: call->device, else the thread's current device.
int bind_call() {
    const mk_call* c = mk::current_call();
    int dev = c ? c->device : -1;
    if (dev < 0) {
        if (probe_devices() <= 0) return fail(MK_ENODEV, "no gfx950 device visible");
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    return bind_dev(dev);
}

// dev entry points: the device of `stream` (call->device must agree), else as bind_call
int bind_stream(hipStream_t st) {
    if (!st) return bind_call();
    if (probe_devices() <= 0) return fail(MK_ENODEV, "no gfx950 device visible");
    hipDevice_t d = -1;
    HIPCHK(hipStreamGetDevice(st, &d));
    const mk_call* c = mk::current_call();
    if (c && c->device >= 0 && c->device != (int)d)
        return fail(MK_EINVAL, "stream belongs to device %d, call->device is %d", (int)d, c->device);
    return bind_dev((int)d);
}

// Uploads `bytes` of host data to device memory on `st` through the
// context's small pinned ring (the caller's buffer may die on return).
int upload_small(DevCtx* c, void* d_dst, const void* src, size_t bytes, hipStream_t st) {
    if (!bytes) return MK_OK;
    SmallStage& S = c->small;
    std::lock_guard<std::mutex> lk(S.mu);
    const int i = S.next;
    S.next = (S.next + 1) % SmallStage::kSlots;
    if (S.used[i]) HIPCHK(hipEventSynchronize(S.ev[i]));
    if (S.cap[i] < bytes) {
        if (S.host[i]) (void)hipHostFree(S.host[i]);
        S.host[i] = nullptr;
        S.cap[i] = 0;
        const size_t cap = std::max<size_t>(bytes, 64 << 10);
        if (hipHostMalloc(&S.host[i], cap, hipHostMallocDefault) != hipSuccess)
            return fail(MK_ENOMEM, "hipHostMalloc(%zu) failed", cap);
        S.cap[i] = cap;
    }
    std::memcpy(S.host[i], src, bytes);
    HIPCHK(hipMemcpyAsync(d_dst, S.host[i], bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(S.ev[i], st));
    S.used[i] = true;
    return MK_OK;
}

// Test hook (MK_INJECT_EHIP=1 in the environment when the library is
// loaded): every merkle plan launch and Hash batch fails the way a failed HIP
// launch does (MK_EHIP with its detail in the call's context), so a binding
// can prove a GPU failure reaches its caller as an error and is never
// answered by a CPU fallback (tests/c_abi/harness.c `inject`).
bool inject_ehip() {
    static const bool on = [] {
        const char* e = std::getenv("MK_INJECT_EHIP");
        return e && e[0] == '1';
    }();
    return on;
}

// Workgroups of a persistent phase-locked launch on `st`: one per CU the
// stream may use (its CU mask, hipExtStreamCreateWithCUMask), at most
// MK_LOCK_GRID.  A persistent 1024-thread workgroup needs a whole CU, so a
// grid larger than the stream's CUs would run a second, straggling round.
uint64_t lock_grid_cap(hipStream_t st) {
    // no stream query inside a graph capture (the default grid is recorded)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return MK_LOCK_GRID;
    }
    uint32_t m[16] = {0};  // up to 512 CUs
    if (hipExtStreamGetCUMask(st, 16, m) != hipSuccess) {
        (void)hipGetLastError();
        return MK_LOCK_GRID;
    }
    uint64_t c = 0;
    for (uint32_t w : m) c += (uint64_t)__builtin_popcount(w);
    return c ? std::min<uint64_t>(c, MK_LOCK_GRID) : MK_LOCK_GRID;
}

// ---- measurement -------------------------------------------------------------
bool prof_on() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    return g_prof_on;
}

void prof_enable(bool on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on;
}

int prof_begin(ProfRec& r, hipStream_t st) {
    HIPCHK(hipEventCreate(&r.a));
    HIPCHK(hipEventCreate(&r.b));
    HIPCHK(hipEventRecord(r.a, st));
    return MK_OK;
}

int prof_end(ProfRec& r, double perms, double hashes, hipStream_t st) {
    HIPCHK(hipEventRecord(r.b, st));
    r.perms = perms;
    r.hashes = hashes;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(r);
    return MK_OK;
}

int prof_read(double* leaf_ms, uint64_t* leaf_launches, double* leaf_perms, double* leaf_hashes) {
    std::vector<ProfRec> recs;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        recs.swap(g_prof);
    }
    double ms = 0, perms = 0, hashes = 0;
    for (auto& r : recs) {
        HIPCHK(hipEventSynchronize(r.b));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
        ms += t;
        perms += r.perms;
        hashes += r.hashes;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    if (leaf_ms) *leaf_ms = ms;
    if (leaf_launches) *leaf_launches = recs.size();
    if (leaf_perms) *leaf_perms = perms;
    if (leaf_hashes) *leaf_hashes = hashes;
    return MK_OK;
}

}  // namespace mk::rt
