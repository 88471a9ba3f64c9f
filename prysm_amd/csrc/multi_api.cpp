// merkleHash sharded over several devices (or several shards on one): the
// host-buffer path with overlapped uploads and the device-resident path,
// frontier blocks gathered over RCCL.
#include <rccl/rccl.h>

#include <map>
#include <string>
#include <thread>

#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

#define MK_STAGE_BYTES (32ull << 20)
constexpr size_t kStageBytes = MK_STAGE_BYTES;  // H2D chunk of the multi-device upload

// ---- multi-device ------------------------------------------------------------------------
std::mutex g_multi_mu;  // one multi-device call at a time (device locks are taken per device)
std::map<std::vector<int>, std::vector<ncclComm_t>> g_comms;

int comms_for(const std::vector<int>& devs, std::vector<ncclComm_t>*& out) {
    auto it = g_comms.find(devs);
    if (it == g_comms.end()) {
        std::vector<ncclComm_t> comms(devs.size(), nullptr);
        if (ncclCommInitAll(comms.data(), (int)devs.size(), devs.data()) != ncclSuccess)
            return fail(MK_ECOMM, "ncclCommInitAll(%zu) failed", devs.size());
        it = g_comms.emplace(devs, std::move(comms)).first;
    }
    out = &it->second;
    return MK_OK;
}

// Shard s of the frontier sharding reduced on the bound device: nodes of
// level (h - k) into d_block (k = 0: the 32-B shard root).
int launch_shard(const uint8_t* d_items, uint64_t sn, uint32_t item_len, uint32_t h, uint32_t k, uint8_t* d_block,
                 const DevBuf& ws, hipStream_t st) {
    if (sn == 0) {
        HIPCHK(hipMemsetAsync(d_block, 0, (size_t)32 << k, st));
        return MK_OK;
    }
    Plan p;
    TRY(mk::make_plan(sn, item_len, true, h, true, ((uintptr_t)d_items % 16) == 0, p, false, k));
    return launch_plan(p, d_items, d_block, (uint8_t*)ws.p, ws.cap, st);
}

uint32_t multi_frontier(uint32_t h) { return h > 5 ? std::min<uint32_t>(10, h - 5) : 0; }

// Test hook (MK_FORCE_COLLECTIVE=1 in the environment when the library is
// loaded): a one-device multi call takes the sharded path with one shard —
// frontier pass, ncclCommInitAll + in-place ncclAllGather over one rank,
// finisher — instead of the plain one-device merkleHash, so the library's
// RCCL code runs on a one-GPU box (RCCL refuses two ranks on one device).
bool force_collective() {
    static const bool on = [] {
        const char* e = std::getenv("MK_FORCE_COLLECTIVE");
        return e && e[0] == '1';
    }();
    return on;
}

// Uploads items[0, bytes) into d_dst on `copy`: chunked hipMemcpyAsync
// straight from the caller's pageable buffer, i.e. the runtime's own staged
// DMA (52-55 GB/s on one MI355X link).  The first multi-device form copied
// through two pinned slots with a host memcpy per chunk; one host thread's
// memcpy capped that at 22-35 GB/s (profiles/r02d/multi_host_probe.log).
int staged_upload(DevCtx* c, uint8_t* d_dst, const uint8_t* src, size_t bytes) {
    for (size_t off = 0; off < bytes; off += kStageBytes)
        HIPCHK(hipMemcpyAsync(d_dst + off, src + off, std::min(kStageBytes, bytes - off), hipMemcpyHostToDevice,
                              c->copy));
    return MK_OK;
}

struct MultiJob {
    int dev;
    std::vector<uint32_t> shards;  // shard indices on this device, in order
};

// Worker of mk_ssz_merkle_hash_multi for one device: its shards are uploaded
// into two alternating regions on the copy stream; each shard's passes run on
// the compute stream once its upload landed, while the next shard uploads.
// elem_len > 0 (the TreeHash-of-byte-strings path): `items` are elements of
// elem_len bytes and the tree's 32-B items are their digests
// K(le32(elem_len) || element); a shard's elements are uploaded, hashed into
// the matching digest region (k_elem_digests) and reduced from there.
int multi_device_worker(const MultiJob& job, const uint8_t* items, const std::vector<uint64_t>& begin,
                        uint32_t item_len, uint32_t h, uint32_t k, size_t block, uint32_t elem_len = 0) {
    TRY(bind_dev(job.dev));
    DevCtx* c = ctx();
    const size_t tree_region = (size_t)((1ull << h) * mk::chunk_bytes(item_len));  // tree items of a shard
    const size_t per_shard_items = tree_region / item_len;
    const size_t region = elem_len ? per_shard_items * elem_len : tree_region;     // uploaded bytes of a shard
    const int nreg = job.shards.size() > 1 ? 2 : 1;
    TRY(grow(c->in, std::max<size_t>(region, 16) * nreg));
    if (elem_len) TRY(grow(c->dig, tree_region * nreg));
    TRY(grow(c->out, block * (begin.size() - 1) + 32));
    Plan p;
    uint64_t wsb = 256;
    for (uint32_t s : job.shards) {
        const uint64_t sn = begin[s + 1] - begin[s];
        if (sn && mk::make_plan(sn, item_len, true, h, true, true, p, false, k) == MK_OK)
            wsb = std::max(wsb, mk::plan_ws_bytes(p));
    }
    TRY(grow(c->ws, wsb));
    c->region_used[0] = c->region_used[1] = false;
    for (size_t i = 0; i < job.shards.size(); ++i) {
        const uint32_t s = job.shards[i];
        const int r = (int)(i % 2);
        uint8_t* dreg = (uint8_t*)c->in.p + region * r;
        const uint64_t sn = begin[s + 1] - begin[s];
        const uint32_t up_len = elem_len ? elem_len : item_len;
        if (c->region_used[r]) HIPCHK(hipStreamWaitEvent(c->copy, c->region_ev[r], 0));  // its last shard is done
        TRY(staged_upload(c, dreg, items + begin[s] * up_len, sn * (size_t)up_len));
        HIPCHK(hipEventRecord(c->h2d, c->copy));
        HIPCHK(hipStreamWaitEvent(c->stream, c->h2d, 0));
        const uint8_t* tree_items = dreg;
        if (elem_len) {
            uint8_t* dg = (uint8_t*)c->dig.p + tree_region * r;
            TRY(launch_elem_digests(dreg, sn, elem_len, dg, c->stream));
            tree_items = dg;
        }
        TRY(launch_shard(tree_items, sn, item_len, h, k, (uint8_t*)c->out.p + block * s, c->ws, c->stream));
        HIPCHK(hipEventRecord(c->region_ev[r], c->stream));
        c->region_used[r] = true;
    }
    return MK_OK;
}

int dev_merkle_multi(const void* const* d_shards, uint64_t n, uint32_t item_len, int ndev, void* d_out32,
                     void* const* streams) {
    if (ndev <= 0 || !d_shards || !d_out32) return fail(MK_EINVAL, "bad arguments");
    if (probe_devices() < ndev) return fail(MK_ENODEV, "%d devices requested, %d visible", ndev, probe_devices());
    uint32_t h = 0, ne = 0;
    std::vector<uint64_t> begin(ndev + 1);
    TRY(mk::shard_plan(n, item_len, (uint32_t)ndev, &h, &ne, begin.data()));
    auto stream_of = [&](int d) { return streams && streams[d] ? (hipStream_t)streams[d] : g_ctx[d]->stream; };
    // one multi call at a time: the mout/mws/maux buffers and the communicator cache
    std::lock_guard<std::mutex> mlk(g_multi_mu);
    if (ne <= 1 && !(ndev == 1 && h > 5 && force_collective())) {
        TRY(bind_dev(0));
        DevCtx* c = ctx();
        Plan p;
        TRY(mk::make_plan(n, item_len, false, 0, false, ((uintptr_t)d_shards[0] % 16) == 0, p));
        TRY(grow(c->mws, p.small ? 256 : mk::plan_ws_bytes(p)));
        return launch_plan(p, (const uint8_t*)d_shards[0], (uint8_t*)d_out32, (uint8_t*)c->mws.p, c->mws.cap,
                           stream_of(0));
    }
    const uint32_t k = multi_frontier(h);
    const size_t block = (size_t)32 << k;
    const uint64_t last_nodes = k ? mk::frontier_nodes(begin[ne] - begin[ne - 1], item_len, h, k) : 1;
    const uint64_t count = ((uint64_t)(ne - 1) << k) + last_nodes;
    std::vector<int> devs(ndev);
    for (int d = 0; d < ndev; ++d) devs[d] = d;
    // size every buffer (and the communicators) before the first launch, so
    // no call frees or allocates between its own enqueues
    for (int d = 0; d < ndev; ++d) {
        TRY(bind_dev(d));
        DevCtx* c = ctx();
        TRY(grow(c->mout, block * ndev + 32));
        const uint64_t sn = begin[d + 1] - begin[d];
        Plan p;
        if (sn) {
            TRY(mk::make_plan(sn, item_len, true, h, true, ((uintptr_t)d_shards[d] % 16) == 0, p, false, k));
            TRY(grow(c->mws, mk::plan_ws_bytes(p)));
        }
        if (d == 0 && k) TRY(grow(c->maux, finish_ws_bytes(count)));
    }
    std::vector<ncclComm_t>* comms = nullptr;
    TRY(comms_for(devs, comms));
    for (int d = 0; d < ndev; ++d) {  // every device: its shard to the frontier level, block d
        TRY(bind_dev(d));
        DevCtx* c = ctx();
        TRY(launch_shard((const uint8_t*)d_shards[d], begin[d + 1] - begin[d], item_len, h, k,
                         (uint8_t*)c->mout.p + block * d, c->mws, stream_of(d)));
    }
    if (ncclGroupStart() != ncclSuccess) return fail(MK_ECOMM, "ncclGroupStart");
    for (int d = 0; d < ndev; ++d) {
        uint8_t* lvl = (uint8_t*)g_ctx[d]->mout.p;
        if (ncclAllGather(lvl + block * d, lvl, block, ncclUint8, (*comms)[d], stream_of(d)) != ncclSuccess) {
            ncclGroupEnd();
            return fail(MK_ECOMM, "ncclAllGather on device %d", d);
        }
    }
    if (ncclGroupEnd() != ncclSuccess) return fail(MK_ECOMM, "ncclGroupEnd");
    TRY(bind_dev(0));
    DevCtx* c0 = ctx();
    if (k) return dev_finish_nodes(c0->mout.p, count, n, d_out32, c0->maux.p, c0->maux.cap, stream_of(0));
    return dev_finish(c0->mout.p, ne, n, d_out32, stream_of(0));
}

}  // namespace

namespace mk::rt {

int host_merkle_multi(const uint8_t* items, uint64_t n, uint32_t item_len, int nshards, const int* devs_in,
                      uint8_t* out, uint32_t elem_len) {
    if (nshards <= 0) return fail(MK_EINVAL, "nshards %d <= 0", nshards);
    if (elem_len && item_len != 32) return fail(MK_EINVAL, "element digests are 32-B tree items");
    if (!out || (n && item_len && !items)) return fail(MK_EINVAL, "null pointer");
    const int nvis = probe_devices();
    if (nvis <= 0) return fail(MK_ENODEV, "no gfx950 device visible");
    std::vector<int> devs(nshards);
    for (int s = 0; s < nshards; ++s) {
        devs[s] = devs_in ? devs_in[s] : s;
        if (devs[s] < 0 || devs[s] >= nvis)
            return fail(MK_ENODEV, "shard %d: device %d out of range (%d visible)", s, devs[s], nvis);
    }
    uint32_t h = 0, ne = 0;
    std::vector<uint64_t> begin(nshards + 1);
    TRY(mk::shard_plan(n, item_len, (uint32_t)nshards, &h, &ne, begin.data()));
    if (ne <= 1 && !(nshards == 1 && h > 5 && force_collective())) {  // too small to shard: one device
        mk_call local{};
        local.device = devs[0];
        mk_call* prev = mk::swap_call(&local);
        const int rc = elem_len ? host_tree_hash_elems_plain(items, n, elem_len, out)
                                : host_merkle_hash_plain(items, n, item_len, out);
        mk::swap_call(prev);
        return rc ? fail(rc, "%s", local.err) : MK_OK;
    }
    std::vector<int> uniq;
    for (int d : devs)
        if (std::find(uniq.begin(), uniq.end(), d) == uniq.end()) uniq.push_back(d);
    const bool one_each = (int)uniq.size() == nshards;
    // several devices or RCCL: one multi-device call at a time (device lock
    // order, the communicator cache); shards on one device need only that
    // device's lock, so one-device calls on different devices stay concurrent
    std::unique_lock<std::mutex> mlk(g_multi_mu, std::defer_lock);
    if (uniq.size() > 1 || one_each) mlk.lock();
    const uint32_t k = multi_frontier(h);
    const size_t block = (size_t)32 << k;
    std::vector<MultiJob> jobs;
    for (int d : uniq) {
        MultiJob j{d, {}};
        for (int s = 0; s < nshards; ++s)
            if (devs[s] == d && begin[s + 1] > begin[s]) j.shards.push_back((uint32_t)s);
        jobs.push_back(j);
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int d : uniq) {
        TRY(bind_dev(d));
        locks.emplace_back(g_ctx[d]->mu);
    }
    // one host thread per device: uploads through pinned staging + the shard passes
    std::vector<int> rcs(jobs.size(), MK_OK);
    std::vector<std::string> errs(jobs.size());
    std::vector<std::thread> th;
    mk_call* parent = mk::current_call();
    for (size_t j = 0; j < jobs.size(); ++j)
        th.emplace_back([&, j]() {
            mk_call local{};
            local.device = jobs[j].dev;
            mk::swap_call(&local);
            rcs[j] = multi_device_worker(jobs[j], items, begin, item_len, h, k, block, elem_len);
            if (rcs[j] == MK_OK && !one_each && hipStreamSynchronize(g_ctx[jobs[j].dev]->stream) != hipSuccess)
                rcs[j] = fail(MK_EHIP, "hipStreamSynchronize failed on device %d", jobs[j].dev);
            errs[j] = local.err;
            mk::swap_call(nullptr);
        });
    for (auto& t : th) t.join();
    for (size_t j = 0; j < jobs.size(); ++j)
        if (rcs[j] != MK_OK) {
            mk::swap_call(parent);
            return fail(rcs[j], "device %d: %s", jobs[j].dev, errs[j].c_str());
        }
    DevCtx* c0 = g_ctx[devs[0]];
    uint8_t* lvl0 = (uint8_t*)c0->out.p;
    if (one_each) {  // gather the frontier blocks over RCCL (in place: block s of every device)
        std::vector<ncclComm_t>* comms = nullptr;
        TRY(comms_for(devs, comms));
        // (blocks of empty shards are never read: they follow the non-empty ones)
        if (ncclGroupStart() != ncclSuccess) return fail(MK_ECOMM, "ncclGroupStart");
        for (int s = 0; s < nshards; ++s) {
            uint8_t* lvl = (uint8_t*)g_ctx[devs[s]]->out.p;
            if (ncclAllGather(lvl + block * s, lvl, block, ncclUint8, (*comms)[s], g_ctx[devs[s]]->stream) !=
                ncclSuccess) {
                ncclGroupEnd();
                return fail(MK_ECOMM, "ncclAllGather on device %d", devs[s]);
            }
        }
        if (ncclGroupEnd() != ncclSuccess) return fail(MK_ECOMM, "ncclGroupEnd");
    } else {  // several shards per device: copy the other devices' blocks to devs[0]
        TRY(bind_dev(devs[0]));
        for (uint32_t s = 0; s < ne; ++s)  // (blocks of the trailing empty shards are never read)
            if (devs[s] != devs[0])
                HIPCHK(hipMemcpyPeerAsync(lvl0 + block * s, devs[0], (uint8_t*)g_ctx[devs[s]]->out.p + block * s,
                                          devs[s], block, c0->stream));
    }
    TRY(bind_dev(devs[0]));
    const uint64_t last_nodes = k ? mk::frontier_nodes(begin[ne] - begin[ne - 1], item_len, h, k) : 1;
    const uint64_t count = ((uint64_t)(ne - 1) << k) + last_nodes;
    uint8_t* root = lvl0 + block * nshards;
    if (k) {
        TRY(grow(c0->aux, finish_ws_bytes(count)));
        TRY(dev_finish_nodes(lvl0, count, n, root, c0->aux.p, c0->aux.cap, c0->stream));
    } else {
        TRY(dev_finish(lvl0, ne, n, root, c0->stream));
    }
    HIPCHK(hipMemcpyAsync(out, root, 32, hipMemcpyDeviceToHost, c0->stream));
    for (int d : uniq) {
        TRY(bind_dev(d));
        HIPCHK(hipStreamSynchronize(g_ctx[d]->stream));
    }
    return MK_OK;
}

}  // namespace mk::rt

extern "C" {

int mk_ssz_merkle_hash_multi(mk_call* call, const uint8_t* items, uint64_t n, uint32_t item_len, int nshards,
                             const int* devs, uint8_t out[32]) {
    Scope S(call);
    return S.done(host_merkle_multi(items, n, item_len, nshards, devs, out));
}

int mk_dev_ssz_merkle_hash_multi(mk_call* call, const void* const* d_shards, uint64_t n, uint32_t item_len,
                                 int ndev, void* d_out32, void* const* streams) {
    Scope S(call);
    return S.done(dev_merkle_multi(d_shards, n, item_len, ndev, d_out32, streams));
}

}  // extern "C"
