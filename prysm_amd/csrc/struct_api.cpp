// Flat fixed-layout records (hash.go:141-159): struct roots, the registry
// list root in its three forms, the level-1 front, the pipelined stream of
// states, and the mk_*ssz_struct* entry points.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

// ---- struct hashing ---------------------------------------------------------------
// parsing and every check of the layout: struct_spec.cpp (no HIP, no device)
int make_spec(const mk_field* fields, uint32_t nfields, uint32_t record_len, mk::HostSpec& sp) {
    return mk::parse_struct_layout(fields, nfields, record_len, sp);
}

// k_struct_lock's compile-time layout: the SURVEY §8d ValidatorRecord
// (3 bytes fields, 6 uint64, 160-B records); never a layout with the nested kinds
bool validator_layout(const mk::HostSpec& sp) {
    if (sp.nested) return false;
    static const uint32_t off[9] = {0, 48, 80, 112, 120, 128, 136, 144, 152};
    static const uint32_t len[9] = {48, 32, 32, 8, 8, 8, 8, 8, 8};
    if (sp.nfields != 9 || sp.rec_len != 160 || sp.msg_len != 144) return false;
    for (uint32_t f = 0; f < 9; ++f) {
        const bool bytes = f < 3;
        if (sp.kind[f] != (bytes ? MK_FIELD_BYTES : MK_FIELD_RAW) || sp.off[f] != off[f] || sp.len[f] != len[f] ||
            sp.out_off[f] != (bytes ? 32 * f : 96 + 8 * (f - 3)))
            return false;
    }
    return true;
}

// The struct kernels' selectors for n records of layout sp at d_rec
struct StructForm {
    bool fused, vec16, layout, split;
    uint32_t nb, nraw;
};
StructForm struct_form(const void* d_rec, uint64_t n, const mk::HostSpec& sp) {
    StructForm f{};
    f.split = n <= mk::kStructSplitMaxN;
    if (sp.nested) return f;  // MK_FIELD_VARBYTES / _STRUCT: k_struct_nested alone takes them
    // fused path: dword-granular single-block fields, dword-aligned message
    f.fused = sp.msg_len % 4 == 0 && sp.msg_len <= mk::kStructFusedMaxMsg && ((uintptr_t)d_rec % 4) == 0;
    f.vec16 = ((uintptr_t)d_rec % 16) == 0 && sp.rec_len % 16 == 0;
    for (uint32_t k = 0; k < sp.nfields; ++k) {
        if (sp.out_off[k] % 4) f.fused = false;
        if (sp.kind[k] == MK_FIELD_BYTES) {
            if ((sp.len[k] % 4) != 0 || sp.len[k] > mk::kStructFusedMaxField) f.fused = false;
            if (sp.off[k] % 16 || sp.off[k] + ((sp.len[k] + 15) & ~15u) > sp.rec_len) f.vec16 = false;
        } else if (sp.len[k] % 4 || sp.off[k] % 4) {
            f.fused = false;
        }
    }
    // compile-time message layout: NB dword-granular bytes fields (<= 64 B)
    // first, then NRAW 8-byte scalars, at 4-byte aligned record offsets
    while (f.nb < sp.nfields && sp.kind[f.nb] == MK_FIELD_BYTES) ++f.nb;
    f.layout = f.fused && f.nb > 0;
    for (uint32_t k = f.nb; k < sp.nfields; ++k)
        if (sp.kind[k] != MK_FIELD_RAW || sp.len[k] != 8) f.layout = false;
    f.nraw = sp.nfields - f.nb;
    f.split = n <= mk::kStructSplitMaxN;  // latency-bound: 4 lanes per record
    return f;
}

// roots of n records into d_roots (n x 32); d_msg holds n x msg_len bytes
int launch_struct_roots(const void* d_rec, uint64_t n, const mk::HostSpec& sp, void* d_msg, void* d_roots,
                        hipStream_t st) {
    if (n == 0) return MK_OK;
    if (sp.nested) {  // nested structs, variable-length byte fields: one launch, messages in LDS
        if ((uintptr_t)d_rec % 4) return fail(MK_EINVAL, "records of a nested layout must be 4-byte aligned");
        if (sp.rec_len == 0) return fail(MK_EINVAL, "record_len == 0");
        if (sp.lists) {  // list fields: the longer program, down to one wave per workgroup
            const mk::ListSpec& ls = sp.lprog;
            const dim3 grid(ceil_div(n, ls.threads)), block(ls.threads);
            const uint32_t lds = ls.threads * ls.peak;
            if (ls.threads == mk::kListThreadsMax)
                hipLaunchKernelGGL((mk::k_struct_list<128>), grid, block, lds, st, (const uint8_t*)d_rec, n, ls,
                                   (uint4*)d_roots);
            else
                hipLaunchKernelGGL((mk::k_struct_list<64>), grid, block, lds, st, (const uint8_t*)d_rec, n, ls,
                                   (uint4*)d_roots);
            return launched();
        }
        const mk::NestedSpec& ns = sp.prog;
        if (ns.threads == mk::kNestedThreadsMax)
            hipLaunchKernelGGL((mk::k_struct_nested<mk::kNestedThreadsMax>), dim3(ceil_div(n, ns.threads)),
                               dim3(ns.threads), ns.threads * ns.peak, st, (const uint8_t*)d_rec, n, ns,
                               (uint4*)d_roots);
        else
            hipLaunchKernelGGL((mk::k_struct_nested<mk::kNestedThreadsMin>), dim3(ceil_div(n, ns.threads)),
                               dim3(ns.threads), ns.threads * ns.peak, st, (const uint8_t*)d_rec, n, ns,
                               (uint4*)d_roots);
        return launched();
    }
    const StructForm sf = struct_form(d_rec, n, sp);
    const bool fused = sf.fused, vec16 = sf.vec16, layout = sf.layout, split = sf.split;
    const uint32_t nb = sf.nb, nraw = sf.nraw;
    if (layout && split && nb == 3 && nraw == 6) {
        hipLaunchKernelGGL((mk::k_struct_split<3, 6>), dim3(ceil_div(n, 64)), dim3(256), 0, st, (const uint8_t*)d_rec,
                           n, sp, vec16 ? 1u : 0u, (uint4*)d_roots);
        return launched();
    }
    if (layout && split && nb == 2 && nraw == 0) {
        hipLaunchKernelGGL((mk::k_struct_split<2, 0>), dim3(ceil_div(n, 64)), dim3(256), 0, st, (const uint8_t*)d_rec,
                           n, sp, vec16 ? 1u : 0u, (uint4*)d_roots);
        return launched();
    }
    if (layout && nb == 3 && nraw == 6) {
        if (vec16 && validator_layout(sp) && n >= (1u << 18))  // phase-locked, partial last group
            hipLaunchKernelGGL(mk::k_struct_lock<false>,
                               dim3(std::min<uint64_t>(ceil_div(n, mk::kLockThreads), lock_grid_cap(st))),
                               dim3(mk::kLockThreads), 0, st, (const uint8_t*)d_rec, n, (uint4*)d_roots, 0u,
                               (uint4*)nullptr, (const uint8_t*)nullptr, (uint64_t)0, (uint4*)nullptr,
                               mk::StructPrev{});
        else
            hipLaunchKernelGGL((mk::k_struct_reg<3, 6>), dim3(ceil_div(n, mk::kStructThreads)),
                               dim3(mk::kStructThreads), 0, st, (const uint8_t*)d_rec, n, sp, vec16 ? 1u : 0u,
                               (uint4*)d_roots);
        return launched();
    }
    if (layout && nb == 2 && nraw == 0) {
        hipLaunchKernelGGL((mk::k_struct_reg<2, 0>), dim3(ceil_div(n, mk::kStructThreads)), dim3(mk::kStructThreads),
                           0, st, (const uint8_t*)d_rec, n, sp, vec16 ? 1u : 0u, (uint4*)d_roots);
        return launched();
    }
    if (fused) {
        hipLaunchKernelGGL(mk::k_struct_fused, dim3(ceil_div(n, mk::kStructThreads)), dim3(mk::kStructThreads),
                           mk::kStructThreads * sp.msg_len, st, (const uint8_t*)d_rec, n, sp, vec16 ? 1u : 0u,
                           (uint4*)d_roots);
        return launched();
    }
    bool fast = true;  // every bytes field hashes as one dword-granular block
    for (uint32_t f = 0; f < sp.nfields; ++f)
        if (sp.kind[f] == MK_FIELD_BYTES && ((sp.len[f] % 4) != 0 || sp.len[f] + 4 >= 136)) fast = false;
    if (fast)
        hipLaunchKernelGGL((mk::k_struct_fields<true>), dim3(ceil_div(n * sp.nfields, 256)), dim3(256), 0, st,
                           (const uint8_t*)d_rec, n, sp, (uint8_t*)d_msg);
    else
        hipLaunchKernelGGL((mk::k_struct_fields<false>), dim3(ceil_div(n * sp.nfields, 256)), dim3(256), 0, st,
                           (const uint8_t*)d_rec, n, sp, (uint8_t*)d_msg);
    HIPCHK(hipGetLastError());
    if (sp.msg_len % 8 == 0)
        hipLaunchKernelGGL(mk::k_keccak_words, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const uint2*)d_msg, n,
                           sp.msg_len / 8, (uint4*)d_roots);
    else
        hipLaunchKernelGGL(mk::k_keccak_fixed, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const uint8_t*)d_msg, n,
                           sp.msg_len, (uint4*)d_roots);
    return launched();
}

// host-buffer entries: H2D in up to kH2dChunks pieces of at least kH2dMinChunk records
#define MK_H2D_CHUNKS 8
// (smaller floors measured slower: C1's 16,384 records 0.212 ms in one piece,
// 0.280 / 0.421 ms in 4 / 8 pieces; the per-piece copy + event cost outweighs
// the overlap, profiles/r05/h2d_chunk_ab.txt)
#define MK_H2D_MIN_CHUNK 65536
constexpr uint64_t kH2dChunks = MK_H2D_CHUNKS;
constexpr uint64_t kH2dMinChunk = MK_H2D_MIN_CHUNK;

// The registry list root with the merkleHash leaf pass fused into the
// phase-locked struct kernel (k_struct_lock gpw > 0): whole ValidatorRecord
// registries of >= 2^18 records at a 16-B aligned address.  The kernel writes
// the roots and the level-1 windows; the node passes and the length mix-in
// finish from the windows (dev_finish_nodes: the same odd rule at every
// level, hash.go:225-237).  false: not this layout / size (caller takes the
// two-launch path).
bool struct_win_ok(const void* d_rec, uint64_t n, const mk::HostSpec& sp) {
    if (n < (1u << 18)) return false;
    if (((uintptr_t)d_rec % 16) != 0 || sp.rec_len % 16 != 0 || !validator_layout(sp)) return false;
    for (uint32_t f = 0; f < sp.nfields; ++f)
        if (sp.kind[f] == MK_FIELD_BYTES && (sp.off[f] % 16 || sp.off[f] + ((sp.len[f] + 15) & ~15u) > sp.rec_len))
            return false;
    return true;
}

// d_vals (nullable): a second list of vbytes bytes whose level-1 windows the
// kernel hashes on its leftover lanes (item length dividing 128, 16-B aligned)
uint32_t struct_gpw(uint64_t n, hipStream_t st) {  // contiguous groups per workgroup
    return (uint32_t)ceil_div(ceil_div(n, mk::kLockThreads), lock_grid_cap(st));
}
int dev_struct_level1(const void* d_rec, uint64_t n, void* d_roots, void* d_wins, hipStream_t st,
                      const void* d_vals = nullptr, uint64_t vbytes = 0, void* d_vwins = nullptr,
                      const mk::StructPrev* prev = nullptr) {
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    const uint64_t ngroups = ceil_div(n, mk::kLockThreads);
    const uint32_t gpw = struct_gpw(n, st);
    if (prev)
        hipLaunchKernelGGL(mk::k_struct_lock<true>, dim3(ceil_div(ngroups, gpw)), dim3(mk::kLockThreads), 0, st,
                           (const uint8_t*)d_rec, n, (uint4*)d_roots, gpw, (uint4*)d_wins,
                           (const uint8_t*)(vbytes ? d_vals : nullptr), vbytes, (uint4*)d_vwins, *prev);
    else
        hipLaunchKernelGGL(mk::k_struct_lock<false>, dim3(ceil_div(ngroups, gpw)), dim3(mk::kLockThreads), 0, st,
                           (const uint8_t*)d_rec, n, (uint4*)d_roots, gpw, (uint4*)d_wins,
                           (const uint8_t*)(vbytes ? d_vals : nullptr), vbytes, (uint4*)d_vwins, mk::StructPrev{});
    return launched();
}

int dev_struct_list_root_win(const void* d_rec, uint64_t n, void* d_roots, void* d_wins, void* d_out32,
                             void* d_ws, uint64_t ws_bytes, hipStream_t st) {
    TRY(dev_struct_level1(d_rec, n, d_roots, d_wins, st));
    const uint64_t c1 = ceil_div(n, 8);  // windows: ceil(ceil(n / 4) / 2) chunk pairs
    if (ws_bytes < finish_ws_bytes(c1)) return fail(MK_ENOMEM, "workspace too small for the registry top");
    return dev_finish_nodes(d_wins, c1, n, d_out32, d_ws, ws_bytes, st);
}

// A small list of ValidatorRecord-shaped structs (3 bytes fields, 6 8-byte
// scalars: C1) in ONE launch, k_struct_list_fused<3, 6>: the k_struct_split
// records, the latency list tree's windows and levels, and the fused top's
// groups and mix-in, where they were three launches (round 6)
bool struct_list_fused_ok(const void* d_rec, uint64_t n, const mk::HostSpec& sp) {
    const StructForm f = struct_form(d_rec, n, sp);
    return n && f.layout && f.split && f.nb == 3 && f.nraw == 6 && list_tree_ok(n, 32);
}
int launch_struct_list_fused(const void* d_rec, uint64_t n, const mk::HostSpec& sp, uint8_t* d_roots,
                             uint8_t* d_sub, void* d_out32, hipStream_t st) {
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    const StructForm f = struct_form(d_rec, n, sp);
    mk::ReduceArgs a{};  // the window pass over the roots, as dev_list_tree's
    a.cb = 128;
    a.total = 32 * n;
    a.nchunks = ceil_div(a.total, a.cb);
    a.c1 = ceil_div(a.nchunks, 2);
    a.items = d_roots;
    a.n_items = n;
    a.levels = 4;
    const uint64_t nwg = ceil_div(n, 64);  // = the level-4 nodes, ceil(c1 / 8)
    hipLaunchKernelGGL((mk::k_struct_list_fused<3, 6>), dim3((uint32_t)nwg), dim3(1024), 0, st, (const uint8_t*)d_rec,
                       n, sp, f.vec16 ? 1u : 0u, (uint4*)d_roots, a, (uint32_t*)d_sub, (uint32_t*)d_out32,
                       next_arrive_slots(top_arrive_slots(nwg)));
    return launched();
}

uint64_t struct_list_ws(uint64_t n, const mk::HostSpec& sp) {
    Plan p;
    uint64_t mws = 256;
    if (mk::make_plan(n, 32, false, 0, false, true, p) == MK_OK && !p.small) mws = mk::plan_ws_bytes(p);
    mws = std::max(mws, list_tree_ws(n, 32));
    return align256(n * sp.msg_len) + align256(32 * n) + mws;
}

// ---- a stream of states (registry.StatePipeline) ----------------------------
// Workgroup b of the pipelined launch writes the level-1 nodes [sub b, sub b +
// sub) of each tree -- sub = 512 for the registry (4 groups x 1024 records /
// 8), 128 for the second list (the balances) -- a complete subtree whose
// levels 2..K the NEXT launch builds in its slots (k_struct_lock<true>): K =
// 10 for the registry (1 node per subtree), 4 for the second list (16).  A
// levels buffer holds level k (2..K) of subtree b at node offset
// level_off(k) + (sub >> (k - 1)) b, the levels back to back, level K last
// with room after the nfull complete subtrees' nodes for the ragged last
// subtree's (its level-1 nodes reduced on the finisher's stream).
struct PipeTree {
    uint64_t sub;   // level-1 nodes per subtree
    uint32_t K;     // the highest level the slots build
    uint64_t c1;    // level-1 nodes of the whole tree
    uint64_t nfull() const { return c1 / sub; }
    uint64_t per_top() const { return sub >> (K - 1); }
    uint64_t level_off(uint32_t k) const {  // nodes before level k
        uint64_t off = 0;
        for (uint32_t j = 2; j < k; ++j) off += (sub >> (j - 1)) * nfull();
        return off;
    }
    uint64_t levels_bytes() const { return 32 * (level_off(K + 1) + per_top()); }
};
PipeTree pipe_reg(uint64_t n) { return {512, 10, ceil_div(n, 8)}; }
PipeTree pipe_val(uint64_t nvalues, uint32_t value_len) { return {128, 4, ceil_div(nvalues * value_len, 256)}; }
bool struct_pipe_ok(const void* d_rec, uint64_t n, const mk::HostSpec& sp, hipStream_t st) {
    return struct_win_ok(d_rec, n, sp) && struct_gpw(n, st) == 4 && pipe_reg(n).nfull() >= 1;
}

uint64_t pipe_top_ws(const PipeTree& t) {
    mk::WideWaves wide;  // the plans mk_dev_ssz_struct_pipe_top makes
    const uint64_t rag = t.c1 - t.sub * t.nfull();
    uint64_t ws = std::max<uint64_t>(256, finish_ws_bytes(t.nfull() * t.per_top() + t.per_top()));
    Plan p;
    if (rag && mk::make_plan(rag, 32, true, 63 - __builtin_clzll(t.sub), true, true, p, true,
                             63 - __builtin_clzll(t.per_top())) == MK_OK)
        ws = std::max<uint64_t>(ws, mk::plan_ws_bytes(p));
    return ws;
}

int host_struct_roots(const uint8_t* records, uint64_t n, uint32_t record_len, const mk_field* fields,
                      uint32_t nfields, uint8_t* roots) {
    mk::HostSpec sp;
    TRY(make_spec(fields, nfields, record_len, sp));
    if (n && (!records || !roots)) return fail(MK_EINVAL, "null pointer");
    TRY(mk::check_var_lengths(sp, records, n));
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    TRY(grow(c->in, n * (size_t)record_len));
    TRY(grow(c->ws, align256(n * sp.msg_len)));
    TRY(grow(c->out, 32 * n));
    HIPCHK(hipMemcpyAsync(c->in.p, records, n * (size_t)record_len, hipMemcpyHostToDevice, st));
    TRY(launch_struct_roots(c->in.p, n, sp, c->ws.p, c->out.p, st));
    HIPCHK(hipMemcpyAsync(roots, c->out.p, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int host_struct_list_root(const uint8_t* records, uint64_t n, uint32_t record_len, const mk_field* fields,
                          uint32_t nfields, uint8_t* out) {
    mk::HostSpec sp;
    TRY(make_spec(fields, nfields, record_len, sp));
    if (!out || (n && !records)) return fail(MK_EINVAL, "null pointer");
    TRY(mk::check_var_lengths(sp, records, n));
    TRY(bind_call());
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    const uint64_t wsb = struct_list_ws(n, sp);
    TRY(grow(c->in, n * (size_t)record_len));
    TRY(grow(c->ws, wsb));
    TRY(grow(c->out, 32));
    // The records cross PCIe in chunks on the copy stream; the struct-roots
    // kernel of chunk i runs on the compute stream while chunk i+1 is in
    // flight, so only the last chunk's roots and the list merkleHash follow
    // the copy.
    uint8_t* ws = (uint8_t*)c->ws.p;
    uint8_t* msg = ws;
    uint8_t* roots = ws + align256(n * sp.msg_len);
    uint8_t* mws = roots + align256(32 * n);
    const uint8_t* din = (const uint8_t*)c->in.p;
    uint64_t chunk = std::max<uint64_t>(kH2dMinChunk, ceil_div(n, kH2dChunks));
    chunk = (chunk + 15) & ~15ull;  // chunk starts keep the records' 16-B alignment
    if (n <= chunk && struct_list_fused_ok(din, n, sp) && wsb - (uint64_t)(mws - ws) >= list_tree_ws(n, 32)) {
        // one piece: the records cross PCIe, then the whole list in one launch
        HIPCHK(hipMemcpyAsync((uint8_t*)c->in.p, records, n * (size_t)record_len, hipMemcpyHostToDevice, c->copy));
        HIPCHK(hipEventRecord(c->h2d, c->copy));
        HIPCHK(hipStreamWaitEvent(st, c->h2d, 0));
        TRY(launch_struct_list_fused(din, n, sp, roots, mws, c->out.p, st));
        HIPCHK(hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return MK_OK;
    }
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t cnt = std::min(chunk, n - off);
        HIPCHK(hipMemcpyAsync((uint8_t*)c->in.p + off * record_len, records + off * record_len,
                              cnt * (size_t)record_len, hipMemcpyHostToDevice, c->copy));
        HIPCHK(hipEventRecord(c->h2d, c->copy));
        HIPCHK(hipStreamWaitEvent(st, c->h2d, 0));
        TRY(launch_struct_roots(din + off * record_len, cnt, sp, msg + off * sp.msg_len, roots + 32 * off, st));
    }
    TRY(dev_merkle_hash(roots, n, 32, c->out.p, mws, wsb - (uint64_t)(mws - ws), st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

}  // namespace

// what the registry tree (struct_tree_api.cpp) takes from here
namespace mk::rt {
int struct_make_spec(const mk_field* fields, uint32_t nfields, uint32_t record_len, mk::HostSpec& sp) {
    return make_spec(fields, nfields, record_len, sp);
}
bool struct_fused_layout(const mk::HostSpec& sp) { return sp.nested || struct_form(nullptr, 0, sp).fused; }
int struct_launch_roots(const void* d_rec, uint64_t n, const mk::HostSpec& sp, void* d_msg, void* d_roots,
                        hipStream_t st) {
    return launch_struct_roots(d_rec, n, sp, d_msg, d_roots, st);
}
}  // namespace mk::rt

extern "C" {

// ---- struct hashing ---------------------------------------------------------------
uint64_t mk_ssz_struct_msg_len(const mk_field* fields, uint32_t nfields) {
    Scope S(nullptr, false);
    mk::HostSpec sp;
    if (make_spec(fields, nfields, 0, sp) != MK_OK) return 0;
    return sp.msg_len;
}

uint64_t mk_ssz_struct_list_workspace_bytes(uint64_t n, const mk_field* fields, uint32_t nfields) {
    Scope S(nullptr, false);
    mk::HostSpec sp;
    if (make_spec(fields, nfields, 0, sp) != MK_OK) return 0;
    return struct_list_ws(n, sp);
}

int mk_dev_ssz_struct_list_root(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                                const mk_field* fields, uint32_t nfields, void* d_out32, void* d_ws,
                                uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        mk::HostSpec sp;
        TRY(make_spec(fields, nfields, record_len, sp));
        if (ws_bytes < struct_list_ws(n, sp))
            return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes,
                        (unsigned long long)struct_list_ws(n, sp));
        if (n && !d_records) return fail(MK_EINVAL, "null pointer");
        uint8_t* ws = (uint8_t*)d_ws;
        uint8_t* msg = ws;
        uint8_t* roots = ws + align256(n * sp.msg_len);
        uint8_t* mws = roots + align256(32 * n);
        hipStream_t st = (hipStream_t)stream;
        if (struct_win_ok(d_records, n, sp))  // the windows go where the two-launch path keeps its messages
            return dev_struct_list_root_win(d_records, n, roots, msg, d_out32, mws,
                                            ws_bytes - (uint64_t)(mws - ws), st);
        if (struct_list_fused_ok(d_records, n, sp) && ws_bytes - (uint64_t)(mws - ws) >= list_tree_ws(n, 32))
            return launch_struct_list_fused(d_records, n, sp, roots, mws, d_out32, st);
        TRY(launch_struct_roots(d_records, n, sp, msg, roots, st));
        return dev_merkle_hash(roots, n, 32, d_out32, mws, ws_bytes - (uint64_t)(mws - ws), st);
    });
}

int mk_ssz_struct_list_level1_ok(const void* d_records, uint64_t n, uint32_t record_len, const mk_field* fields,
                                 uint32_t nfields) {
    Scope S(nullptr, false);
    mk::HostSpec sp;
    if (make_spec(fields, nfields, record_len, sp) != MK_OK) return 0;
    return struct_win_ok(d_records, n, sp) ? 1 : 0;
}

int mk_dev_ssz_struct_list_level1(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                                  const mk_field* fields, uint32_t nfields, void* d_roots, void* d_nodes,
                                  const void* d_values, uint64_t nvalues, uint32_t value_len, void* d_value_nodes,
                                  void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        mk::HostSpec sp;
        TRY(make_spec(fields, nfields, record_len, sp));
        if (!d_records || !d_roots || !d_nodes) return fail(MK_EINVAL, "null pointer");
        if (!struct_win_ok(d_records, n, sp))
            return fail(MK_EINVAL, "level-1 front needs >= 2^18 ValidatorRecords at a 16-B aligned address");
        if (nvalues) {
            if (!d_values || !d_value_nodes) return fail(MK_EINVAL, "null pointer");
            if (value_len % 8 || value_len == 0 || 128 % value_len || ((uintptr_t)d_values % 16))
                return fail(MK_EINVAL, "second list: items of 8, 16, 32, 64 or 128 B at a 16-B aligned address");
            if (nvalues * value_len <= 128)
                return fail(MK_EINVAL, "second list of one chunk has no level-1 window");
        }
        return dev_struct_level1(d_records, n, d_roots, d_nodes, (hipStream_t)stream, d_values,
                                 nvalues * (uint64_t)value_len, d_value_nodes);
    });
}

int mk_ssz_struct_pipe_ok(const void* d_records, uint64_t n, uint32_t record_len, const mk_field* fields,
                          uint32_t nfields, void* stream) {
    Scope S(nullptr);
    mk::HostSpec sp;
    if (make_spec(fields, nfields, record_len, sp) != MK_OK || bind_stream((hipStream_t)stream)) return S.done(0);
    return S.done(struct_pipe_ok(d_records, n, sp, (hipStream_t)stream) ? 1 : 0);
}

uint64_t mk_ssz_struct_pipe_levels_bytes(uint64_t n, uint64_t nvalues, uint32_t value_len, uint32_t which) {
    if (which > 1 || (which == 1 && (value_len == 0 || nvalues == 0))) return 0;
    return which ? pipe_val(nvalues, value_len).levels_bytes() : pipe_reg(n).levels_bytes();
}

uint64_t mk_ssz_struct_pipe_top_workspace_bytes(uint64_t n, uint64_t nvalues, uint32_t value_len, uint32_t which) {
    Scope S(nullptr, false);
    if (which > 1 || (which == 1 && (value_len == 0 || nvalues == 0))) return 0;
    return pipe_top_ws(which ? pipe_val(nvalues, value_len) : pipe_reg(n));
}

int mk_dev_ssz_struct_list_level1_pipe(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                                       const mk_field* fields, uint32_t nfields, void* d_roots, void* d_nodes,
                                       const void* d_values, uint64_t nvalues, uint32_t value_len,
                                       void* d_value_nodes, const void* d_prev_nodes, void* d_prev_levels,
                                       const void* d_prev_value_nodes, void* d_prev_value_levels, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        mk::HostSpec sp;
        TRY(make_spec(fields, nfields, record_len, sp));
        if (!d_records || !d_roots || !d_nodes || (d_prev_nodes && !d_prev_levels) ||
            (d_prev_value_nodes && !d_prev_value_levels))
            return fail(MK_EINVAL, "null pointer");
        if (!struct_pipe_ok(d_records, n, sp, (hipStream_t)stream))
            return fail(MK_EINVAL, "pipelined struct launch needs ValidatorRecords at a 16-B aligned address, "
                                          "4 groups of 1024 per workgroup (n = %llu)", (unsigned long long)n);
        if (d_prev_nodes && d_prev_nodes == d_nodes)
            return fail(MK_EINVAL, "the previous state's nodes alias this state's");
        const uint64_t grid = ceil_div(ceil_div(n, mk::kLockThreads), 4);
        if (nvalues) {
            if (!d_values || !d_value_nodes) return fail(MK_EINVAL, "null pointer");
            if (value_len % 8 || value_len == 0 || 128 % value_len || ((uintptr_t)d_values % 16))
                return fail(MK_EINVAL, "second list: items of 8, 16, 32, 64 or 128 B at a 16-B aligned address");
            if (nvalues * value_len <= 128)
                return fail(MK_EINVAL, "second list of one chunk has no level-1 window");
            if (pipe_val(nvalues, value_len).c1 > 128 * grid)
                return fail(MK_EINVAL, "second list longer than 128 windows per workgroup");
            if (d_prev_value_nodes && d_prev_value_nodes == d_value_nodes)
                return fail(MK_EINVAL, "the previous state's second-list nodes alias this state's");
        } else if (d_prev_value_nodes) {
            return fail(MK_EINVAL, "previous second list without this state's");
        }
        const PipeTree reg = pipe_reg(n), val = pipe_val(nvalues, value_len);
        mk::StructPrev prev{};
        prev.nfull = (uint32_t)reg.nfull();
        prev.live = d_prev_nodes ? 1u : 0u;
        prev.l1 = (const uint4*)d_prev_nodes;
        for (uint32_t k = 2; k <= 10; ++k)
            prev.lv[k - 2] = d_prev_levels ? (uint4*)d_prev_levels + 2 * reg.level_off(k) : nullptr;
        // the second list's slots (waves 13-15) only with a previous second list
        prev.nvfull = d_prev_value_nodes ? (uint32_t)val.nfull() : 0u;
        prev.v1 = (const uint4*)d_prev_value_nodes;
        for (uint32_t k = 2; k <= 4; ++k)
            prev.vlv[k - 2] = d_prev_value_levels ? (uint4*)d_prev_value_levels + 2 * val.level_off(k) : nullptr;
        return dev_struct_level1(d_records, n, d_roots, d_nodes, (hipStream_t)stream, d_values,
                                 nvalues * (uint64_t)value_len, d_value_nodes, &prev);
    });
}

int mk_dev_ssz_struct_pipe_top(mk_call* call, const void* d_nodes, uint64_t n, uint64_t nvalues,
                               uint32_t value_len, uint32_t which, void* d_levels, void* d_pair_block, uint32_t slot,
                               uint32_t epoch, void* d_ws, uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (!d_nodes || !d_levels || !d_pair_block) return fail(MK_EINVAL, "null pointer");
        if (which > 1 || (which == 1 && (value_len == 0 || nvalues == 0)))
            return fail(MK_EINVAL, "tree %u: 0 = the registry, 1 = a non-empty second list", which);
        if (slot > 1) return fail(MK_EINVAL, "pair slot %u out of range (0..1)", slot);
        if (epoch == 0 || epoch >= (1u << 30)) return fail(MK_EINVAL, "pair epoch %u out of range (1..2^30-1)", epoch);
        if ((uintptr_t)d_pair_block % 16) return fail(MK_EINVAL, "pair block not 16-B aligned");
        const PipeTree t = which ? pipe_val(nvalues, value_len) : pipe_reg(n);
        const uint64_t nfull = t.nfull(), rag = t.c1 - t.sub * nfull;
        if (nfull == 0) return fail(MK_EINVAL, "no complete subtree");
        mk::WideWaves wide;  // beside the next pipelined launch: whole-CU workgroups only
        if (ws_bytes < pipe_top_ws(t)) return fail(MK_ENOMEM, "workspace too small");
        uint8_t* top = (uint8_t*)d_levels + 32 * t.level_off(t.K);  // level K: per_top nodes per subtree
        uint64_t count = nfull * t.per_top();
        if (rag) {  // the ragged last subtree from level 1 to level K, the odd rule at every level (pad_at_one)
            Plan p;
            const uint32_t h = 63 - __builtin_clzll(t.sub), f = 63 - __builtin_clzll(t.per_top());
            TRY(mk::make_plan(rag, 32, true, h, true, ((uintptr_t)d_nodes % 16) == 0, p, true, f));
            TRY(launch_plan(p, (const uint8_t*)d_nodes + 32 * t.sub * nfull, top + 32 * count, (uint8_t*)d_ws,
                            ws_bytes, (hipStream_t)stream));
            count += f ? p.out_nodes : 1;
        }
        return dev_finish_nodes(top, count, which ? nvalues : n, nullptr, d_ws, ws_bytes, (hipStream_t)stream,
                                d_pair_block, slot, epoch);
    });
}

int mk_dev_ssz_struct_roots(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                            const mk_field* fields, uint32_t nfields, void* d_roots, void* d_ws, uint64_t ws_bytes,
                            void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        mk::HostSpec sp;
        TRY(make_spec(fields, nfields, record_len, sp));
        if (n && (!d_records || !d_roots)) return fail(MK_EINVAL, "null pointer");
        if (ws_bytes < n * (uint64_t)sp.msg_len)
            return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes,
                        (unsigned long long)(n * (uint64_t)sp.msg_len));
        return launch_struct_roots(d_records, n, sp, d_ws, d_roots, (hipStream_t)stream);
    });
}

int mk_ssz_struct_roots(mk_call* call, const uint8_t* records, uint64_t n, uint32_t record_len,
                        const mk_field* fields, uint32_t nfields, uint8_t* roots) {
    Scope S(call);
    return S.done(host_struct_roots(records, n, record_len, fields, nfields, roots));
}

int mk_ssz_struct_list_root(mk_call* call, const uint8_t* records, uint64_t n, uint32_t record_len,
                            const mk_field* fields, uint32_t nfields, uint8_t out[32]) {
    Scope S(call);
    return S.done(host_struct_list_root(records, n, record_len, fields, nfields, out));
}

}  // extern "C"
