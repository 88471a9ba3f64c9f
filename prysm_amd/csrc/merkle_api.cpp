// merkleHash on the device: the launch side of the pass planner (planner.cpp),
// the latency list tree, the fused tops and their arrival slots, element
// digests, many lists, and the mk_*ssz_merkle* / tree_hash entry points.
#include <atomic>

#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

// ---- merkleHash plan launch --------------------------------------------------------
template <bool LEAF>
void launch_wave3(uint32_t nt, uint64_t nwg, const ReduceArgs& a, hipStream_t st) {
    switch (nt) {
        case 64: hipLaunchKernelGGL((mk::k_wave3<64, LEAF>), dim3(nwg), dim3(64), 0, st, a); break;
        case 128: hipLaunchKernelGGL((mk::k_wave3<128, LEAF>), dim3(nwg), dim3(128), 0, st, a); break;
        case 256: hipLaunchKernelGGL((mk::k_wave3<256, LEAF>), dim3(nwg), dim3(256), 0, st, a); break;
        case 512: hipLaunchKernelGGL((mk::k_wave3<512, LEAF>), dim3(nwg), dim3(512), 0, st, a); break;
        default: hipLaunchKernelGGL((mk::k_wave3<1024, LEAF>), dim3(nwg), dim3(1024), 0, st, a); break;
    }
}

// ---- fused list tops (k_merkle_top_fused) -------------------------------------------
// Workgroups of NT = 1024 threads (one per CU).  Per list: nodes per
// workgroup = the power of two that gives the list about 256 / nlists
// workgroups, so the throughput-bound lower levels spread over the chip (two
// lists side by side in one grid), 64..1024; a list of <= 1024 nodes runs in
// one workgroup (no hand-off).  C3 (125,000 + 31,250 nodes): 123 + 123
// workgroups.  (512-thread workgroups, two per CU, 245 + 245 of them:
// C3 one state 0.5748 / 0.5819 against 0.5712 / 0.5719 ms, rejected.)
struct TopPlan {
    static constexpr uint32_t nt = 1024;
    uint32_t span_log2[2] = {0, 0}, nwg[2] = {0, 0};
    uint64_t ws = 0;
};
int top_plan(const uint64_t* c, uint32_t nl, TopPlan& p) {
    p = TopPlan();
    for (uint32_t l = 0; l < nl; ++l) {
        if (c[l] == 0) return fail(MK_EINVAL, "empty level");
        if (c[l] > (1ull << 20)) return fail(MK_EINVAL, "fused top: %llu nodes > 2^20", (unsigned long long)c[l]);
    }
    const uint32_t lmax = 10;
    const uint64_t target = 256 / nl;
    for (uint32_t l = 0; l < nl; ++l) {
        uint32_t sl = lmax;
        if (c[l] > p.nt) {
            sl = 6;
            while (sl < lmax && (c[l] >> sl) >= target) ++sl;
        }
        p.span_log2[l] = sl;
        p.nwg[l] = (uint32_t)ceil_div(c[l], 1ull << sl);
        p.ws += 32 * (uint64_t)p.nwg[l];
    }
    p.ws = (p.ws + 255) & ~255ull;
    return MK_OK;
}

int launch_top_fused(const TopPlan& p, uint32_t nl, const void* const* nodes, const uint64_t* c,
                     const uint64_t* nit, void* d_out, uint32_t epoch, void* d_ws, hipStream_t st) {
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    mk::MerkleTopArgs a{};
    a.nlists = nl;
    a.pair = nl == 2 ? (uint32_t*)d_out : nullptr;
    a.pair_slot = nl == 2 ? next_arrive_slots(1) : 0;
    (void)epoch;  // both finishers are in this launch: an arrival counter, not the epoch word
    uint32_t wg = 0;
    uint32_t* sub = (uint32_t*)d_ws;
    for (uint32_t l = 0; l < nl; ++l) {
        mk::MerkleTopList& t = a.l[l];
        t.nodes = (const uint4*)nodes[l];
        t.c = c[l];
        t.n_items = nit[l];
        t.sub = sub;
        t.out = nl == 2 ? (uint32_t*)d_out + 8 * l : (uint32_t*)d_out;
        t.wg0 = wg;
        t.nwg = p.nwg[l];
        t.span_log2 = p.span_log2[l];
        t.slot = next_arrive_slots(top_arrive_slots(t.nwg));
        wg += t.nwg;
        sub += 8 * t.nwg;
    }
    hipLaunchKernelGGL(mk::k_merkle_top_fused<1024>, dim3(wg), dim3(1024), 0, st, a);
    return launched();
}

// k_merkle_top_fused over one list's complete level of c nodes in spans of
// 2^span_log2 nodes per workgroup, to the root with the length mix-in
int launch_top_span(const void* d_nodes, uint64_t c, uint64_t n_items, uint32_t span_log2, void* d_out32,
                    uint8_t* d_ws, hipStream_t st) {
    TopPlan p;
    p.span_log2[0] = span_log2;
    p.nwg[0] = (uint32_t)ceil_div(c, 1ull << span_log2);
    p.ws = align256(32 * (uint64_t)p.nwg[0]);
    const void* nodes[1] = {d_nodes};
    const uint64_t cc[1] = {c}, nit[1] = {n_items};
    return launch_top_fused(p, 1, nodes, cc, nit, d_out32, 0, d_ws, st);
}

// ---- the latency list tree ------------------------------------------------------------
// The latency form of a small list's tree (round 6): merkleHash of n items
// whose first level has 16 < windows <= 2^12 (C1's 16,384 ValidatorRecord
// roots: 2,048 windows).  k_spread_leaf<8> hashes the windows one per wave, 8
// per workgroup (two waves per SIMD, where the general plan's 16 put four on
// each: 2 x ~9.8 k cycles against 2 x ~17.8 k -- a lone wave is issue-bound,
// DESIGN §4.5), and folds each workgroup's 8 to one node 3 levels up;
// k_merkle_top_fused takes those nodes 16 per workgroup (4 levels in the
// spread form), groups of 16 workgroups, and the last to the root and the
// length mix-in -- where the general plan ran one 1024-thread k_wave3 over
// the last <= 256 nodes, whose widest levels run as lane pairs at ~14 k
// cycles each.  C1 0.095 -> 0.085 ms (profiles/r06/c1/).
int dev_list_tree(const void* d_items, uint64_t n, uint32_t item_len, void* d_out32, uint8_t* ws,
                  hipStream_t st) {
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    mk::ReduceArgs a{};
    a.cb = mk::chunk_bytes(item_len);
    a.total = n * (uint64_t)item_len;
    a.nchunks = ceil_div(a.total, a.cb);
    a.c1 = ceil_div(a.nchunks, 2);
    a.items = (const uint8_t*)d_items;
    a.out = ws;
    a.n_items = n;
    a.levels = 4;  // the windows + 3 levels: one node per workgroup
    const uint32_t w8 = (((uintptr_t)d_items % 8) == 0 && a.cb % 8 == 0) ? 1u : 0u;
    hipLaunchKernelGGL(mk::k_spread_leaf<8>, dim3(ceil_div(a.c1, 8)), dim3(1024), 0, st, a, w8);
    HIPCHK(hipGetLastError());
    const uint64_t c4 = ceil_div(a.c1, 8);
    return launch_top_span(ws, c4, n, 4, d_out32, ws + align256(32 * c4), st);
}

// ---- TreeHash of a list of byte strings (makeSliceHasher + hashedEncoding) ---------------
// The tree's items are the n element digests K(le32(elem_len) || element)
// (hash.go:100-107, 118-139).  Fused (k_reduce_elem, no digest array) when
// the elements are 32 B, 16-B aligned and the leaf pass is a throughput
// pass; otherwise the digests go to the workspace first (k_elem_digests) and
// the ordinary plan runs over them.
struct ElemPlan {
    Plan p;
    bool fused = false;
    uint64_t dig_bytes = 0;  // two-phase: digest array at the start of the workspace
    uint64_t ws_bytes = 0;
    bool locked = false;  // k_elem_lock writes the window digests, `p` reduces them (node input, mix-in n)
    uint64_t nwin = 0;
};

#define MK_ELEM_LOCK_MIN_LOG2 23  // elements (2^20 windows: 1024 groups)

int make_elem_plan(uint64_t n, uint32_t elem_len, bool aligned16, ElemPlan& e) {
    e = ElemPlan();
    if (n > (UINT64_MAX / 4) / 32) return fail(MK_EINVAL, "n too large");
    const bool fast32 = elem_len == 32 && aligned16;
    if (fast32 && n % 8 == 0 && n >= (1ull << MK_ELEM_LOCK_MIN_LOG2)) {
        // phase-locked element windows (every window full: 8 elements = 2
        // chunks), then the tree above them from its level-1 nodes
        e.locked = true;
        e.nwin = n / 8;
        TRY(mk::make_plan(e.nwin, 32, false, 0, false, true, e.p, /*node_input=*/true, 0, /*mixin_n=*/n));
        e.dig_bytes = (32 * e.nwin + 255) & ~255ull;
        e.ws_bytes = e.dig_bytes + mk::plan_ws_bytes(e.p);
        return MK_OK;
    }
    TRY(mk::make_plan(n, 32, false, 0, false, fast32, e.p, false, 0, 0, /*leaf_ni1=*/fast32));
    e.fused = fast32 && !e.p.small && !e.p.passes.empty() && !e.p.passes[0].wave && !e.p.passes[0].sp;
    if (!e.fused && fast32) TRY(mk::make_plan(n, 32, false, 0, false, true, e.p));  // the ordinary plan over digests
    if (e.fused) {
        Pass& ps = e.p.passes[0];
        ps.a.elem_len = 32;
        ps.perms += (double)n;  // one permutation per 36-B element message
        ps.hashes += (double)n;
        e.ws_bytes = mk::plan_ws_bytes(e.p);
    } else {
        e.dig_bytes = (32 * n + 255) & ~255ull;
        e.ws_bytes = e.dig_bytes + (e.p.small ? 256 : mk::plan_ws_bytes(e.p));
    }
    return MK_OK;
}

int dev_tree_hash_elems(const void* d_elems, uint64_t n, uint32_t elem_len, void* d_out32, void* d_ws,
                        uint64_t ws_bytes, hipStream_t st) {
    if (!d_out32 || (n && elem_len && !d_elems)) return fail(MK_EINVAL, "null pointer");
    ElemPlan e;
    const bool aligned16 = ((uintptr_t)d_elems % 16) == 0;
    TRY(make_elem_plan(n, elem_len, aligned16, e));
    uint64_t need = e.ws_bytes;
    if (!aligned16) {  // the documented two-phase size: the query's plus the digest array
        ElemPlan q;
        TRY(make_elem_plan(n, elem_len, true, q));
        need = std::max<uint64_t>(need, q.ws_bytes + align256(32 * n));
    }
    if (ws_bytes < need)
        return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes,
                    (unsigned long long)need);
    if (n && !d_ws) return fail(MK_EINVAL, "null workspace");
    if (e.fused) return launch_plan(e.p, (const uint8_t*)d_elems, (uint8_t*)d_out32, (uint8_t*)d_ws, ws_bytes, st);
    uint8_t* dig = (uint8_t*)d_ws;
    ProfRec rec{};
    const bool prof = prof_on();
    if (e.locked) {
        if (prof) TRY(prof_begin(rec, st));
        hipLaunchKernelGGL(mk::k_elem_lock, dim3(std::min<uint64_t>(ceil_div(e.nwin, mk::kLockThreads), lock_grid_cap(st))),
                           dim3(mk::kLockThreads), 0, st, (const uint4*)d_elems, e.nwin, (uint4*)dig);
        HIPCHK(hipGetLastError());
        // 8 element digests + the 2-block window
        if (prof) TRY(prof_end(rec, 10.0 * (double)e.nwin, 9.0 * (double)e.nwin, st));
    } else if (n) {
        if (prof) TRY(prof_begin(rec, st));
        TRY(launch_elem_digests(d_elems, n, elem_len, dig, st));
        if (prof) TRY(prof_end(rec, (double)n * (double)mk::perms_for_len((uint64_t)elem_len + 4), (double)n, st));
    }
    return launch_plan(e.p, dig, (uint8_t*)d_out32, dig + e.dig_bytes, ws_bytes - e.dig_bytes, st);
}

// merkleHash of a host buffer (the cgo TreeHash path).  A large buffer goes
// through the sharded path with its shards on this one device: shard i+1
// crosses PCIe while shard i's passes run, so the compute hides under the
// copy (8 GiB: copy then compute 162-164 ms) and the device holds
// two shard regions instead of the whole input.
#define MK_HOST_OVERLAP_MIN_LOG2 28  // bytes; 64 = never
int host_merkle_hash(const uint8_t* items, uint64_t n, uint32_t item_len, uint8_t* out) {
    if (!out || (n && item_len && !items)) return fail(MK_EINVAL, "null pointer");
    const uint64_t inb = n * (uint64_t)item_len;
    if (MK_HOST_OVERLAP_MIN_LOG2 < 64 && item_len && n <= (UINT64_MAX / 2) / item_len &&
        inb >= (1ull << (MK_HOST_OVERLAP_MIN_LOG2 & 63))) {
        TRY(bind_call());
        const int d = t_bound;
        const int ns = (int)std::min<uint64_t>(8, std::max<uint64_t>(2, inb >> 26));  // >= 64 MB per shard
        std::vector<int> devs(ns, d);
        return host_merkle_multi(items, n, item_len, ns, devs.data(), out);
    }
    return host_merkle_hash_plain(items, n, item_len, out);
}

// TreeHash of a host list of byte strings (the cgo path): like
// host_merkle_hash, a buffer of at least 2^MK_HOST_OVERLAP_MIN_LOG2 bytes goes
// through the sharded path on its one device, so shard i+1's elements cross
// PCIe while shard i is hashed (element digests, then the digest subtree).
int host_tree_hash_elems(const uint8_t* elems, uint64_t n, uint32_t elem_len, uint8_t* out) {
    if (!out || (n && elem_len && !elems)) return fail(MK_EINVAL, "null pointer");
    if (elem_len && n > (UINT64_MAX / 4) / elem_len) return fail(MK_EINVAL, "n * elem_len overflows");
    const uint64_t inb = n * (uint64_t)elem_len;
    if (MK_HOST_OVERLAP_MIN_LOG2 < 64 && elem_len && inb >= (1ull << (MK_HOST_OVERLAP_MIN_LOG2 & 63))) {
        TRY(bind_call());
        const int d = t_bound;
        const int ns = (int)std::min<uint64_t>(8, std::max<uint64_t>(2, inb >> 26));  // >= 64 MB per shard
        std::vector<int> devs(ns, d);
        return host_merkle_multi(elems, n, 32, ns, devs.data(), out, elem_len);
    }
    return host_tree_hash_elems_plain(elems, n, elem_len, out);
}

// ---- many lists ------------------------------------------------------------------------
int dev_merkle_many(const void* d_items, const mk::ManyPlan& mp, uint32_t nlists, void* d_roots, void* d_ws,
                    uint64_t ws_bytes, hipStream_t st) {
    if (ws_bytes < mp.ws_bytes)
        return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes,
                    (unsigned long long)mp.ws_bytes);
    if (nlists == 0) return MK_OK;
    if (!d_roots || !d_ws) return fail(MK_EINVAL, "null pointer");
    // the per-list descriptors are planned on the host and uploaded through
    // the pinned ring: a captured copy node would replay whatever a later
    // call left in that slot, so this entry point refuses stream capture
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(MK_EINVAL, "mk_dev_ssz_merkle_many cannot be captured into a graph (host-planned descriptors)");
    uint8_t* ws = (uint8_t*)d_ws;
    auto* lists = (mk::ManyList*)(ws + mp.off_lists);
    auto* act = (mk::ManyAct*)(ws + mp.off_act);
    uint4* buf[2] = {(uint4*)(ws + mp.off_buf0), (uint4*)(ws + mp.off_buf1)};
    uint4* tops = (uint4*)(ws + mp.off_tops);
    DevCtx* c = ctx();
    TRY(upload_small(c, lists, mp.lists.data(), sizeof(mk::ManyList) * nlists, st));
    TRY(upload_small(c, act, mp.act.data(), sizeof(mk::ManyAct) * mp.act.size(), st));
    const uint8_t* items = (const uint8_t*)d_items;
    for (uint32_t l = 0; l < mp.nlevels; ++l) {  // level l+1 into buffer l % 2
        const uint64_t nodes = mp.lvl_nodes[l];
        const uint32_t nact = (uint32_t)(mp.lvl_begin[l + 1] - mp.lvl_begin[l]);
        if (!nodes) continue;
        const mk::ManyAct* a = act + mp.lvl_begin[l];
        if (l == 0)
            hipLaunchKernelGGL((mk::k_many_level<true>), dim3(ceil_div(nodes, 256)), dim3(256), 0, st, items, lists, a,
                               nact, nodes, (const uint4*)nullptr, buf[0], tops);
        else
            hipLaunchKernelGGL((mk::k_many_level<false>), dim3(ceil_div(nodes, 256)), dim3(256), 0, st, items, lists,
                               a, nact, nodes, (const uint4*)buf[(l - 1) % 2], buf[l % 2], tops);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mk::k_many_final, dim3(ceil_div(nlists, 256)), dim3(256), 0, st, items, lists, nlists,
                       (const uint4*)tops, (uint4*)d_roots);
    HIPCHK(hipGetLastError());
    for (size_t b = 0; b < mp.big.size(); ++b) {  // big lists: their own fused plans, one shared workspace
        const mk::ManyList& L = mp.lists[mp.big[b]];
        TRY(launch_plan(mp.big_plans[b], items + L.items_off, (uint8_t*)d_roots + 32 * (uint64_t)mp.big[b],
                        ws + mp.off_big, ws_bytes - mp.off_big, st));
    }
    return MK_OK;
}

int host_merkle_many(const uint8_t* items, const uint64_t* offs, const uint64_t* n, const uint32_t* item_len,
                     uint32_t nlists, uint8_t* roots) {
    if (nlists == 0) return MK_OK;
    if (!offs || !n || !item_len || !roots) return fail(MK_EINVAL, "null pointer");
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint32_t i = 0; i < nlists; ++i) {
        const uint64_t b = n[i] * (uint64_t)item_len[i];
        if (b) {
            lo = std::min(lo, offs[i]);
            hi = std::max(hi, offs[i] + b);
        }
    }
    if (lo == UINT64_MAX) lo = hi = 0;
    if (hi > lo && !items) return fail(MK_EINVAL, "null items");
    // upload [lo, hi) of the caller's buffer; offsets shift by lo (rounded down to 16 keeps alignment)
    lo &= ~15ull;
    std::vector<uint64_t> rel(offs, offs + nlists);
    for (uint32_t i = 0; i < nlists; ++i) rel[i] = n[i] * (uint64_t)item_len[i] ? offs[i] - lo : 0;
    mk::ManyPlan mp;
    // the device copy starts 256-B aligned: a list is 16-B aligned there iff its offset is
    TRY(mk::make_many_plan(rel.data(), n, item_len, nlists, hi - lo, true, mp));
    TRY(bind_call());
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    TRY(grow(c->in, hi - lo));
    TRY(grow(c->ws, mp.ws_bytes));
    TRY(grow(c->out, 32 * (size_t)nlists));
    if (hi > lo) HIPCHK(hipMemcpyAsync(c->in.p, items + lo, hi - lo, hipMemcpyHostToDevice, st));
    TRY(dev_merkle_many(c->in.p, mp, nlists, c->out.p, c->ws.p, c->ws.cap, st));
    HIPCHK(hipMemcpyAsync(roots, c->out.p, 32 * (size_t)nlists, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int launch_plan(const Plan& p, const uint8_t* d_items, uint8_t* d_out32, uint8_t* d_ws, uint64_t ws_bytes,
                hipStream_t st, uint8_t* pair_block, uint32_t pair_slot, uint32_t pair_epoch) {
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    if (p.small && pair_block) return fail(MK_EINVAL, "internal: pair finalize needs a k_wave3 plan");
    if (p.small) {
        hipLaunchKernelGGL(mk::k_final_small, dim3(1), dim3(64), 0, st, d_items, p.total, p.n, d_out32);
        return launched();
    }
    if (ws_bytes < mk::plan_ws_bytes(p))
        return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes,
                    (unsigned long long)mk::plan_ws_bytes(p));
    if (pair_block)  // checked before any pass is launched
        for (const Pass& ps : p.passes)
            if (ps.a.finalize && (!ps.wave || !ps.w3))
                return fail(MK_EINVAL, "internal: pair finalize needs the spread-form k_wave3 final pass");
    uint8_t* slots[2] = {d_ws, d_ws + 32 * p.slot_nodes[0]};
    const bool prof = prof_on();
    for (const Pass& ps : p.passes) {
        ReduceArgs a = ps.a;
        a.items = ps.in_ws < 0 ? d_items : slots[ps.in_ws];
        a.out = ps.out_ws < 0 ? d_out32 : slots[ps.out_ws];
        if (a.finalize && pair_block) {  // a two-field struct root (wave3_spread_final)
            a.pair_block = pair_block;
            a.pair_slot = pair_slot;
            a.pair_epoch = pair_epoch;
            a.out = pair_block + 32 * pair_slot;
        }
        ProfRec rec{};
        const bool rec_this = prof && ps.leaf;
        if (rec_this) TRY(prof_begin(rec, st));
        if (ps.sp) {
            a.wg_base = 0;
            const uint32_t w8 = (((uintptr_t)a.items % 8) == 0 && a.cb % 8 == 0) ? 1u : 0u;
            hipLaunchKernelGGL(mk::k_spread_leaf<16>, dim3(ps.nwg), dim3(1024), 0, st, a, w8);
            HIPCHK(hipGetLastError());
        } else if (ps.wave) {
            a.wg_base = 0;
            if (ps.leaf)
                launch_wave3<true>(ps.nt, ps.nwg, a, st);
            else
                launch_wave3<false>(ps.nt, ps.nwg, a, st);
            HIPCHK(hipGetLastError());
        } else {
            // The ragged workgroup(s) of a pass are latency-bound; when the pass
            // also has full workgroups they go first, on the side stream, so
            // they overlap the full ones (fork/join through events on `st`).
            const bool ragged = ps.nwg > ps.nfast;
            DevCtx* c = (ragged && ps.nfast) ? ctx() : nullptr;
            std::unique_lock<std::mutex> lk;
            if (ragged) {
                hipStream_t gs = st;
                if (c) {
                    lk = std::unique_lock<std::mutex>(c->side_mu);
                    HIPCHK(hipEventRecord(c->fork, st));
                    HIPCHK(hipStreamWaitEvent(c->side, c->fork, 0));
                    gs = c->side;
                }
                ReduceArgs g = a;
                g.wg_base = ps.nfast;
                if (ps.leaf && a.elem_len)  // planned with NI = 1
                    hipLaunchKernelGGL((mk::k_reduce_elem<false>), dim3(ps.nwg - ps.nfast), dim3(kReduceThreads), 0,
                                       gs, g);
                else if (ps.leaf && ps.ni == 1)
                    hipLaunchKernelGGL((mk::k_reduce<true, false, 1>), dim3(ps.nwg - ps.nfast), dim3(kReduceThreads),
                                       0, gs, g);
                else if (ps.leaf)
                    hipLaunchKernelGGL((mk::k_reduce<true, false, 2>), dim3(ps.nwg - ps.nfast), dim3(kReduceThreads),
                                       0, gs, g);
                else
                    hipLaunchKernelGGL((mk::k_reduce<false, false, 2>), dim3(ps.nwg - ps.nfast), dim3(kReduceThreads),
                                       0, gs, g);
                HIPCHK(hipGetLastError());
                if (c) HIPCHK(hipEventRecord(c->join, c->side));
            }
            uint64_t fast_base = 0;
            if (ps.nlock && ps.leaf && !a.elem_len) {  // phase-locked leaf workgroups first: 4 spans each, levels == 3
                a.wg_base = 0;
                // persistent grid (one 1024-thread workgroup per CU), whole trees and subtree shards
                // alike: a shard's pipelined step beside its side-stream passes measured 1.2-3.7 %
                // faster than one group per workgroup (profiles/r05/shard_persist/)
                hipLaunchKernelGGL(mk::k_leaf_lock_sc, dim3(std::min<uint64_t>(ps.nlock, lock_grid_cap(st))),
                                   dim3(mk::kLockThreads), 0, st, a, ps.nlock);
                HIPCHK(hipGetLastError());
                fast_base = ps.nlock * 4;
            } else if (ps.nlock && !ps.leaf) {  // phase-locked node groups first: 16 spans each, levels == 5
                a.wg_base = 0;
                hipLaunchKernelGGL(mk::k_node_lock, dim3(std::min<uint64_t>(ps.nlock, lock_grid_cap(st))),
                                   dim3(mk::kLockThreads), 0, st, a, ps.nlock);
                HIPCHK(hipGetLastError());
                fast_base = ps.nlock * mk::kNodeLockSpans;
            }
            if (ps.nfast > fast_base) {
                a.wg_base = fast_base;
                const uint64_t nfast = ps.nfast - fast_base;
                if (ps.leaf && a.elem_len)
                    hipLaunchKernelGGL((mk::k_reduce_elem<true>), dim3(nfast), dim3(kReduceThreads), 0, st, a);
                else if (ps.leaf && ps.ni == 1)
                    hipLaunchKernelGGL((mk::k_reduce<true, true, 1>), dim3(nfast), dim3(kReduceThreads), 0, st, a);
                else if (ps.leaf)
                    hipLaunchKernelGGL((mk::k_reduce<true, true, 2>), dim3(nfast), dim3(kReduceThreads), 0, st, a);
                else
                    hipLaunchKernelGGL((mk::k_reduce<false, true, 2>), dim3(nfast), dim3(kReduceThreads), 0, st, a);
                HIPCHK(hipGetLastError());
            }
            if (c) HIPCHK(hipStreamWaitEvent(st, c->join, 0));
        }
        if (rec_this) TRY(prof_end(rec, ps.perms, ps.hashes, st));
    }
    return MK_OK;
}

bool list_tree_ok(uint64_t n, uint32_t item_len) { return mk::list_tree_fits(n, item_len); }
uint64_t list_tree_ws(uint64_t n, uint32_t item_len) { return mk::list_tree_ws_bytes(n, item_len); }

int ws_too_small(uint64_t ws_bytes, uint64_t need) {
    return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes, (unsigned long long)need);
}

// The workspace contract is the query's size whatever the pointers' alignment:
// a workspace below mk_ssz_merkle_workspace_bytes is refused before any launch,
// also where this call's own plan (the list tree's shapes through the planner,
// items that are not 16-B aligned) would have fitted into less.
int dev_merkle_hash(const void* d_items, uint64_t n, uint32_t item_len, void* d_out32, void* d_ws, uint64_t ws_bytes,
                    hipStream_t st) {
    if (!d_out32 || (n && item_len && !d_items)) return fail(MK_EINVAL, "null pointer");
    const bool aligned16 = ((uintptr_t)d_items % 16) == 0;
    if (list_tree_ok(n, item_len)) {
        if (ws_bytes < list_tree_ws(n, item_len)) return ws_too_small(ws_bytes, list_tree_ws(n, item_len));
        if ((uintptr_t)d_ws % 16 == 0) return dev_list_tree(d_items, n, item_len, d_out32, (uint8_t*)d_ws, st);
    }
    Plan p;
    TRY(mk::make_plan(n, item_len, false, 0, false, aligned16, p));
    if (!p.small && !aligned16 && ws_bytes < mk::merkle_ws_bytes(n, item_len))
        return ws_too_small(ws_bytes, mk::merkle_ws_bytes(n, item_len));
    return launch_plan(p, (const uint8_t*)d_items, (uint8_t*)d_out32, (uint8_t*)d_ws, ws_bytes, st);
}

int dev_finish(const void* d_roots, uint64_t nroots, uint64_t n_total, void* d_out32, hipStream_t st,
               void* d_pair_block, uint32_t pair_slot, uint32_t pair_epoch) {
    if (nroots == 0 || nroots > 2 * mk::kWave2Span)
        return fail(MK_EINVAL, "nroots %llu out of range (1..%u)", (unsigned long long)nroots, 2 * mk::kWave2Span);
    if (!d_roots || (!d_out32 && !d_pair_block)) return fail(MK_EINVAL, "null pointer");
    // the reference level loop over the shard roots (odd -> 0^128) plus the
    // length mix-in is one finalizing node pass of the two-lane latency kernel
    ReduceArgs a{};
    a.items = (const uint8_t*)d_roots;
    a.cin = nroots;
    a.c1 = nroots > 1 ? (nroots + 1) / 2 : 1;
    a.c1_full = nroots / 2;
    a.out = (uint8_t*)d_out32;
    a.n_items = n_total;
    a.levels = 64;
    a.finalize = 1;
    if (d_pair_block) {
        a.pair_block = (uint8_t*)d_pair_block;
        a.pair_slot = pair_slot;
        a.pair_epoch = pair_epoch;
        a.out = (uint8_t*)d_pair_block + 32 * pair_slot;
    }
    launch_wave3<false>(mk::kWaveThreads, 1, a, st);
    return launched();
}

uint64_t finish_ws_bytes(uint64_t count) {
    Plan p;
    if (count <= 2 * mk::kWave2Span) return 256;
    if (mk::make_plan(count, 32, false, 0, false, true, p, true, 0, 1) != MK_OK) return 0;
    return mk::plan_ws_bytes(p);
}

int dev_finish_nodes(const void* d_nodes, uint64_t count, uint64_t n_total, void* d_out32, void* d_ws,
                     uint64_t ws_bytes, hipStream_t st, void* d_pair_block, uint32_t pair_slot, uint32_t pair_epoch) {
    if (count <= 2 * mk::kWave2Span)
        return dev_finish(d_nodes, count, n_total, d_out32, st, d_pair_block, pair_slot, pair_epoch);
    if (!d_nodes || (!d_out32 && !d_pair_block)) return fail(MK_EINVAL, "null pointer");
    Plan p;
    TRY(mk::make_plan(count, 32, false, 0, false, ((uintptr_t)d_nodes % 16) == 0, p, true, 0, n_total));
    return launch_plan(p, (const uint8_t*)d_nodes, (uint8_t*)d_out32, (uint8_t*)d_ws, ws_bytes, st,
                       (uint8_t*)d_pair_block, pair_slot, pair_epoch);
}

int launch_elem_digests(const void* d_elems, uint64_t n, uint32_t elem_len, void* d_dig, hipStream_t st) {
    if (n == 0) return MK_OK;
    if (elem_len == 32 && ((uintptr_t)d_elems % 16) == 0)
        hipLaunchKernelGGL(mk::k_elem_digests<true>, dim3(ceil_div(n, 256)), dim3(256), 0, st,
                           (const uint8_t*)d_elems, n, elem_len, (uint4*)d_dig);
    else
        hipLaunchKernelGGL(mk::k_elem_digests<false>, dim3(ceil_div(n, 256)), dim3(256), 0, st,
                           (const uint8_t*)d_elems, n, elem_len, (uint4*)d_dig);
    return launched();
}

int host_tree_hash_elems_plain(const uint8_t* elems, uint64_t n, uint32_t elem_len, uint8_t* out) {
    if (!out || (n && elem_len && !elems)) return fail(MK_EINVAL, "null pointer");
    if (elem_len && n > (UINT64_MAX / 4) / elem_len) return fail(MK_EINVAL, "n * elem_len overflows");
    TRY(bind_call());
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    ElemPlan e;
    TRY(make_elem_plan(n, elem_len, true, e));
    const size_t inb = n * (size_t)elem_len;
    TRY(grow(c->in, inb));
    TRY(grow(c->out, 32));
    TRY(grow(c->ws, e.ws_bytes));
    hipStream_t st = c->stream;
    if (inb) HIPCHK(hipMemcpyAsync(c->in.p, elems, inb, hipMemcpyHostToDevice, st));
    TRY(dev_tree_hash_elems(c->in.p, n, elem_len, c->out.p, c->ws.p, c->ws.cap, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int host_merkle_hash_plain(const uint8_t* items, uint64_t n, uint32_t item_len, uint8_t* out) {
    if (!out || (n && item_len && !items)) return fail(MK_EINVAL, "null pointer");
    TRY(bind_call());
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    Plan p;
    TRY(mk::make_plan(n, item_len, false, 0, false, true, p));
    const size_t inb = n * (size_t)item_len;
    TRY(grow(c->in, inb));
    TRY(grow(c->out, 32));
    TRY(grow(c->ws, std::max<uint64_t>(p.small ? 256 : mk::plan_ws_bytes(p), list_tree_ws(n, item_len))));
    hipStream_t st = c->stream;
    if (inb) HIPCHK(hipMemcpyAsync(c->in.p, items, inb, hipMemcpyHostToDevice, st));
    if (list_tree_ok(n, item_len))
        TRY(dev_list_tree(c->in.p, n, item_len, c->out.p, (uint8_t*)c->ws.p, st));
    else
        TRY(launch_plan(p, (const uint8_t*)c->in.p, (uint8_t*)c->out.p, (uint8_t*)c->ws.p, c->ws.cap, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// First of `k` consecutive arrival-counter slots for the next fused-top
// launch (mk::g_arrive, round robin, never running past the last slot; each
// counter's last arriving workgroup resets it).
uint32_t next_arrive_slots(uint32_t k) {
    static std::atomic<uint64_t> next{0};
    uint64_t cur = next.load(std::memory_order_relaxed), start;
    do {
        const uint64_t base = cur % mk::kArriveSlots;
        start = base + k > mk::kArriveSlots ? cur + (mk::kArriveSlots - base) : cur;
    } while (!next.compare_exchange_weak(cur, start + k, std::memory_order_relaxed));
    return (uint32_t)(start % mk::kArriveSlots);
}
// Arrival slots one fused top of `parts` workgroups uses (k_trie_top_fused,
// k_merkle_top_fused): the final counter plus one per group of each grouping
// stage.  Reserving only those, not kTopGroupSlots, keeps ~1,300 small fused
// tops (C1's list tree: 16 workgroups, one slot) in flight on a device
// before a slot comes round again, where a fixed 129 allowed 31.
uint32_t top_arrive_slots(uint64_t parts) {
    uint32_t k = 1;
    while (mk::kTopGroupLog2 > 0 && parts > mk::kTopGroup) {
        parts = ceil_div(parts, (uint64_t)mk::kTopGroup);
        k += (uint32_t)parts;
    }
    return k;
}

}  // namespace mk::rt

extern "C" {

// ---- merkleHash ---------------------------------------------------------------
uint64_t mk_ssz_merkle_workspace_bytes(uint64_t n, uint32_t item_len) {
    Scope S(nullptr, false);
    return mk::merkle_ws_bytes(n, item_len);
}

int mk_dev_ssz_merkle_hash(mk_call* call, const void* d_items, uint64_t n, uint32_t item_len, void* d_out32,
                           void* d_ws, uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_merkle_hash(d_items, n, item_len, d_out32, d_ws, ws_bytes, (hipStream_t)stream);
    });
}

int mk_ssz_merkle_hash(mk_call* call, const uint8_t* items, uint64_t n, uint32_t item_len, uint8_t out[32]) {
    Scope S(call);
    return S.done(host_merkle_hash(items, n, item_len, out));
}

uint64_t mk_ssz_tree_hash_bytes_list_workspace_bytes(uint64_t n, uint32_t elem_len) {
    ElemPlan e;
    if (make_elem_plan(n, elem_len, true, e) != MK_OK) return 0;
    return e.ws_bytes;
}

int mk_dev_ssz_tree_hash_bytes_list(mk_call* call, const void* d_elems, uint64_t n, uint32_t elem_len,
                                    void* d_out32, void* d_ws, uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_tree_hash_elems(d_elems, n, elem_len, d_out32, d_ws, ws_bytes, (hipStream_t)stream);
    });
}

int mk_ssz_tree_hash_bytes_list(mk_call* call, const uint8_t* elems, uint64_t n, uint32_t elem_len, uint8_t out[32]) {
    Scope S(call);
    return S.done(host_tree_hash_elems(elems, n, elem_len, out));
}

uint64_t mk_ssz_merkle_many_workspace_bytes(const uint64_t* n, const uint32_t* item_len, uint32_t nlists) {
    Scope S(nullptr, false);
    mk::ManyPlan mp;
    std::vector<uint64_t> offs(nlists, 0);  // the layout does not depend on the offsets
    if (mk::make_many_plan(offs.data(), n, item_len, nlists, UINT64_MAX, true, mp) != MK_OK) return 0;
    return mp.ws_bytes;
}

int mk_dev_ssz_merkle_many(mk_call* call, const void* d_items, const uint64_t* offs, const uint64_t* n,
                           const uint32_t* item_len, uint32_t nlists, void* d_roots, void* d_ws, uint64_t ws_bytes,
                           void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (nlists && !offs) return fail(MK_EINVAL, "null offsets");
        mk::ManyPlan mp;
        TRY(mk::make_many_plan(offs, n, item_len, nlists, UINT64_MAX, ((uintptr_t)d_items % 16) == 0, mp));
        return dev_merkle_many(d_items, mp, nlists, d_roots, d_ws, ws_bytes, (hipStream_t)stream);
    });
}

int mk_ssz_merkle_many(mk_call* call, const uint8_t* items, const uint64_t* offs, const uint64_t* n,
                       const uint32_t* item_len, uint32_t nlists, uint8_t* roots) {
    Scope S(call);
    return S.done(host_merkle_many(items, offs, n, item_len, nlists, roots));
}

// ---- sharding -------------------------------------------------------------------
int mk_ssz_merkle_shard_plan(mk_call* call, uint64_t n, uint32_t item_len, uint32_t nshards, uint32_t* height,
                             uint32_t* nonempty, uint64_t* item_begin) {
    Scope S(call, false);
    if (!height || !nonempty || !item_begin) return S.done(fail(MK_EINVAL, "null pointer"));
    return S.done(mk::shard_plan(n, item_len, nshards, height, nonempty, item_begin));
}

int mk_dev_ssz_merkle_subtree(mk_call* call, const void* d_shard_items, uint64_t shard_n, uint32_t item_len,
                              uint32_t height, int pad_at_one, void* d_out32, void* d_ws, uint64_t ws_bytes,
                              void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (!d_out32 || (shard_n && !d_shard_items)) return fail(MK_EINVAL, "null pointer");
        Plan p;
        TRY(mk::make_plan(shard_n, item_len, true, height, pad_at_one != 0, ((uintptr_t)d_shard_items % 16) == 0, p));
        if (ws_bytes < mk::merkle_ws_bytes(shard_n, item_len))
            return ws_too_small(ws_bytes, mk::merkle_ws_bytes(shard_n, item_len));
        return launch_plan(p, (const uint8_t*)d_shard_items, (uint8_t*)d_out32, (uint8_t*)d_ws, ws_bytes,
                           (hipStream_t)stream);
    });
}

int mk_dev_ssz_merkle_subtree_frontier(mk_call* call, const void* d_shard_items, uint64_t shard_n,
                                       uint32_t item_len, uint32_t height, uint32_t frontier_log2, int pad_at_one,
                                       void* d_out, uint64_t* nodes_out, void* d_ws, uint64_t ws_bytes,
                                       void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (!d_out || (shard_n && !d_shard_items)) return fail(MK_EINVAL, "null pointer");
        Plan p;
        TRY(mk::make_plan(shard_n, item_len, true, height, pad_at_one != 0, ((uintptr_t)d_shard_items % 16) == 0, p,
                          false, frontier_log2));
        if (ws_bytes < mk::merkle_ws_bytes(shard_n, item_len))
            return ws_too_small(ws_bytes, mk::merkle_ws_bytes(shard_n, item_len));
        if (nodes_out) *nodes_out = p.out_nodes;
        return launch_plan(p, (const uint8_t*)d_shard_items, (uint8_t*)d_out, (uint8_t*)d_ws, ws_bytes,
                           (hipStream_t)stream);
    });
}

uint64_t mk_ssz_merkle_node_frontier_workspace_bytes(uint64_t count, uint32_t height, uint32_t frontier_log2) {
    Scope S(nullptr, false);
    Plan p;
    if (mk::make_plan(count, 32, true, height, true, true, p, true, frontier_log2) != MK_OK) return 0;
    return std::max<uint64_t>(256, mk::plan_ws_bytes(p));
}

int mk_dev_ssz_merkle_node_frontier(mk_call* call, const void* d_nodes, uint64_t count, uint32_t height,
                                    uint32_t frontier_log2, int pad_at_one, void* d_out, uint64_t* nodes_out,
                                    void* d_ws, uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (!d_out || !d_nodes || count == 0) return fail(MK_EINVAL, "null pointer or empty level");
        Plan p;
        TRY(mk::make_plan(count, 32, true, height, pad_at_one != 0, ((uintptr_t)d_nodes % 16) == 0, p, true,
                          frontier_log2));
        if (nodes_out) *nodes_out = frontier_log2 ? p.out_nodes : 1;
        return launch_plan(p, (const uint8_t*)d_nodes, (uint8_t*)d_out, (uint8_t*)d_ws, ws_bytes,
                           (hipStream_t)stream);
    });
}

uint64_t mk_ssz_merkle_finish_workspace_bytes(uint64_t count) {
    Scope S(nullptr, false);
    return finish_ws_bytes(count);
}

int mk_dev_ssz_merkle_finish_nodes(mk_call* call, const void* d_nodes, uint64_t count, uint64_t n_total,
                                   void* d_out32, void* d_ws, uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_finish_nodes(d_nodes, count, n_total, d_out32, d_ws, ws_bytes, (hipStream_t)stream);
    });
}

uint64_t mk_ssz_merkle_top_fused_workspace_bytes(uint64_t count0, uint64_t count1) {
    const uint64_t c[2] = {count0, count1};
    TopPlan p;
    return top_plan(c, count1 ? 2 : 1, p) == MK_OK ? p.ws : 0;
}

int mk_dev_ssz_merkle_top_fused(mk_call* call, const void* d_nodes0, uint64_t count0, uint64_t n0,
                                const void* d_nodes1, uint64_t count1, uint64_t n1, void* d_out, uint32_t epoch,
                                void* d_ws, uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        const uint32_t nl = count1 ? 2 : 1;
        const uint64_t c[2] = {count0, count1};
        const void* nodes[2] = {d_nodes0, d_nodes1};
        const uint64_t nit[2] = {n0, n1};
        TopPlan p;
        TRY(top_plan(c, nl, p));
        if (!d_out || !d_ws || !d_nodes0 || (nl == 2 && !d_nodes1)) return fail(MK_EINVAL, "null pointer");
        if (ws_bytes < p.ws) return fail(MK_ENOMEM, "workspace too small: %llu < %llu", (unsigned long long)ws_bytes,
                                         (unsigned long long)p.ws);
        if ((uintptr_t)d_nodes0 % 8 || (uintptr_t)d_nodes1 % 8 || (uintptr_t)d_ws % 16)
            return fail(MK_EINVAL, "nodes not 8-B aligned or workspace not 16-B aligned");
        if (nl == 2) {
            if (epoch == 0 || epoch >= (1u << 30))
                return fail(MK_EINVAL, "pair epoch %u out of range (1..2^30-1)", epoch);
            if ((uintptr_t)d_out % 16) return fail(MK_EINVAL, "pair block not 16-B aligned");
        }
        return launch_top_fused(p, nl, nodes, c, nit, d_out, epoch, d_ws, (hipStream_t)stream);
    });
}

int mk_dev_ssz_merkle_finish_nodes_pair(mk_call* call, const void* d_nodes, uint64_t count, uint64_t n_total,
                                        void* d_pair_block, uint32_t slot, uint32_t epoch, void* d_ws,
                                        uint64_t ws_bytes, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (!d_pair_block) return fail(MK_EINVAL, "null pointer");
        if (slot > 1) return fail(MK_EINVAL, "pair slot %u out of range (0..1)", slot);
        if (epoch == 0 || epoch >= (1u << 30)) return fail(MK_EINVAL, "pair epoch %u out of range (1..2^30-1)", epoch);
        if ((uintptr_t)d_pair_block % 16) return fail(MK_EINVAL, "pair block not 16-B aligned");
        return dev_finish_nodes(d_nodes, count, n_total, nullptr, d_ws, ws_bytes, (hipStream_t)stream,
                                d_pair_block, slot, epoch);
    });
}

int mk_dev_ssz_merkle_finish(mk_call* call, const void* d_roots, uint64_t nroots, uint64_t n_total, void* d_out32,
                             void* stream) {
    return dev_entry(call, stream, [&] { return dev_finish(d_roots, nroots, n_total, d_out32, (hipStream_t)stream); });
}

}  // extern "C"
