// hashutil.MerkleRoot and the deposit trie: batch build, append, branch,
// the pipelined stream of tries, the mk_trie handle and the mk_*deposit_trie*,
// mk_*merkle_root* and mk_verify_* entry points.
#include "runtime.hpp"
#include "trie_handle.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

#define MK_TRIE_TOP_MAX_LOG2 17
constexpr uint64_t kTrieTopMax = 1ull << MK_TRIE_TOP_MAX_LOG2;  // trie levels at or below: k_trie_top3
constexpr uint64_t kTrieTopWgs = 256;
constexpr uint64_t kAppendMaxRange = 1020;  // k_trie_append<1024>: one parent per lane pair

// Leaf hashes of deposits/values: offsets (device) or fixed-length records.
int dev_leaf_hashes(const void* d_data, const uint64_t* d_offs, uint64_t n, uint32_t fixed_len, uint4* out,
                    hipStream_t st) {
    if (n == 0) return MK_OK;
    if (d_offs) return dev_hash_var(d_data, d_offs, n, out, st);
    return dev_hash_batch(d_data, n, fixed_len, out, st);
}

// ---- hashutil.MerkleRoot (merkleRoot.go:12-30) ------------------------------------
// Heap o[1..2n): leaves o[n+i] = Hash(values[i]); o[i] = Hash(o[2i] || o[2i+1])
// for i = n-1 .. 1; the result is o[1].  The children of a heap band
// [2^k, 2^(k+1)) are the contiguous range [2^(k+1), 2^(k+2)), so with
// P = 2^floor(log2 n): when n > P the partial band [P, n) is one pairwise
// level over o[2P, 2n), and everything above is a power-of-two binary tree
// over o[P, 2P) -- a node-input merkle plan.  (The reference's spurious
// newSet[0] = Hash(nil || o[1]) is computed and discarded; it is skipped.)
uint64_t pow2_floor(uint64_t n) {
    uint64_t p = 1;
    while (p * 2 <= n) p *= 2;
    return p;
}

uint64_t merkle_root_ws(uint64_t n) {
    if (n == 0) return 0;
    const uint64_t P = pow2_floor(n);
    Plan p;
    uint64_t ws = 0;
    if (P > 1 && mk::make_plan(P, 32, true, ilog2(P), false, true, p, true) == MK_OK) ws = mk::plan_ws_bytes(p);
    return 64 * n + align256(ws) + 256;
}

int dev_merkle_root(const void* d_data, const uint64_t* d_offs, uint64_t n, uint32_t fixed_len, void* d_heap,
                    uint64_t heap_bytes, void* d_leaves32, void* d_out32, hipStream_t st) {
    if (n == 0) return fail(MK_EINVAL, "MerkleRoot of an empty list (reference: index out of range)");
    if (!d_heap || !d_out32 || (!d_offs && !d_data && fixed_len)) return fail(MK_EINVAL, "null pointer");
    if (heap_bytes < merkle_root_ws(n))
        return fail(MK_ENOMEM, "heap workspace too small: %llu < %llu", (unsigned long long)heap_bytes,
                    (unsigned long long)merkle_root_ws(n));
    uint8_t* heap = (uint8_t*)d_heap;  // node i at heap + 32 i (node 0 unused)
    uint4* leaves = (uint4*)(heap + 32 * n);
    TRY(dev_leaf_hashes(d_data, d_offs, n, fixed_len, leaves, st));
    if (d_leaves32 && d_leaves32 != (void*)leaves)
        HIPCHK(hipMemcpyAsync(d_leaves32, leaves, 32 * n, hipMemcpyDeviceToDevice, st));
    if (n == 1) {  // the loop body never runs: o[1] is the hashed value
        HIPCHK(hipMemcpyAsync(d_out32, leaves, 32, hipMemcpyDeviceToDevice, st));
        return MK_OK;
    }
    const uint64_t P = pow2_floor(n);
    if (P < n) {  // partial band [P, n): o[i] = Hash(o[2i] || o[2i+1]) over o[2P, 2n)
        hipLaunchKernelGGL(mk::k_trie_level, dim3(ceil_div(n - P, 256)), dim3(256), 0, st,
                           (const uint4*)(heap + 64 * P), 2 * (n - P), (uint4*)(heap + 32 * P));
        HIPCHK(hipGetLastError());
    }
    Plan p;
    TRY(mk::make_plan(P, 32, true, ilog2(P), false, true, p, true));
    uint8_t* ws = heap + 64 * n;
    return launch_plan(p, heap + 32 * P, (uint8_t*)d_out32, ws, heap_bytes - 64 * n, st);
}

// ---- deposit trie -------------------------------------------------------------------
uint4* trie_level(void* d_levels, uint64_t cap, uint32_t d) {
    return (uint4*)d_levels + 2 * mk::trie_level_off(cap, d);
}

int check_trie(uint64_t cap, uint64_t count, uint64_t k, uint32_t depth) {
    if (depth == 0 || depth > 63) return fail(MK_EINVAL, "depth %u out of range (1..63)", depth);
    if (count + k > cap) return fail(MK_EINVAL, "trie capacity %llu < %llu deposits", (unsigned long long)cap,
                                     (unsigned long long)(count + k));
    if (count + k > (1ull << depth))
        return fail(MK_EINVAL, "%llu deposits do not fit a depth-%u trie", (unsigned long long)(count + k), depth);
    return MK_OK;
}

// Most parents any level d .. d_end-1 has when the nodes [lo, c) of level d
// changed (the right edge of an append; lo = 0 for a batch top).
uint64_t edge_max_parents(uint64_t lo, uint64_t c, uint32_t d, uint32_t d_end) {
    uint64_t m = 0;
    for (; d < d_end; ++d) {
        const uint64_t plo = lo >> 1, cp = (c + 1) >> 1;
        m = std::max(m, cp - plo);
        lo = plo;
        c = cp;
    }
    return m;
}

// k_trie_spread over levels d .. d_end-1 (one wave per parent, <= 16 parents;
// with leaves.k > 0 it first hashes the new deposits into level 0 [lo, c))
int launch_trie_spread(void* d_levels, uint64_t cap, uint32_t d, uint64_t lo, uint64_t c, uint32_t d_end,
                       uint32_t depth, void* d_root32, hipStream_t st, mk::SpreadLeaves leaves = {}) {
    const uint64_t m = std::max<uint64_t>(edge_max_parents(lo, c, d, d_end), leaves.k);
    uint32_t* lv = (uint32_t*)d_levels;
    uint32_t* root = (uint32_t*)d_root32;
    if (m <= 1)
        hipLaunchKernelGGL(mk::k_trie_spread<1>, dim3(1), dim3(64), 0, st, lv, cap, d, lo, c, d_end, depth, root,
                           leaves);
    else if (m <= 2)
        hipLaunchKernelGGL(mk::k_trie_spread<2>, dim3(1), dim3(128), 0, st, lv, cap, d, lo, c, d_end, depth, root,
                           leaves);
    else if (m <= 4)
        hipLaunchKernelGGL(mk::k_trie_spread<4>, dim3(1), dim3(256), 0, st, lv, cap, d, lo, c, d_end, depth, root,
                           leaves);
    else if (m <= 16 && m <= mk::kSpreadWavesMax)
        hipLaunchKernelGGL(mk::k_trie_spread<16>, dim3(1), dim3(1024), 0, st, lv, cap, d, lo, c, d_end, depth, root,
                           leaves);
    else
        return fail(MK_EINVAL, "internal: trie edge of %llu parents for the spread kernel", (unsigned long long)m);
    return launched();
}

// Levels d_from+1 .. d_to of the batch build over `n` deposits, level d_from
// complete; the root (level depth node 0) to d_root32 when d_to == depth.
// nt_max / spread_max: the largest k_trie_top3 workgroup and k_trie_spread
// wave count (256 / 4: at most one wave per SIMD, which fits beside a
// resident k_trie_rec_lock<1024, 4, true> workgroup of 104 VGPRs).
int trie_levels_range(void* d_levels, uint64_t cap, uint64_t n, uint32_t d_from, uint32_t d_to, uint32_t depth,
                      void* d_root32, hipStream_t st, uint32_t nt_max = mk::kMidThreads,
                      uint32_t spread_max = mk::kSpreadWavesMax, bool fused = false) {
    // Wide levels: one launch per level (every lane busy); the narrow top
    // (<= 2^17 nodes) plus the zero-sibling tail: k_trie_top3 (bit-interleaved
    // lane pairs), log2(NT) levels per workgroup of NT inputs, the last
    // launch to the top.  `fused` (a whole trie alone on the stream): every
    // level from the first of <= 2^20 nodes to the root in one launch
    // (k_trie_top_fused).
    uint64_t c = mk::trie_count(n, d_from);
    uint32_t d = d_from;
    if (fused && d_to == depth && d_root32) {
        constexpr uint64_t NT = 1024;
        while (d < d_to && c > NT * NT) {
            const uint64_t cn = (c + 1) / 2;
            hipLaunchKernelGGL(mk::k_trie_level, dim3(ceil_div(cn, 256)), dim3(256), 0, st,
                               (const uint4*)trie_level(d_levels, cap, d), c, trie_level(d_levels, cap, d + 1));
            HIPCHK(hipGetLastError());
            c = cn;
            ++d;
        }
        hipLaunchKernelGGL(mk::k_trie_top_fused<NT>, dim3(ceil_div(c, NT)), dim3(NT), 0, st, (uint32_t*)d_levels, cap,
                           c, d, depth, (uint32_t*)d_root32, next_arrive_slots(top_arrive_slots(ceil_div(c, NT))));
        return launched();
    }
    while (d < d_to && c > kTrieTopMax) {
        const uint64_t cn = (c + 1) / 2;
        hipLaunchKernelGGL(mk::k_trie_level, dim3(ceil_div(cn, 256)), dim3(256), 0, st,
                           (const uint4*)trie_level(d_levels, cap, d), c, trie_level(d_levels, cap, d + 1));
        HIPCHK(hipGetLastError());
        c = cn;
        ++d;
    }
    bool root_done = false;
    while (d < d_to) {
        if (c <= 2 * spread_max) {  // the last <= 5 levels + zero-sibling tail
            void* root = d_to == depth ? d_root32 : nullptr;
            TRY(launch_trie_spread(d_levels, cap, d, 0, c, d_to, depth, root, st));
            root_done = root != nullptr;
            d = d_to;
            break;
        }
        uint32_t nt = mk::kWaveThreads;
        while (nt < nt_max && ceil_div(c, nt) > kTrieTopWgs) nt *= 2;
        while (nt < nt_max && c <= nt_max && c > nt) nt *= 2;  // the last <= nt_max nodes in one WG
        const uint64_t nwg = ceil_div(c, nt);
        uint32_t k = nwg == 1 ? d_to - d : std::min<uint32_t>(ilog2(nt), d_to - d);
        if (nwg == 1) {  // stop where k_trie_spread takes over
            uint64_t cc = c;
            uint32_t kk = 0;
            while (kk < k && cc > 2 * spread_max) {
                cc = (cc + 1) / 2;
                ++kk;
            }
            k = kk;
        }
        const uint32_t* src = (const uint32_t*)trie_level(d_levels, cap, d);
        uint32_t* dst = (uint32_t*)trie_level(d_levels, cap, d + 1);
        const uint64_t capn = mk::trie_count(cap, d + 1);
        switch (nt) {
            case 64: hipLaunchKernelGGL(mk::k_trie_top3<64>, dim3(nwg), dim3(64), 0, st, src, c, dst, k, capn); break;
            case 128: hipLaunchKernelGGL(mk::k_trie_top3<128>, dim3(nwg), dim3(128), 0, st, src, c, dst, k, capn); break;
            case 256: hipLaunchKernelGGL(mk::k_trie_top3<256>, dim3(nwg), dim3(256), 0, st, src, c, dst, k, capn); break;
            case 512: hipLaunchKernelGGL(mk::k_trie_top3<512>, dim3(nwg), dim3(512), 0, st, src, c, dst, k, capn); break;
            default: hipLaunchKernelGGL(mk::k_trie_top3<1024>, dim3(nwg), dim3(1024), 0, st, src, c, dst, k, capn); break;
        }
        HIPCHK(hipGetLastError());
        for (uint32_t i = 0; i < k; ++i) c = (c + 1) / 2;
        d += k;
    }
    if (d_to == depth && d_root32 && !root_done)
        HIPCHK(hipMemcpyAsync(d_root32, trie_level(d_levels, cap, depth), 32, hipMemcpyDeviceToDevice, st));
    return MK_OK;
}

// Levels 1..nlv of the batch build for the leaves [done, n) (level 0 holds
// them; the levels of [0, done) are already built): the suffix of each level,
// one k_trie_level launch per level.
int trie_suffix_levels(void* d_levels, uint64_t cap, uint64_t n, uint64_t done, uint32_t nlv, hipStream_t st) {
    for (uint32_t d = 0; d < nlv; ++d) {
        const uint64_t c = mk::trie_count(n, d), plo = done >> (d + 1);
        if (c <= 2 * plo) continue;  // nothing left at this level
        hipLaunchKernelGGL(mk::k_trie_level, dim3(ceil_div(((c + 1) >> 1) - plo, 256)), dim3(256), 0, st,
                           (const uint4*)(trie_level(d_levels, cap, d) + 2 * (2 * plo)), c - 2 * plo,
                           trie_level(d_levels, cap, d + 1) + 2 * plo);
        HIPCHK(hipGetLastError());
    }
    return MK_OK;
}

// Batch build front over an empty trie: leaf hashes into level 0, then
// levels 1 .. d_to.  A whole trie in one call (d_to == depth) of 280-B
// deposits at a 16-B aligned address: whole groups of the phase-locked
// k_trie_rec_lock_sm (leaves + levels 1-2 in one launch), the rest (a
// partial group) k_keccak_rec + k_trie_level.  A front whose top the caller
// runs elsewhere (d_to < depth: pipeline.TriePipeline overlaps trie i's top
// with trie i+1's front) keeps the free-running kernels: a locked workgroup
// fills its CU, so the top could not co-run (one process, same box,
// profiles/r04c-r04d: one trie 0.596 -> 0.582 ms locked, the stream of
// tries 0.514 -> 0.604 ms/step).
int trie_front(void* d_levels, uint64_t cap, const void* d_data, const uint64_t* d_offs, uint64_t n,
               uint32_t fixed_len, uint32_t d_to, uint32_t depth, void* d_root32, hipStream_t st) {
    constexpr uint32_t NT = 1024, DPT = 4, nlv = 2;  // k_trie_rec_lock_sm: 4 slots per thread, levels 0-2
    const uint64_t ng = (!d_offs && fixed_len == 280 && ((uintptr_t)d_data % 16) == 0 &&
                         n >= MK_TRIE_LOCK_MIN && d_to == depth && depth >= nlv)
                            ? n / (NT * DPT)
                            : 0;
    if (!ng) {
        TRY(dev_leaf_hashes(d_data, d_offs, n, fixed_len, trie_level(d_levels, cap, 0), st));
        return trie_levels_range(d_levels, cap, n, 0, d_to, depth, d_root32, st, mk::kMidThreads,
                                 mk::kSpreadWavesMax, d_to == depth);
    }
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    uint4* L[3];
    for (uint32_t d = 0; d <= nlv; ++d) L[d] = trie_level(d_levels, cap, d);
    // persistent: every workgroup runs the same number of groups where possible
    const uint64_t cap_wg = std::min<uint64_t>(MK_TRIE_LOCK_GRID, lock_grid_cap(st));
    const uint64_t grid = ceil_div(ng, ceil_div(ng, cap_wg));
    // slot-major (lane m, slot i: deposit 64 i + m), not the row form of the
    // stream's k_trie_rec_lock<1024, 4, true> (deposits 4m .. 4m + 3 per
    // lane): one trie 0.4908-0.4913 -> 0.4781-0.4798 ms, fetch 561 -> 535 MB
    // (profiles/r06/c5_slot_major/, interleaved on one box)
    hipLaunchKernelGGL(mk::k_trie_rec_lock_sm<NT>, dim3(grid), dim3(NT), 0, st, (const uint2*)d_data, ng, L[0], L[1],
                       L[2]);
    HIPCHK(hipGetLastError());
    const uint64_t done = ng * NT * DPT;
    if (done < n) {
        TRY(dev_hash_batch((const uint8_t*)d_data + done * 280, n - done, 280, L[0] + 2 * done, st));
        TRY(trie_suffix_levels(d_levels, cap, n, done, nlv, st));
    }
    return trie_levels_range(d_levels, cap, n, nlv, d_to, depth, d_root32, st, mk::kMidThreads, mk::kSpreadWavesMax,
                             true);
}

// A stream of tries with the previous trie's wide top in the front's
// lock-step slots (k_trie_rec_lock<1024, 4, true>): 280-B deposits at a 16-B
// aligned address, n a whole number of 4096-deposit groups, one group per
// workgroup (n / 4096 <= the stream's CUs), depth >= 7.
bool trie_pipe_ok(const void* d_data, uint64_t n, uint32_t fixed_len, uint32_t depth, hipStream_t st) {
    constexpr uint64_t G = 1024 * 4;
    return fixed_len == 280 && ((uintptr_t)d_data % 16) == 0 && n >= G && n % G == 0 &&
           n / G <= std::min<uint64_t>(MK_TRIE_LOCK_GRID, lock_grid_cap(st)) && depth >= 7;
}

// Levels 0..2 of the trie in d_levels and levels 3..7 of the previous one in
// d_prev (NULL: none), one launch.
int trie_front_pipe(void* d_levels, void* d_prev, uint64_t cap, const void* d_data, uint64_t n, uint32_t depth,
                    hipStream_t st) {
    if (inject_ehip()) return fail(MK_EHIP, "hipLaunchKernelGGL: injected failure (MK_INJECT_EHIP)");
    uint4* L[4];
    for (uint32_t d = 0; d < 4; ++d) L[d] = trie_level(d_levels, cap, d);
    mk::TriePrev prev{};
    if (d_prev) {
        prev.l2 = trie_level(d_prev, cap, 2);
        for (uint32_t k = 0; k < 5; ++k) prev.l[k] = trie_level(d_prev, cap, 3 + k);
        prev.live = 1;
    }
    const uint64_t ng = n / (1024 * 4);
    hipLaunchKernelGGL((mk::k_trie_rec_lock<1024, 4, true>), dim3(ng), dim3(1024), 0, st, (const uint2*)d_data, ng,
                       L[0], L[1], L[2], L[3], prev);
    return launched();
}

int dev_trie_append(void* d_levels, uint64_t cap, uint64_t count, const void* d_data, const uint64_t* d_offs,
                    uint64_t k, uint32_t fixed_len, uint32_t depth, void* d_root32, hipStream_t st) {
    TRY(check_trie(cap, count, k, depth));
    if (!d_root32 || (cap && !d_levels)) return fail(MK_EINVAL, "null pointer");
    if (k && !d_offs && !d_data && fixed_len) return fail(MK_EINVAL, "null deposits");
    if (count + k == 0) {
        HIPCHK(hipMemsetAsync(d_root32, 0, 32, st));
        return MK_OK;
    }
    if (k <= mk::kSpreadWavesMax && edge_max_parents(count, count + k, 0, depth) <= mk::kSpreadWavesMax) {
        // a few deposits (powchain's one log at a time): the leaf hashes and
        // the whole right edge in one single-workgroup launch
        const bool w8 = !d_offs && fixed_len % 8 == 0 && ((uintptr_t)d_data % 8) == 0;
        mk::SpreadLeaves lv{(const uint8_t*)d_data, d_offs, fixed_len, (uint32_t)k, (uint32_t)w8};
        // one deposit: a register chain with the siblings prefetched
        // (k_trie_append1: 100.5 against 102.6 us per append + Root() through
        // k_trie_spread<1>, 2^16-deposit trie, profiles/r06/append/)
        if (k == 1 && depth <= 64) {
            hipLaunchKernelGGL(mk::k_trie_append1, dim3(1), dim3(64), 0, st, (uint32_t*)d_levels, cap, count, depth,
                               (uint32_t*)d_root32, lv);
            return launched();
        }
        return launch_trie_spread(d_levels, cap, 0, count, count + k, depth, depth, d_root32, st, lv);
    }
    if (count == 0) return trie_front(d_levels, cap, d_data, d_offs, k, fixed_len, depth, depth, d_root32, st);
    // leaf hashes of the new deposits: Hash(depositData) (deposit_trie.go:32)
    TRY(dev_leaf_hashes(d_data, d_offs, k, fixed_len, trie_level(d_levels, cap, 0) + 2 * count, st));
    // right edge only: level d changes on [lo, c)
    uint64_t lo = count, c = count + k;
    uint32_t d = 0;
    while (d < depth && c - lo > kAppendMaxRange) {
        const uint64_t plo = lo >> 1;
        hipLaunchKernelGGL(mk::k_trie_level, dim3(ceil_div(((c + 1) >> 1) - plo, 256)), dim3(256), 0, st,
                           (const uint4*)(trie_level(d_levels, cap, d) + 2 * (2 * plo)), c - 2 * plo,
                           trie_level(d_levels, cap, d + 1) + 2 * plo);
        HIPCHK(hipGetLastError());
        lo = plo;
        c = (c + 1) >> 1;
        ++d;
    }
    if (d == depth) {
        HIPCHK(hipMemcpyAsync(d_root32, trie_level(d_levels, cap, depth), 32, hipMemcpyDeviceToDevice, st));
        return MK_OK;
    }
    // lane pairs (k_trie_append) while a level has more than kSpreadWavesMax
    // changed parents, then one state per wave (k_trie_spread) to the root
    uint32_t d_stop = d;
    uint64_t slo = lo, sc = c;
    while (d_stop < depth && edge_max_parents(slo, sc, d_stop, depth) > mk::kSpreadWavesMax) {
        slo >>= 1;
        sc = (sc + 1) >> 1;
        ++d_stop;
    }
    const uint64_t r = c - lo;
    uint32_t* lv = (uint32_t*)d_levels;
    uint32_t* root = (uint32_t*)d_root32;
    if (d_stop > d) {
        if (r <= 60)
            hipLaunchKernelGGL(mk::k_trie_append<64>, dim3(1), dim3(64), 0, st, lv, cap, d, lo, c, d_stop, depth, root);
        else if (r <= 252)
            hipLaunchKernelGGL(mk::k_trie_append<256>, dim3(1), dim3(256), 0, st, lv, cap, d, lo, c, d_stop, depth,
                               root);
        else
            hipLaunchKernelGGL(mk::k_trie_append<1024>, dim3(1), dim3(1024), 0, st, lv, cap, d, lo, c, d_stop, depth,
                               root);
        HIPCHK(hipGetLastError());
    }
    if (d_stop < depth) TRY(launch_trie_spread(d_levels, cap, d_stop, slo, sc, depth, depth, d_root32, st));
    return MK_OK;
}

int dev_trie_branch(const void* d_levels, uint64_t cap, uint64_t count, uint32_t depth, uint64_t index,
                    void* d_branch, hipStream_t st) {
    if (depth == 0 || depth > 63) return fail(MK_EINVAL, "depth %u out of range (1..63)", depth);
    if (!d_branch || (count && !d_levels)) return fail(MK_EINVAL, "null pointer");
    if (count > cap) return fail(MK_EINVAL, "count > capacity");
    hipLaunchKernelGGL(mk::k_trie_branch, dim3(1), dim3(64), 0, st, (const uint4*)d_levels, cap, count, depth, index,
                       (uint4*)d_branch);
    return launched();
}

// Branches of k indices and the root as of `as_of` <= count deposits, one
// launch: every workgroup walks the straddling chain itself, then its waves
// take one branch per turn (k_trie_branches_at).
constexpr uint64_t kBranchGridMax = 2048;  // workgroups: 8 per CU, the rest by grid stride
int dev_trie_branches_at(const void* d_levels, uint64_t cap, uint64_t count, uint32_t depth, uint64_t as_of,
                         const uint64_t* d_indices, uint64_t k, void* d_branches, void* d_root_at, hipStream_t st) {
    if (depth == 0 || depth > 63) return fail(MK_EINVAL, "depth %u out of range (1..63)", depth);
    if (count > cap) return fail(MK_EINVAL, "count > capacity");
    if (as_of > count)
        return fail(MK_EINVAL, "as_of %llu beyond %llu deposits", (unsigned long long)as_of, (unsigned long long)count);
    if ((as_of && !d_levels) || (k && (!d_indices || !d_branches))) return fail(MK_EINVAL, "null pointer");
    if (((uintptr_t)d_levels | (uintptr_t)d_branches | (uintptr_t)d_root_at) % 16 || (uintptr_t)d_indices % 8)
        return fail(MK_EINVAL, "levels, branches and root_at need 16-B alignment, indices 8-B");
    if (k > UINT64_MAX / (32ull * depth)) return fail(MK_EINVAL, "k x depth x 32 bytes overflow");
    if (k == 0 && !d_root_at) return MK_OK;
    const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(k, mk::kBranchWaves), kBranchGridMax));
    hipLaunchKernelGGL(mk::k_trie_branches_at, dim3(grid), dim3(64 * mk::kBranchWaves), 0, st, (const uint4*)d_levels,
                       cap, count, as_of, depth, d_indices, k, (uint4*)d_branches, (uint4*)d_root_at);
    return launched();
}

int dev_verify_deposits(const void* d_data, const uint64_t* d_offs, const void* d_branches, const uint64_t* d_indices,
                        uint64_t n, uint32_t depth, uint32_t tree_depth, const void* d_roots, uint32_t root_stride,
                        void* d_ok, hipStream_t st) {
    if (root_stride != 0 && root_stride != 32)
        return fail(MK_EINVAL, "root_stride %u (0: one root for the batch, 32: one per deposit)", root_stride);
    if (n == 0) return MK_OK;
    if (!d_offs || !d_indices || !d_roots || !d_ok || (depth && !d_branches)) return fail(MK_EINVAL, "null pointer");
    if (((uintptr_t)d_branches | (uintptr_t)d_roots) % 16 || ((uintptr_t)d_offs | (uintptr_t)d_indices) % 8)
        return fail(MK_EINVAL, "branches and roots need 16-B alignment, offsets and indices 8-B");
    hipLaunchKernelGGL(mk::k_verify_deposits, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const uint8_t*)d_data, d_offs,
                       (const uint4*)d_branches, d_indices, depth, tree_depth, (const uint4*)d_roots, root_stride, n,
                       (uint8_t*)d_ok);
    return launched();
}

int host_merkle_root(const uint8_t* data, const uint64_t* offs, uint64_t n, uint8_t* leaves_out,
                     uint8_t* out) {
    if (!out || (n && !offs)) return fail(MK_EINVAL, "null pointer");
    if (n == 0) return fail(MK_EINVAL, "MerkleRoot of an empty list (reference: index out of range)");
    TRY(bind_call());
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    const size_t inb = offs[n] - offs[0];
    const int64_t ulen = uniform_len(offs, n);
    const uint64_t wsb = merkle_root_ws(n);
    TRY(grow(c->in, inb + 16));
    TRY(grow(c->aux, 8 * (n + 1)));
    TRY(grow(c->ws, wsb));
    TRY(grow(c->out, 32));
    if (inb) HIPCHK(hipMemcpyAsync(c->in.p, data + offs[0], inb, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> rel;
    if (ulen < 0) {
        rel.assign(offs, offs + n + 1);
        for (auto& o : rel) o -= offs[0];
        HIPCHK(hipMemcpyAsync(c->aux.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
    }
    TRY(dev_merkle_root(c->in.p, ulen < 0 ? (const uint64_t*)c->aux.p : nullptr, n, ulen < 0 ? 0 : (uint32_t)ulen,
                        c->ws.p, wsb, nullptr, c->out.p, st));
    HIPCHK(hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, st));
    if (leaves_out) HIPCHK(hipMemcpyAsync(leaves_out, (uint8_t*)c->ws.p + 32 * n, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // `rel` and the caller's buffers are released after this
    return MK_OK;
}

// Uploads host deposits (data, offs[k+1]) for an append; fixed_len > 0 when uniform.
int upload_deposits(DevCtx* c, DevBuf& in, DevBuf& offs_buf, const uint8_t* data, const uint64_t* offs,
                    uint64_t k, const uint64_t** d_offs, uint32_t* fixed_len, std::vector<uint64_t>& rel) {
    const size_t inb = offs[k] - offs[0];
    const int64_t ulen = uniform_len(offs, k);
    TRY(grow(in, inb + 16));
    if (inb) HIPCHK(hipMemcpyAsync(in.p, data + offs[0], inb, hipMemcpyHostToDevice, c->stream));
    if (ulen >= 0) {
        *d_offs = nullptr;
        *fixed_len = (uint32_t)ulen;
        return MK_OK;
    }
    rel.assign(offs, offs + k + 1);
    for (auto& o : rel) o -= offs[0];
    TRY(grow(offs_buf, 8 * (k + 1)));
    HIPCHK(hipMemcpyAsync(offs_buf.p, rel.data(), 8 * (k + 1), hipMemcpyHostToDevice, c->stream));
    *d_offs = (const uint64_t*)offs_buf.p;
    *fixed_len = 0;
    return MK_OK;
}

int host_trie_build(const uint8_t* data, const uint64_t* offs, uint64_t n, uint32_t depth,
                    uint8_t* levels_out, uint8_t* root) {
    if (!root || (n && !offs)) return fail(MK_EINVAL, "null pointer");
    TRY(check_trie(n, 0, n, depth));
    if (n == 0) {
        std::memset(root, 0, 32);
        return MK_OK;
    }
    TRY(bind_call());
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    const uint64_t lv_bytes = mk_deposit_trie_levels_bytes(n, depth);
    TRY(grow(c->ws, lv_bytes));
    TRY(grow(c->out, 32));
    const uint64_t* d_offs = nullptr;
    uint32_t fixed = 0;
    std::vector<uint64_t> rel;
    TRY(upload_deposits(c, c->in, c->aux, data, offs, n, &d_offs, &fixed, rel));
    TRY(dev_trie_append(c->ws.p, n, 0, c->in.p, d_offs, n, fixed, depth, c->out.p, st));
    HIPCHK(hipMemcpyAsync(root, c->out.p, 32, hipMemcpyDeviceToHost, st));
    if (levels_out) HIPCHK(hipMemcpyAsync(levels_out, c->ws.p, lv_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// keep == nullptr: synchronous (the caller's buffers may die on return);
// otherwise the relative offsets live in *keep and the caller synchronizes.
int trie_append_locked(mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k,
                       std::vector<uint64_t>* keep = nullptr) {
    if (k == 0) return MK_OK;
    TRY(check_trie(UINT64_MAX, t->count, k, t->depth));
    TRY(bind_dev(t->dev));
    DevCtx* c = ctx();
    hipStream_t st = c->stream;
    if (t->count + k > t->cap) {  // double the capacity, moving every level to its new slot
        uint64_t ncap = std::max(2 * t->cap, t->count + k);
        if (t->depth < 63) ncap = std::min<uint64_t>(ncap, 1ull << t->depth);
        DevBuf nl;
        TRY(grow(nl, mk_deposit_trie_levels_bytes(ncap, t->depth)));
        for (uint32_t d = 0; d <= t->depth && t->count; ++d)
            HIPCHK(hipMemcpyAsync(trie_level(nl.p, ncap, d), trie_level(t->levels.p, t->cap, d),
                                  32 * mk::trie_count(t->count, d), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(t->levels.p);
        t->levels = nl;
        t->cap = ncap;
    }
    const uint64_t* d_offs = nullptr;
    uint32_t fixed = 0;
    std::vector<uint64_t> own;
    std::vector<uint64_t>& rel = keep ? *keep : own;
    TRY(upload_deposits(c, t->in, t->offs, data, offs, k, &d_offs, &fixed, rel));
    TRY(dev_trie_append(t->levels.p, t->cap, t->count, t->in.p, d_offs, k, fixed, t->depth, t->root.p, st));
    if (!keep) HIPCHK(hipStreamSynchronize(st));  // the caller's buffers and `rel` are released after this
    t->count += k;
    return MK_OK;
}

int trie_append(mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k) {
    if (!t || (k && !offs)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    return trie_append_locked(t, data, offs, k);
}

int trie_root_locked(mk_trie* t, uint8_t* root) {
    if (t->count == 0) {
        std::memset(root, 0, 32);
        return MK_OK;
    }
    TRY(bind_dev(t->dev));
    HIPCHK(hipMemcpyAsync(root, t->root.p, 32, hipMemcpyDeviceToHost, ctx()->stream));
    HIPCHK(hipStreamSynchronize(ctx()->stream));
    return MK_OK;
}

int trie_root(mk_trie* t, uint8_t* root) {
    if (!t || !root) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    return trie_root_locked(t, root);
}

// saveInTrie over a batch of logs (service.go:379-386 called per log by
// ProcessDepositLog :248-258, which skips a log whose check fails): in log
// order, deposit j is appended iff Root() before it equals log_roots[j].
// A round appends every remaining deposit at once, computes the root after
// each (k_trie_prefix_roots) and compares on the host; at the first
// mismatch the trie is cut back to the deposits before it (the right edge
// of the new last leaf recomputed) and the next round starts after the
// skipped log.
int trie_save_logs(mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k,
                   const uint8_t* log_roots, uint8_t* accepted) {
    if (!t || (k && (!offs || !log_roots || !accepted))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    uint64_t pos = 0;
    while (pos < k) {
        const uint64_t m = k - pos;
        const uint64_t count0 = t->count;
        TRY(bind_dev(t->dev));
        hipStream_t st = ctx()->stream;
        // d_roots[f] = Root() before log pos + f: [0] the current root, [1..m]
        // the root after each appended deposit (the last one is the append's)
        TRY(grow(t->branch, std::max<size_t>(32 * (size_t)t->depth, 32 * (m + 1))));
        uint8_t* d_roots = (uint8_t*)t->branch.p;
        if (count0)
            HIPCHK(hipMemcpyAsync(d_roots, t->root.p, 32, hipMemcpyDeviceToDevice, st));
        else
            HIPCHK(hipMemsetAsync(d_roots, 0, 32, st));
        std::vector<uint64_t> rel;
        TRY(trie_append_locked(t, data, offs + pos, m, &rel));
        if (m > 1) {  // one wave per prefix, one wave per SIMD
            hipLaunchKernelGGL((mk::k_trie_prefix_roots<4>), dim3(ceil_div(m - 1, 4)), dim3(256), 0, st,
                               (const uint4*)t->levels.p, t->cap, count0, m - 1, t->depth, (uint4*)(d_roots + 32));
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(d_roots + 32 * m, t->root.p, 32, hipMemcpyDeviceToDevice, st));
        std::vector<uint8_t> roots(32 * (m + 1));
        HIPCHK(hipMemcpyAsync(roots.data(), d_roots, 32 * (m + 1), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        uint64_t f = 0;
        while (f < m && std::memcmp(roots.data() + 32 * f, log_roots + 32 * (pos + f), 32) == 0) {
            accepted[pos + f] = 1;
            ++f;
        }
        if (f == m) break;
        accepted[pos + f] = 0;  // skipped; the deposits after it were appended tentatively
        t->count = count0 + f;
        if (t->count) {  // recompute the last leaf's path without the cut deposits
            TRY(launch_trie_spread(t->levels.p, t->cap, 0, t->count - 1, t->count, t->depth, t->depth, t->root.p,
                                   st));
            HIPCHK(hipStreamSynchronize(st));
        }
        pos += f + 1;
    }
    return MK_OK;
}

int trie_branch(mk_trie* t, uint64_t index, uint8_t* branch) {
    if (!t || !branch) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (t->count == 0) {
        std::memset(branch, 0, 32 * (size_t)t->depth);
        return MK_OK;
    }
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    TRY(dev_trie_branch(t->levels.p, t->cap, t->count, t->depth, index, t->branch.p, st));
    HIPCHK(hipMemcpyAsync(branch, t->branch.p, 32 * (size_t)t->depth, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// Branches of k indices (and the root) as of `as_of` deposits.  The handle's
// scratch holds [root 32 B | chunk indices | chunk branches]; a chunk is at
// most kBranchChunk indices (8.3 MB of scratch at depth 32), one launch, one
// read-back and one synchronize each.
constexpr uint64_t kBranchChunk = 8192;
int trie_branches(mk_trie* t, uint64_t as_of, const uint64_t* indices, uint64_t k, uint8_t* branches,
                  uint8_t* root_at) {
    if (!t || (k && (!indices || !branches))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (as_of > t->count)
        return fail(MK_EINVAL, "as_of %llu beyond %llu deposits", (unsigned long long)as_of,
                    (unsigned long long)t->count);
    const size_t bb = 32 * (size_t)t->depth;  // one branch
    if (k > SIZE_MAX / bb) return fail(MK_EINVAL, "k x depth x 32 bytes overflow");
    if (as_of == 0) {  // no node existed yet: every sibling and the root read 0^32
        if (k) std::memset(branches, 0, bb * k);
        if (root_at) std::memset(root_at, 0, 32);
        return MK_OK;
    }
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    const uint64_t m_max = std::min(k, kBranchChunk);
    const size_t idx_off = 32, br_off = idx_off + ((8 * m_max + 15) & ~(size_t)15);
    TRY(grow(t->branch, br_off + bb * m_max));
    uint8_t* base = (uint8_t*)t->branch.p;
    uint64_t pos = 0;
    do {
        const uint64_t m = std::min(k - pos, kBranchChunk);
        void* d_root = (pos == 0 && root_at) ? base : nullptr;
        if (m) HIPCHK(hipMemcpyAsync(base + idx_off, indices + pos, 8 * m, hipMemcpyHostToDevice, st));
        TRY(dev_trie_branches_at(t->levels.p, t->cap, t->count, t->depth, as_of, (const uint64_t*)(base + idx_off), m,
                                 base + br_off, d_root, st));
        if (m) HIPCHK(hipMemcpyAsync(branches + bb * pos, base + br_off, bb * m, hipMemcpyDeviceToHost, st));
        if (d_root) HIPCHK(hipMemcpyAsync(root_at, base, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        pos += m;
    } while (pos < k);
    return MK_OK;
}

int trie_leaves(mk_trie* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    if (!t || (cnt && !out)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> tl(t->mu);
    if (first > t->count || cnt > t->count - first)
        return fail(MK_EINVAL, "leaves [%llu, +%llu) beyond %llu deposits", (unsigned long long)first,
                    (unsigned long long)cnt, (unsigned long long)t->count);
    if (!cnt) return MK_OK;
    TRY(bind_dev(t->dev));
    hipStream_t st = ctx()->stream;
    HIPCHK(hipMemcpyAsync(out, trie_level(t->levels.p, t->cap, 0) + 2 * first, 32 * cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int host_verify(const uint8_t* leaves, const uint8_t* branches, const uint64_t* indices, uint64_t n,
                uint32_t depth, uint32_t tree_depth, const uint8_t* roots, uint8_t* ok) {
    if (n && (!leaves || !indices || !roots || !ok || (depth && !branches))) return fail(MK_EINVAL, "null pointer");
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    const size_t bb = 32 * (size_t)depth * n;
    TRY(grow(c->in, bb + 64 * n + 16));
    TRY(grow(c->aux, 8 * n));
    TRY(grow(c->out, n));
    uint8_t* base = (uint8_t*)c->in.p;
    uint8_t* d_leaves = base;
    uint8_t* d_roots = base + 32 * n;
    uint8_t* d_br = base + 64 * n;
    HIPCHK(hipMemcpyAsync(d_leaves, leaves, 32 * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_roots, roots, 32 * n, hipMemcpyHostToDevice, st));
    if (bb) HIPCHK(hipMemcpyAsync(d_br, branches, bb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->aux.p, indices, 8 * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mk::k_verify_branches, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const uint4*)d_leaves,
                       (const uint4*)d_br, (const uint64_t*)c->aux.p, depth, tree_depth, (const uint4*)d_roots, n,
                       (uint8_t*)c->out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ok, c->out.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

int host_verify_deposits(const uint8_t* data, const uint64_t* offs, const uint8_t* branches, const uint64_t* indices,
                         uint64_t n, uint32_t depth, uint32_t tree_depth, const uint8_t* roots, uint32_t root_stride,
                         uint8_t* ok) {
    if (root_stride != 0 && root_stride != 32)
        return fail(MK_EINVAL, "root_stride %u (0: one root for the batch, 32: one per deposit)", root_stride);
    if (n && (!offs || !indices || !roots || !ok || (depth && !branches))) return fail(MK_EINVAL, "null pointer");
    if (n && offs[n] > offs[0] && !data) return fail(MK_EINVAL, "null deposit data");
    TRY(bind_call());
    if (n == 0) return MK_OK;
    DevCtx* c = ctx();
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = c->stream;
    const size_t inb = offs[n] - offs[0], bb = 32 * (size_t)depth * n, rb = root_stride ? 32 * n : 32;
    // in: [roots | branches | data], aux: [offsets (n + 1) | indices (n)]
    TRY(grow(c->in, rb + bb + inb + 16));
    TRY(grow(c->aux, 8 * (2 * n + 1)));
    TRY(grow(c->out, n));
    uint8_t* d_roots = (uint8_t*)c->in.p;
    uint8_t* d_br = d_roots + rb;
    uint8_t* d_data = d_br + bb;
    uint64_t* d_offs = (uint64_t*)c->aux.p;
    uint64_t* d_idx = d_offs + n + 1;
    std::vector<uint64_t> rel(offs, offs + n + 1);
    for (auto& o : rel) o -= offs[0];
    HIPCHK(hipMemcpyAsync(d_roots, roots, rb, hipMemcpyHostToDevice, st));
    if (bb) HIPCHK(hipMemcpyAsync(d_br, branches, bb, hipMemcpyHostToDevice, st));
    if (inb) HIPCHK(hipMemcpyAsync(d_data, data + offs[0], inb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_offs, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_idx, indices, 8 * n, hipMemcpyHostToDevice, st));
    TRY(dev_verify_deposits(d_data, d_offs, d_br, d_idx, n, depth, tree_depth, d_roots, root_stride, c->out.p, st));
    HIPCHK(hipMemcpyAsync(ok, c->out.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // `rel` and the caller's buffers are released after this
    return MK_OK;
}

}  // namespace

extern "C" {

// ---- hashutil.MerkleRoot -----------------------------------------------------------
uint64_t mk_merkle_root_workspace_bytes(uint64_t n) {
    Scope S(nullptr, false);
    return merkle_root_ws(n);
}

int mk_dev_merkle_root(mk_call* call, const void* d_data, const uint64_t* d_offs, uint64_t n, uint32_t fixed_len,
                       void* d_heap, uint64_t heap_bytes, void* d_leaves32, void* d_out32, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_merkle_root(d_data, d_offs, n, fixed_len, d_heap, heap_bytes, d_leaves32, d_out32,
                                           (hipStream_t)stream);
    });
}

int mk_merkle_root(mk_call* call, const uint8_t* data, const uint64_t* offs, uint64_t n, uint8_t* leaves_out,
                   uint8_t out[32]) {
    Scope S(call);
    return S.done(host_merkle_root(data, offs, n, leaves_out, out));
}

// ---- deposit trie -------------------------------------------------------------------
uint64_t mk_deposit_trie_levels_bytes(uint64_t capacity, uint32_t depth) {
    if (capacity == 0) return 0;
    return 32 * mk::trie_levels_nodes(capacity, depth);
}

int mk_dev_deposit_trie_append(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, const void* d_data,
                               const uint64_t* d_offs, uint64_t k, uint32_t fixed_len, uint32_t depth,
                               void* d_root32, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_trie_append(d_levels, capacity, count, d_data, d_offs, k, fixed_len, depth, d_root32,
                                           (hipStream_t)stream);
    });
}

int mk_dev_deposit_trie_build(mk_call* call, void* d_levels, uint64_t capacity, const void* d_data,
                              const uint64_t* d_offs, uint64_t n, uint32_t fixed_len, uint32_t d_to, uint32_t depth,
                              void* d_root32, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        TRY(check_trie(capacity, 0, n, depth));
        if (d_to > depth) return fail(MK_EINVAL, "level %u out of range (0..%u)", d_to, depth);
        if (n == 0) return fail(MK_EINVAL, "empty trie");
        if (!d_levels || (d_to == depth && !d_root32) || (!d_offs && !d_data && fixed_len))
            return fail(MK_EINVAL, "null pointer");
        return trie_front(d_levels, capacity, d_data, d_offs, n, fixed_len, d_to, depth,
                          d_to == depth ? d_root32 : nullptr, (hipStream_t)stream);
    });
}

int mk_deposit_trie_pipe_ok(const void* d_data, uint64_t n, uint32_t deposit_len, uint32_t depth, void* stream) {
    // the same check mk_dev_deposit_trie_build_pipe makes, on the caller's
    // stream (its CU mask bounds the persistent grid), on its device
    Scope S(nullptr);
    if (bind_stream((hipStream_t)stream)) return S.done(0);
    return S.done(trie_pipe_ok(d_data, n, deposit_len, depth, (hipStream_t)stream) ? 1 : 0);
}

int mk_dev_deposit_trie_build_pipe(mk_call* call, void* d_levels, void* d_prev_levels, uint64_t capacity,
                                   const void* d_data, uint64_t n, uint32_t deposit_len, uint32_t depth,
                                   void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        TRY(check_trie(capacity, 0, n, depth));
        if (!d_levels || !d_data) return fail(MK_EINVAL, "null pointer");
        if (d_prev_levels == d_levels) return fail(MK_EINVAL, "the previous trie's levels alias this trie's");
        if (!trie_pipe_ok(d_data, n, deposit_len, depth, (hipStream_t)stream))
            return fail(MK_EINVAL, "pipelined front needs 280-B deposits, 16-B aligned, n a multiple of 4096 "
                                          "with one group per CU, depth >= 7 (n = %llu)", (unsigned long long)n);
        return trie_front_pipe(d_levels, d_prev_levels, capacity, d_data, n, depth, (hipStream_t)stream);
    });
}

int mk_dev_deposit_trie_pipe_top(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, uint32_t depth,
                                 void* d_root32, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        TRY(check_trie(capacity, count, 0, depth));
        if (!d_levels || !d_root32 || count == 0) return fail(MK_EINVAL, "null pointer or empty trie");
        if (depth < 7) return fail(MK_EINVAL, "depth %u < 7", depth);
        return trie_levels_range(d_levels, capacity, count, 7, depth, depth, d_root32, (hipStream_t)stream, 256, 4);
    });
}

int mk_dev_deposit_trie_levels(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, uint32_t d_from,
                               uint32_t d_to, uint32_t depth, void* d_root32, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        TRY(check_trie(capacity, count, 0, depth));
        if (d_from > d_to || d_to > depth) return fail(MK_EINVAL, "levels %u..%u out of range", d_from, d_to);
        if (!d_levels || count == 0 || (d_to == depth && !d_root32))
            return fail(MK_EINVAL, "null pointer or empty trie");
        return trie_levels_range(d_levels, capacity, count, d_from, d_to, depth, d_root32, (hipStream_t)stream);
    });
}

int mk_dev_deposit_trie_branch(mk_call* call, const void* d_levels, uint64_t capacity, uint64_t count,
                               uint32_t depth, uint64_t index, void* d_branch, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_trie_branch(d_levels, capacity, count, depth, index, d_branch, (hipStream_t)stream);
    });
}

int mk_deposit_trie_build(mk_call* call, const uint8_t* data, const uint64_t* offs, uint64_t n, uint32_t depth,
                          uint8_t* levels_out, uint8_t root[32]) {
    Scope S(call);
    return S.done(host_trie_build(data, offs, n, depth, levels_out, root));
}

int mk_deposit_trie_new(mk_call* call, uint32_t depth, uint64_t capacity, mk_trie** out) {
    Scope S(call);
    if (!out) return S.done(fail(MK_EINVAL, "null pointer"));
    *out = nullptr;
    if (depth == 0 || depth > 63) return S.done(fail(MK_EINVAL, "depth %u out of range (1..63)", depth));
    int rc = bind_call();
    if (rc) return S.done(rc);
    auto* t = new (std::nothrow) mk_trie();
    if (!t) return S.done(fail(MK_ENOMEM, "trie allocation failed"));
    t->dev = t_bound;
    t->depth = depth;
    t->cap = std::max<uint64_t>(capacity, 1024);
    if (depth < 63) t->cap = std::min<uint64_t>(t->cap, 1ull << depth);
    rc = grow(t->levels, mk_deposit_trie_levels_bytes(t->cap, depth));
    if (!rc) rc = grow(t->root, 32);
    if (!rc) rc = grow(t->branch, 32 * (size_t)depth);
    if (rc) {
        mk_deposit_trie_free(t);
        return S.done(rc);
    }
    *out = t;
    return S.done(MK_OK);
}

void mk_deposit_trie_free(mk_trie* t) {
    if (!t) return;
    int saved = -1;
    const bool restore = hipGetDevice(&saved) == hipSuccess;
    (void)hipSetDevice(t->dev);
    for (DevBuf* b : {&t->levels, &t->root, &t->in, &t->offs, &t->branch})
        if (b->p) (void)hipFree(b->p);
    if (restore) (void)hipSetDevice(saved);
    delete t;
}

uint64_t mk_deposit_trie_count(const mk_trie* t) { return t ? t->count : 0; }

int mk_deposit_trie_append(mk_call* call, mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k) {
    Scope S(call);
    return S.done(trie_append(t, data, offs, k));
}

int mk_deposit_trie_root(mk_call* call, mk_trie* t, uint8_t root[32]) {
    Scope S(call);
    return S.done(trie_root(t, root));
}

int mk_deposit_trie_save_logs(mk_call* call, mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k,
                              const uint8_t* log_roots, uint8_t* accepted) {
    Scope S(call);
    return S.done(trie_save_logs(t, data, offs, k, log_roots, accepted));
}

int mk_deposit_trie_branch(mk_call* call, mk_trie* t, uint64_t index, uint8_t* branch) {
    Scope S(call);
    return S.done(trie_branch(t, index, branch));
}

int mk_dev_deposit_trie_branches(mk_call* call, const void* d_levels, uint64_t capacity, uint64_t count,
                                 uint32_t depth, uint64_t as_of, const uint64_t* d_indices, uint64_t k,
                                 void* d_branches, void* d_root_at, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_trie_branches_at(d_levels, capacity, count, depth, as_of, d_indices, k, d_branches, d_root_at,
                                    (hipStream_t)stream);
    });
}

int mk_deposit_trie_branches(mk_call* call, mk_trie* t, uint64_t as_of, const uint64_t* indices, uint64_t k,
                             uint8_t* branches, uint8_t* root_at) {
    Scope S(call);
    return S.done(trie_branches(t, as_of, indices, k, branches, root_at));
}

int mk_deposit_trie_root_at(mk_call* call, mk_trie* t, uint64_t as_of, uint8_t root[32]) {
    Scope S(call);
    if (!root) return S.done(fail(MK_EINVAL, "null pointer"));
    return S.done(trie_branches(t, as_of, nullptr, 0, nullptr, root));
}

int mk_dev_verify_deposits(mk_call* call, const void* d_data, const uint64_t* d_offs, const void* d_branches,
                           const uint64_t* d_indices, uint64_t n, uint32_t depth, uint32_t tree_depth,
                           const void* d_roots, uint32_t root_stride, void* d_ok, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        return dev_verify_deposits(d_data, d_offs, d_branches, d_indices, n, depth, tree_depth, d_roots, root_stride,
                                   d_ok, (hipStream_t)stream);
    });
}

int mk_verify_deposits(mk_call* call, const uint8_t* data, const uint64_t* offs, const uint8_t* branches,
                       const uint64_t* indices, uint64_t n, uint32_t depth, uint32_t tree_depth, const uint8_t* roots,
                       uint32_t root_stride, uint8_t* ok) {
    Scope S(call);
    return S.done(host_verify_deposits(data, offs, branches, indices, n, depth, tree_depth, roots, root_stride, ok));
}

int mk_deposit_trie_leaves(mk_call* call, mk_trie* t, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(trie_leaves(t, first, cnt, out));
}

int mk_verify_merkle_branches(mk_call* call, const uint8_t* leaves, const uint8_t* branches,
                              const uint64_t* indices, uint64_t n, uint32_t depth, uint32_t tree_depth,
                              const uint8_t* roots, uint8_t* ok) {
    Scope S(call);
    return S.done(host_verify(leaves, branches, indices, n, depth, tree_depth, roots, ok));
}

}  // extern "C"
