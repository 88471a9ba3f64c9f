// HIP kernels of the MI355X Merkleization engine (gfx950 only).
//
// Hot path: ssz.merkleHash (reference shared/ssz/hash.go:194-239) over a flat
// array of n items of `item_len` bytes, plus the digest it is built on
// (hashutil.Hash, shared/hashutil/hash.go:11-25) and the deposit trie
// (shared/trieutil/deposit_trie.go:29-81).
//
// Tree shape of merkleHash, restated for a flat buffer:
//   cb      = item_len < 128 ? (128 / item_len) * item_len : item_len
//   chunk i = bytes [i*cb, min(total, (i+1)*cb))          (last may be short)
//   level 1 = "windows": node j = K(chunk 2j || chunk 2j+1), or
//             K(chunk 2j || 0^128) when 2j+1 == nchunks (odd count)
//   level l>1: node j = K(n[2j] || n[2j+1]) or K(n[2j] || 0^128) when odd;
//             a level with a single node is the root (no more hashing)
//   final   = K(root || le64(n) || 0^24)
// For item_len | 128 every window is 256 contiguous bytes of the input, so
// level 1 is a pure streaming pass (2 Keccak blocks per window).
//
// This file is the one kernel translation unit.  Every kernels_*.hip is a part of it and none is an object of its
// own ("Kernel files").  A part is included where its lines have always stood, the first
// two inside the one open `namespace mk`: the order of definitions, and where the namespace closes, decide
// where each kernel lands in the code object.  The split is not finished: the groups still below (merkleHash
// passes, [][N]byte lists, k_wave3, batched Keccak, trie fronts, appends and branches, many lists) leave the same
// way.  A new kernel file goes to the end of the list.
#define MK_KERNEL_UNIT 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elem_dev.hpp"
#include "hash_dev.hpp"
#include "keccak_dev.hpp"
#include "merkle_kernels.hpp"
#include "spread3_dev.hpp"

namespace mk {

// ----------------------------------------------------------------------------
// Full 256-B window (two Keccak blocks) for the general leaf paths
// (first_level_generic, k_spread_leaf neighbours): the whole window is in
// registers before the first permutation, so each 128-B line is fetched once.
// The throughput leaf pass uses hash_window256_split below instead.
#define MK_MIN_WAVES 1

__device__ __forceinline__ void hash_window256(const uint4* __restrict__ w, uint4& d0, uint4& d1) {
    State s;
    zero(s);
    uint4 v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = ld_stream(w + k);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s.lo[2 * k] ^= v[k].x;
        s.hi[2 * k] ^= v[k].y;
        s.lo[2 * k + 1] ^= v[k].z;
        s.hi[2 * k + 1] ^= v[k].w;
    }
    s.lo[16] ^= v[8].x;
    s.hi[16] ^= v[8].y;
    keccak_f(s);
    s.lo[0] ^= v[8].z;
    s.hi[0] ^= v[8].w;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        s.lo[1 + 2 * k] ^= v[9 + k].x;
        s.hi[1 + 2 * k] ^= v[9 + k].y;
        s.lo[2 + 2 * k] ^= v[9 + k].z;
        s.hi[2 + 2 * k] ^= v[9 + k].w;
    }
    s.lo[15] ^= 1u;
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, d0, d1);
}

// The throughput leaf pass's window (k_reduce<LEAF, FAST>; the only form
// since round 3).  Block 1 (bytes 0..135) is loaded straight into
// the state registers, block 2 only after the first permutation, in two
// halves, so at most 16 data VGPRs are live beside the state; the thread's
// held digests live in its own LDS level slots (k_reduce), so the kernel
// fits MK_LEAF_SPLIT_WAVES waves per SIMD with 16 KB of LDS per workgroup.
// The 128-B line shared by both blocks is fetched twice when it leaves L2 in
// between (infinity-cache hit).  Against round 2's LDS-staged form (block 2
// parked in LDS through the first permutation: 1.04x fetch, 32 KB LDS): at
// 6 waves 0.4 % faster at 2^28, 1-2 % at 2^25 (profiles/r02zg/README.md), at
// 5 waves about 1 % more (below); the staged form was removed in round 3.
// 5 waves: 94 VGPRs and no spill, 0.8-1.7 % faster than 6 waves (80 VGPRs,
// 15 dwords in scratch) and 7 waves (54 spilled) slower still
// (profiles/r02zi, r02zj).
#define MK_LEAF_SPLIT_WAVES 5
__device__ __forceinline__ void hash_window256_split(const uint4* __restrict__ w, uint4& d0, uint4& d1) {
    State s;
    uint4 v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = ld_stream(w + k);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s.lo[2 * k] = v[k].x;
        s.hi[2 * k] = v[k].y;
        s.lo[2 * k + 1] = v[k].z;
        s.hi[2 * k + 1] = v[k].w;
    }
    s.lo[16] = v[8].x;
    s.hi[16] = v[8].y;
    const uint32_t t0 = v[8].z, t1 = v[8].w;
#pragma unroll
    for (int k = 17; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
    keccak_f(s);
    asm volatile("" ::: "memory");  // block 2 loads stay after the permutation
    s.lo[0] ^= t0;
    s.hi[0] ^= t1;
    {
        uint4 u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = ld_stream(w + 9 + k);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s.lo[1 + 2 * k] ^= u[k].x;
            s.hi[1 + 2 * k] ^= u[k].y;
            s.lo[2 + 2 * k] ^= u[k].z;
            s.hi[2 + 2 * k] ^= u[k].w;
        }
    }
    {
        uint4 u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = ld_stream(w + 13 + k);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.lo[9 + 2 * k] ^= u[k].x;
            s.hi[9 + 2 * k] ^= u[k].y;
            s.lo[10 + 2 * k] ^= u[k].z;
            s.hi[10 + 2 * k] ^= u[k].w;
        }
    }
    s.lo[15] ^= 1u;  // byte 256 = byte 120 of block 1
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, d0, d1);
}

// K(L || R) of two 32-B nodes with phase-locked rounds (the locked kernels).
__device__ __forceinline__ void hash_node_lock(uint4 l0, uint4 l1, uint4 r0, uint4 r1, uint4& d0, uint4& d1) {
    State s;
    s.lo[0] = l0.x; s.hi[0] = l0.y; s.lo[1] = l0.z; s.hi[1] = l0.w;
    s.lo[2] = l1.x; s.hi[2] = l1.y; s.lo[3] = l1.z; s.hi[3] = l1.w;
    s.lo[4] = r0.x; s.hi[4] = r0.y; s.lo[5] = r0.z; s.hi[5] = r0.w;
    s.lo[6] = r1.x; s.hi[6] = r1.y; s.lo[7] = r1.z; s.hi[7] = r1.w;
    // the pad (0x01 at byte 64, 0x80 at byte 135) and the zero lanes are
    // implied by the sparse round 0, which reads lanes 0..7 only
    keccak_f_digest_lock<kNodeMsg>(s);
    digest(s, d0, d1);
}

// Node-pass inputs (read once; a non-temporal load was tried and not kept)
__device__ __forceinline__ uint4 ld_node(const uint4* p) { return ld_stream(p); }

// ----------------------------------------------------------------------------
// First-level node j of a reduce pass.
//   LEAF: window j of the item buffer.
//   NODE: pair j of the 32-B input nodes (count cin).
template <bool LEAF>
__device__ __forceinline__ void first_level_generic(const ReduceArgs& a, uint64_t j, uint4& d0, uint4& d1) {
    if constexpr (LEAF) {
        if (j < a.c1_full) {  // full 256-B window (item_len | 128, 16-B aligned)
            hash_window256(reinterpret_cast<const uint4*>(a.items) + j * 16, d0, d1);
            return;
        }
        const uint64_t lo = j * 2 * a.cb;
        uint64_t la;
        uint32_t lz;
        if (2 * j + 1 < a.nchunks) {
            la = (lo + 2 * a.cb < a.total ? lo + 2 * a.cb : a.total) - lo;
            lz = 0;
        } else {
            la = a.total - lo;
            lz = 128;
        }
        sponge_generic(a.items + lo, la, lz, false, 0, d0, d1);
    } else {
        const uint4* in = reinterpret_cast<const uint4*>(a.items);
        const uint4 l0 = in[4 * j], l1 = in[4 * j + 1];
        if (a.cin == 1 && !a.pad_at_one) {  // single node: it is the root
            d0 = l0;
            d1 = l1;
            return;
        }
        const bool padded = !(2 * j + 1 < a.cin);
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
        if (!padded) {
            r0 = in[4 * j + 2];
            r1 = in[4 * j + 3];
        }
        hash_pair(l0, l1, r0, r1, padded, d0, d1);
    }
}

// Phase B of a fused pass (k_reduce, k_reduce_elem) after the workgroup's
// first two levels sit in LDS (m2 level-2 nodes, lds[2k], lds[2k+1]): the
// remaining levels in LDS, one node per thread per level (read -> barrier ->
// permute -> write -> barrier), then the workgroup's nodes (or, in the final
// pass, the root with the length mix-in) to HBM.
template <int NI>
__device__ __forceinline__ void reduce_levels_out(const ReduceArgs& a, uint4* lds, uint32_t tid, uint64_t lo1,
                                                  uint64_t c2, uint64_t m2, bool pair) {
    uint64_t c = c2, m = m2;
    int left = a.finalize ? 64 : (int)a.levels - (pair ? 2 : 1);
    int done = 0;
    while (left > 0 && (c > 1 || a.pad_at_one)) {
        const uint64_t mn = (m + 1) / 2;
        const bool act = tid < mn;
        uint4 l0, l1, r0 = make_uint4(0, 0, 0, 0), r1 = r0;
        bool padded = false;
        if (act) {
            l0 = lds[4 * tid];
            l1 = lds[4 * tid + 1];
            padded = !(2 * (uint64_t)tid + 1 < m);
            if (!padded) {
                r0 = lds[4 * tid + 2];
                r1 = lds[4 * tid + 3];
            }
        }
        __syncthreads();
        if (act) {
            uint4 d0, d1;
            hash_pair(l0, l1, r0, r1, padded, d0, d1);
            lds[2 * tid] = d0;
            lds[2 * tid + 1] = d1;
        }
        __syncthreads();
        c = (c + 1) / 2;
        m = mn;
        --left;
        ++done;
    }

    // ---- output ------------------------------------------------------------
    uint4* out = reinterpret_cast<uint4*>(a.out);
    if (a.finalize) {
        if (tid == 0) {
            uint4 d0, d1;
            hash_final(lds[0], lds[1], a.n_items, d0, d1);
            out[0] = d0;
            out[1] = d1;
        }
    } else {
        const uint64_t lo_out = (pair ? lo1 / 2 : lo1) >> done;  // the workgroup's first node of this level
        for (uint32_t k = tid; k < m; k += kReduceThreads) {
            out[2 * (lo_out + k)] = lds[2 * k];
            out[2 * (lo_out + k) + 1] = lds[2 * k + 1];
        }
    }
}

// One fused reduce pass.  256 threads; the workgroup owns first-level nodes
// [S*wg, S*wg+S) with S = 512*NI (NI = 2 for wide passes; NI = 1 halves the
// serial work per thread so mid-size trees still spread over all CUs),
// folds them pairwise in registers into S/2 level-2 nodes in LDS, then reduces further levels in LDS (one node per
// thread per level, read -> barrier -> permute -> write -> barrier).
// Non-final passes write 512 >> (levels-2) nodes per workgroup; the final
// pass (one workgroup) reduces to the root and applies the length mix-in.
template <bool LEAF, bool FAST, int NI>
__global__ __launch_bounds__(kReduceThreads, (LEAF && FAST) ? MK_LEAF_SPLIT_WAVES : MK_MIN_WAVES) void
k_reduce(ReduceArgs a) {
    constexpr uint64_t kSpan1 = 2 * NI * kReduceThreads;  // first-level nodes per workgroup
    constexpr uint64_t kSpan2 = kSpan1 / 2;
    constexpr bool kSplit = LEAF && FAST;  // the split window form (hash_window256_split)
    __shared__ uint4 lds[2 * kSpan2];
    const uint32_t tid = threadIdx.x;
    const uint64_t wg = a.wg_base + blockIdx.x;
    const uint64_t lo1 = wg * kSpan1;
    const uint64_t span1 = kSpan1;
    const uint64_t c1 = a.c1;
    const uint64_t m1 = (c1 - lo1) < span1 ? (c1 - lo1) : span1;
    const bool pair = a.levels >= 2 && (c1 > 1 || a.pad_at_one);
    const uint64_t c2 = pair ? (c1 + 1) / 2 : c1;
    const uint64_t m2 = pair ? (m1 + 1) / 2 : m1;

    // ---- phase A: first level (+ pair level) from global memory ----------
    if constexpr (kSplit) {
        // the left window's digest waits in the thread's own level slot (the
        // pair node overwrites it), so no digest is held across a window
#pragma unroll 1
        for (int i = 0; i < NI; ++i) {
            const uint32_t q = i * kReduceThreads + tid;
            const uint4* w = reinterpret_cast<const uint4*>(a.items) + (lo1 + 2 * (uint64_t)q) * 16;
            uint4 l0, l1, r0, r1, d0, d1;
            hash_window256_split(w, d0, d1);
            lds[2 * q] = d0;
            lds[2 * q + 1] = d1;
            hash_window256_split(w + 16, r0, r1);
            l0 = lds[2 * q];
            l1 = lds[2 * q + 1];
            hash_pair(l0, l1, r0, r1, false, d0, d1);
            lds[2 * q] = d0;
            lds[2 * q + 1] = d1;
        }
    } else if constexpr (FAST) {
        // Full workgroup of complete node pairs (host-checked): no bounds
        // checks, no odd padding, one keccak_f copy per call site.
#pragma unroll 1
        for (int i = 0; i < NI; ++i) {
            const uint32_t q = i * kReduceThreads + tid;
            const uint64_t j0 = lo1 + 2 * (uint64_t)q;
            uint4 l0, l1, r0, r1, d0, d1;
            const uint4* in = reinterpret_cast<const uint4*>(a.items) + j0 * 4;
            hash_pair(ld_node(in), ld_node(in + 1), ld_node(in + 2), ld_node(in + 3), false, l0, l1);
            hash_pair(ld_node(in + 4), ld_node(in + 5), ld_node(in + 6), ld_node(in + 7), false, r0, r1);
            hash_pair(l0, l1, r0, r1, false, d0, d1);
            lds[2 * q] = d0;
            lds[2 * q + 1] = d1;
        }
    } else if (pair) {
#pragma unroll 1
        for (int i = 0; i < NI; ++i) {
            const uint32_t q = i * kReduceThreads + tid;
            if (q < m2) {
                const uint64_t j0 = lo1 + 2 * (uint64_t)q;
                uint4 l0, l1, r0 = make_uint4(0, 0, 0, 0), r1 = r0, d0, d1;
                first_level_generic<LEAF>(a, j0, l0, l1);
                const bool padded = !(2 * (uint64_t)q + 1 < m1);
                if (!padded) first_level_generic<LEAF>(a, j0 + 1, r0, r1);
                hash_pair(l0, l1, r0, r1, padded, d0, d1);
                lds[2 * q] = d0;
                lds[2 * q + 1] = d1;
            }
        }
    } else {
        // no pair level (levels == 1, or a single first-level node); the host
        // guarantees m1 <= kSpan2 here.
#pragma unroll 1
        for (int i = 0; i < NI; ++i) {
            const uint32_t q = i * kReduceThreads + tid;
            if (q < m1) {
                uint4 d0, d1;
                first_level_generic<LEAF>(a, lo1 + q, d0, d1);
                lds[2 * q] = d0;
                lds[2 * q + 1] = d1;
            }
        }
    }
    __syncthreads();

    reduce_levels_out<NI>(a, lds, tid, lo1, c2, m2, pair);
}

// ----------------------------------------------------------------------------
// Phase-locked leaf pass (MK_LEAF_LOCK): 1024 threads, one workgroup per CU,
// so the 4 waves of each SIMD belong to one workgroup and the s_barrier in
// every Keccak round (round_asm<true>, keccak_dev.hpp) keeps them on the same
// instruction: the round issues at ~2.8 cycles per wave instruction instead of
// the ~3.5 of free-running waves.  Every thread hashes 4
// consecutive full windows, folds them in registers into one node three
// levels above the chunks (4 x 2 + 2 + 1 = 11 permutations, all locked) and
// writes it: workgroup g covers windows [4096 g, 4096 g + 4096) of the pass,
// i.e. the spans of k_reduce workgroups 4g..4g+3 run with a.levels == 3, and
// writes their output nodes [1024 g, 1024 g + 1024).  No divergence: every
// wave runs the same number of barriers (the host launches only full
// workgroups of full windows).  The windows are staged in LDS by COALESCED
// DMA (global_load_lds_dwordx4: no VGPRs held while a load is in flight) on a
// persistent grid.  With direct per-lane loads (round 3's k_leaf_lock, 2^28
// leaf pass 8.54 vs 8.25 ms, profiles/r03i/ab_lock4_28.jsonl; removed in
// round 4) every wave waits for its window loads, and a locked workgroup has
// no other workgroup on its CU to cover the wait;
// its per-lane 16-B loads of lanes 1 KB apart also touch 64 lines per
// instruction and every line 8 times.  Here phase A of window j (units
// 0..8 = block 1) lands in the wave's LDS (10 KB per wave) during the
// previous window's second permutation and phase B (units 9..15) during this
// window's first.  The 16-B units of a step are flattened window-major
// (phase A: U = 9 m + u; phase B: U = 7 m + u - 9), so consecutive lanes of a
// DMA instruction read consecutive units of one window (~15 lines per
// instruction, each line once), and the LDS image is that flat order: lane m
// reads its unit u at row 9 m + u (or 7 m + u - 9) -- an odd stride, so the
// 16-B reads of any 16 consecutive lanes hit distinct bank quads.
// The window's line 0 (units 0..7) and block 2
// (units 9..15, their last use) are fetched non-temporally, so they do not
// push line 1 out of L2 between block 1's unit 8 and block 2.  Phase A is
// then 9 instructions of line-0 units in a stride-9 image (the 9th position
// repeats unit 7) plus one of unit 8 into rows 576..639 (160 KB of LDS).
// One process, 2^28 (profiles/r03q): fetch 12.14 -> 8.89 GB per leaf pass
// (1.41x -> 1.03x the algorithmic 8.59 GB), leaf pass 8.138 -> 8.071 ms.
// The DMA of each phase in three parts spread over a permutation instead of
// one burst (the C5 front's finding): phase B (the window's
// second block) 3 + 2 + 2 instructions before round 0 and after rounds B1,
// B2 of the first permutation; phase A (the next window's first block) 3 +
// 3 + 3 (+1) after rounds A1, A2 and MK_LOCK_DMA_ROUND of the second.  One
// process A/B (profiles/r05/leaf_dma_split/, 7-9 interleaved rounds, two
// boxes): 2^28 tree -0.6..-0.8 % (leaf pass 7.943 -> 7.885 ms at 2/8/14),
// 2^25 -2.6 % against one burst each (round 4's form).
#define MK_LOCK_SPLIT_B1 4
#define MK_LOCK_SPLIT_B2 8
#define MK_LOCK_SPLIT_A1 2
#define MK_LOCK_SPLIT_A2 8
constexpr int kLockAux = 2;  // global_load_lds aux: nt
// the side configs' locked kernels (C2 messages, C3 records): inputs read once, default policy (nt not kept)
constexpr int kSideAux = 0;
//
// Staging addresses.  Instruction i of a phase moves flat units U = 64 i +
// lane, unit u = U mod NU of window m = U / NU (NU = 9 or 7), from byte
// 1024 m + 16 u of the wave's region.  Both NU divide 63, so from one
// instruction to the next (m, u) -> (m + 63 / NU, u + 1) with one wrap, and
// instruction i is the lane's own (m0, u0) of instruction 0 plus a constant,
// plus 1024 - 16 NU on the lanes that have wrapped by then.  Which lanes
// those are is a compile-time lane set (lane mod NU >= NU - i): an SGPR-pair
// constant selects on it, so there is no division (v_mul_hi_u32, shifts, a
// multiply back) and no compare.  The lane's two byte offsets at instruction
// 0 (phase A in the low half, phase B in the high half) are one VGPR for the
// whole kernel (lock_dma_seed), laundered at every call so that nothing
// larger is hoisted; the constant goes into the wave-uniform base, and the
// instruction takes that base in SGPRs with the 32-bit lane offset (no
// 64-bit per-lane add).  Per DMA instruction 2 VALU (phase B) or 3 (phase A,
// whose position 8 repeats unit 7), all full rate, against 11 with a
// quarter-rate v_mul_hi_u32 and four 64-bit adds before
// (profiles/r07/leaf_nonround_valu.md).
__device__ __forceinline__ uint32_t lock_dma_seed(uint32_t lane) {
    const uint32_t m9 = lane / 9, u9 = lane - 9 * m9, m7 = lane / 7, u7 = lane - 7 * m7;
    return (1024 * m9 + 16 * u9) | (1024 * m7 + 16 * u7) << 16;
}
// lanes whose unit has wrapped into the next window by instruction i / sits at position NU - 1 there
template <int NU>
constexpr uint64_t lock_lanes_wrapped(int i) {
    uint64_t s = 0;
    for (int l = 0; l < 64; ++l) s |= (uint64_t)(l % NU + i >= NU) << l;
    return s;
}
template <int NU>
constexpr uint64_t lock_lanes_last(int i) {
    uint64_t s = 0;
    for (int l = 0; l < 64; ++l) s |= (uint64_t)((l + 64 * i) % NU == NU - 1) << l;
    return s;
}
// lanes of the set ? b : 0
__device__ __forceinline__ uint32_t lock_sel0(uint32_t b, uint64_t lanes) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(b), "s"(lanes));
    return r;
}
// lanes of the set ? b : A (A, an inline constant)
template <int A>
__device__ __forceinline__ uint32_t lock_sel_else(uint32_t b, uint64_t lanes) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "n"(A), "v"(b), "s"(lanes));
    return r;
}
// lanes of the set ? 0 : a
__device__ __forceinline__ uint32_t lock_clear(uint32_t a, uint64_t lanes) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, 0, %2" : "=v"(r) : "v"(a), "s"(lanes));
    return r;
}
// lanes of the set ? 0 : A
template <int A>
__device__ __forceinline__ uint32_t lock_clear_imm(uint64_t lanes) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, 0, %2" : "=v"(r) : "n"(A), "s"(lanes));
    return r;
}
// 16 B per lane from `base` (wave-uniform, kept in SGPRs) + off into row..row + 63 of the wave's image
template <int AUX>
__device__ __forceinline__ void lock_dma_issue(uint4* row, const uint4* base, uint32_t off) {
    asm("" : "+s"(base));  // the constant part stays in the scalar base
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(reinterpret_cast<const char*>(base) + off),
                                     (__attribute__((address_space(3))) void*)row, 16, 0, AUX);
}
// instructions [I0, I1) of the NU (a part of a split issue); Rj, Bw wave-uniform
template <int NU, int U0, int AUX = 0, int I0 = 0, int I1 = NU>
__device__ __forceinline__ void lock_dma_c(uint4* Bw, const uint4* __restrict__ Rj, uint32_t seed) {
    static_assert(NU == 7 && 63 % NU == 0, "the seed's high half is the stride-7 image");
    asm volatile("" : "+v"(seed));
    const uint32_t off0 = seed >> 16;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
        const uint32_t off = i ? off0 + lock_sel0(1024u - 16u * NU, lock_lanes_wrapped<NU>(i)) : off0;
        lock_dma_issue<AUX>(Bw + 64 * i, Rj + (63 / NU) * 64 * i + i + U0, off);
    }
}
// phase A of a window step (block 1 = units 0..8); instructions [I0, I1) of
// the 9 (+ the unit-8 copy with the last part)
template <int I0 = 0, int I1 = 9>
__device__ __forceinline__ void lock_dma_a(uint4* Bw, const uint4* __restrict__ Rj, uint32_t seed, uint32_t lane) {
    asm volatile("" : "+v"(seed));
    const uint32_t off0 = seed & 0xFFFFu;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
        // position 8 repeats unit 7: those lanes step back one unit.  The
        // lane offset is unsigned (lane 0 at i = 8 would go below zero), so
        // the base is one unit low and every other lane adds the unit back:
        // at i = 0 the base is Rj - 1, which for the first wave of the first
        // group lies 16 B below the items, but no lane reads below Rj -- a
        // lane adds 16, or is at position 8 with off0 >= 128.
        const uint32_t d = i ? lock_clear(lock_sel_else<16>(1024u - 16u * 9 + 16u, lock_lanes_wrapped<9>(i)),
                                          lock_lanes_last<9>(i))
                             : lock_clear_imm<16>(lock_lanes_last<9>(i));
        lock_dma_issue<kLockAux>(Bw + 64 * i, Rj + 7 * 64 * i + i - 1, off0 + d);
    }
    if constexpr (I1 == 9) {
        asm volatile("" : "+v"(lane));  // lane << 10 recomputed here as a 32-bit offset, not held as a 64-bit pair
        lock_dma_issue<0>(Bw + 576, Rj + 8, lane << 10);
    }
}

// `after_wait` runs right after phase A's wait: the previous group's output
// store goes there, so no wait ever covers a store issued just before it
// (stores count in vmcnt; a store's wait is the write's round trip).
template <typename F>
__device__ __forceinline__ void hash_window_sc(uint4* Bw, uint32_t lane, uint32_t seed, const uint4* __restrict__ Rj,
                                               const uint4* __restrict__ Rnext, uint4& d0, uint4& d1,
                                               F&& after_wait) {
    State s;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // phase A has landed
    after_wait();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 v = Bw[9 * lane + k];
        s.lo[2 * k] = v.x;
        s.hi[2 * k] = v.y;
        s.lo[2 * k + 1] = v.z;
        s.hi[2 * k + 1] = v.w;
    }
    const uint4 v8 = Bw[576 + lane];
    s.lo[16] = v8.x;
    s.hi[16] = v8.y;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // rows read: phase B may overwrite them
    lock_dma_c<7, 9, kLockAux, 0, 3>(Bw, Rj, seed);  // phase B in three parts over the first permutation
    // lanes 17..24 start at zero: the sparse round 0 reads lanes 0..16 only
    keccak_f_lock_mid2<MK_LOCK_SPLIT_B1, MK_LOCK_SPLIT_B2, kBlock17>(
        s, [&] { lock_dma_c<7, 9, kLockAux, 3, 5>(Bw, Rj, seed); },
        [&] { lock_dma_c<7, 9, kLockAux, 5, 7>(Bw, Rj, seed); });
    s.lo[0] ^= v8.z;
    s.hi[0] ^= v8.w;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // phase B has landed
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const uint4 u = Bw[7 * lane + k];
        s.lo[1 + 2 * k] ^= u.x;
        s.hi[1 + 2 * k] ^= u.y;
        s.lo[2 + 2 * k] ^= u.z;
        s.hi[2 + 2 * k] ^= u.w;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    s.lo[15] ^= 1u;
    s.hi[16] ^= 0x80000000u;
    // the next window's block 1 goes out MK_LOCK_DMA_ROUND rounds into this
    // permutation: late enough that little of the data streamed in between
    // evicts the line block 2 shares with it, early enough to land in time
    keccak_f_digest_lock_mid3<MK_LOCK_SPLIT_A1, MK_LOCK_SPLIT_A2, MK_LOCK_DMA_ROUND>(  // in three parts
        s, [&] { if (Rnext) lock_dma_a<0, 3>(Bw, Rnext, seed, lane); },
        [&] { if (Rnext) lock_dma_a<3, 6>(Bw, Rnext, seed, lane); },
        [&] { if (Rnext) lock_dma_a<6, 9>(Bw, Rnext, seed, lane); });
    digest(s, d0, d1);
}

#if MK_TOP_STAMPS
// diagnostic build only (tools/top_probe.hip): s_memrealtime at the start and
// the end of each workgroup of the leaf pass
__device__ uint64_t g_leaf_stamps[2 * 1024];
#endif
__global__ __launch_bounds__(kLockThreads, 1) void k_leaf_lock_sc(ReduceArgs a, uint64_t ngroups) {
#if MK_TOP_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_leaf_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
    __shared__ uint4 buf[kLockThreads / 64][10 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    // the wave index through readfirstlane: the region bases and the LDS image are then scalar values
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t seed = lock_dma_seed(lane);
    uint4* Bw = buf[wave];
    const uint4* items = reinterpret_cast<const uint4*>(a.items);
    uint4* out = reinterpret_cast<uint4*>(a.out);
    // the wave's 64 nodes = 256 consecutive windows (64 KB); lane m's windows at m * 64 uint4
    auto region = [&](uint64_t g) { return items + (g * kLockThreads + 64 * wave) * 64; };
    uint64_t g = blockIdx.x;
    if (g < ngroups) lock_dma_a(Bw, region(g), seed, lane);
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;  // the previous group's node, stored one group late
    uint64_t qnode = 0;
    bool pend = false;
    auto flush = [&] {
        if (pend) {
            out[2 * qnode] = q0;
            out[2 * qnode + 1] = q1;
        }
    };
    auto none = [] {};
#pragma unroll 1
    for (; g < ngroups; g += gridDim.x) {
        const uint4* R = region(g);
        const uint64_t gn = g + gridDim.x;
        const uint4* Rn = gn < ngroups ? region(gn) : nullptr;
        uint4 l0, l1, r0, r1, p0, p1;
        hash_window_sc(Bw, lane, seed, R, R + 16, l0, l1, flush);
        hash_window_sc(Bw, lane, seed, R + 16, R + 32, r0, r1, none);
        hash_node_lock(l0, l1, r0, r1, p0, p1);
        hash_window_sc(Bw, lane, seed, R + 32, R + 48, l0, l1, none);
        hash_window_sc(Bw, lane, seed, R + 48, Rn, r0, r1, none);
        hash_node_lock(l0, l1, r0, r1, l0, l1);
        hash_node_lock(p0, p1, l0, l1, q0, q1);
        qnode = g * kLockThreads + threadIdx.x;
        pend = true;
    }
    flush();
#if MK_TOP_STAMPS
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_leaf_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
#endif
}

template __global__ void k_reduce<true, true, 2>(ReduceArgs);
template __global__ void k_reduce<true, false, 2>(ReduceArgs);
template __global__ void k_reduce<false, true, 2>(ReduceArgs);
template __global__ void k_reduce<false, false, 2>(ReduceArgs);
template __global__ void k_reduce<true, true, 1>(ReduceArgs);
template __global__ void k_reduce<true, false, 1>(ReduceArgs);

// ----------------------------------------------------------------------------
// ssz.TreeHash of a list of byte strings in one pass (makeSliceHasher over
// []byte / [N]byte elements, hash.go:118-139 with hashedEncoding,
// hash.go:100-107): the tree's items are the element digests
// K(le32(elem_len) || element), 32 B each, 4 per chunk, so a level-1 window is
// the 8 digests of 8 consecutive elements.  k_reduce_elem computes those
// digests in registers and goes straight on into the window, the pair level
// and the LDS levels -- no n x 32-B digest array in HBM.

// Full window of 8 elements of 32 B (256 contiguous bytes, 16-B aligned).
// Two Keccak states cannot be live at once within 128 VGPRs (a permutation
// alone takes ~80), so digests 4..7 -- the last 8 bytes of block 1 and all of
// block 2 of the window message -- are parked in this thread's LDS column
// (stg[k * kReduceThreads], dword-major across the workgroup: conflict-free),
// digests 0..3 stay in registers as block 1, and the window absorbs block 2
// from LDS after its first permutation.
__device__ __forceinline__ void elem_window32(const uint4* __restrict__ w, uint32_t* stg, uint4& o0, uint4& o1) {
#pragma unroll
    for (int e = 4; e < 8; ++e) {
        uint32_t d[8];
        elem32_digest(w + 2 * e, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) stg[(8 * (e - 4) + k) * kReduceThreads] = d[k];
    }
    uint32_t m[32];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t d[8];
        elem32_digest(w + 2 * e, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) m[8 * e + k] = d[k];
    }
    State s;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        s.lo[k] = m[2 * k];
        s.hi[k] = m[2 * k + 1];
    }
    s.lo[16] = stg[0];
    s.hi[16] = stg[kReduceThreads];
#pragma unroll
    for (int k = 17; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
    keccak_f(s);
#pragma unroll
    for (int q = 0; q < 30; ++q) {  // block 2 = staged dwords 2..31
        const uint32_t v = stg[(2 + q) * kReduceThreads];
        if (q & 1)
            s.hi[q >> 1] ^= v;
        else
            s.lo[q >> 1] ^= v;
    }
    s.lo[15] ^= 1u;  // byte 256 = byte 120 of block 2
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, o0, o1);
}

// Window j of the digest tree in general form: digests [8j, min(8j+8, n)),
// odd chunk count -> the 128-B zero chunk appended (hash.go:225-228).
__device__ __noinline__ void elem_window_generic(const ReduceArgs& a, uint64_t j, uint4& o0, uint4& o1) {
    const uint64_t n = a.n_items;
    const uint32_t cnt = (uint32_t)((n - 8 * j) < 8 ? (n - 8 * j) : 8);
    const bool padded = !(2 * j + 1 < a.nchunks);
    const uint32_t L = a.elem_len;
    uint32_t m[64];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if ((uint32_t)e < cnt) elem_digest_any(a.items + (8 * j + e) * (uint64_t)L, L, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) m[8 * e + k] = d[k];
    }
    const uint32_t lm = 32 * cnt + (padded ? 128u : 0u);  // message bytes (<= 256, a multiple of 4)
    const uint32_t nb = lm / 136 + 1;
    State s;
    zero(s);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if ((uint32_t)b >= nb) break;
#pragma unroll
        for (int w = 0; w < 34; ++w) {
            const int q = 34 * b + w;
            uint32_t v = q < 64 ? m[q] : 0u;
            if ((uint32_t)q * 4 == lm) v ^= 1u;
            if ((uint32_t)b == nb - 1 && w == 33) v ^= 0x80000000u;
            if (w & 1)
                s.hi[w >> 1] ^= v;
            else
                s.lo[w >> 1] ^= v;
        }
        if ((uint32_t)b + 1 < nb)
            keccak_f(s);
        else
            keccak_f_digest(s);
    }
    digest(s, o0, o1);
}

#define MK_ELEM_WAVES 4
// The leaf pass of the element-digest tree (a.n_items elements, a.nchunks =
// ceil(n / 4) chunks, a.c1 windows), one window pair per thread (NI = 1:
// 512 windows = 4096 elements per workgroup; LDS 8 KB of levels + 32 KB of
// staged digests, so 4 workgroups of 4 waves fill a CU's 160 KB at 4
// waves/SIMD).  FAST: every window of the workgroup has 8 elements of 32 B,
// 16-B aligned (host-checked).  Otherwise the general window (any elem_len
// and alignment, ragged last window, odd pad).
template <bool FAST>
__global__ __launch_bounds__(kReduceThreads, FAST ? MK_ELEM_WAVES : 1) void k_reduce_elem(ReduceArgs a) {
    constexpr int NI = 1;
    constexpr uint64_t kSpan1 = 2 * NI * kReduceThreads;
    constexpr uint64_t kSpan2 = kSpan1 / 2;
    __shared__ uint4 lds[2 * kSpan2];
    __shared__ uint32_t stg[FAST ? 32 * kReduceThreads : 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t wg = a.wg_base + blockIdx.x;
    const uint64_t lo1 = wg * kSpan1;
    const uint64_t c1 = a.c1;
    const uint64_t m1 = (c1 - lo1) < kSpan1 ? (c1 - lo1) : kSpan1;
    const bool pair = a.levels >= 2 && c1 > 1;  // the host plans k_reduce_elem for trees of > 2^17 windows
    const uint64_t c2 = pair ? (c1 + 1) / 2 : c1;
    const uint64_t m2 = pair ? (m1 + 1) / 2 : m1;
    const uint32_t q = tid;
    if (FAST || q < m2) {
        const uint64_t j0 = lo1 + 2 * (uint64_t)q;
        uint4 l0, l1, r0 = make_uint4(0, 0, 0, 0), r1 = r0, d0, d1;
        bool padded = false;
        if constexpr (FAST) {
            const uint4* w = reinterpret_cast<const uint4*>(a.items) + j0 * 16;
            elem_window32(w, stg + tid, d0, d1);
            lds[2 * q] = d0;  // the left digest waits in this thread's own level slot
            lds[2 * q + 1] = d1;
            elem_window32(w + 16, stg + tid, r0, r1);
            l0 = lds[2 * q];
            l1 = lds[2 * q + 1];
        } else {
            elem_window_generic(a, j0, l0, l1);
            padded = !(2 * (uint64_t)q + 1 < m1);
            if (!padded) elem_window_generic(a, j0 + 1, r0, r1);
        }
        hash_pair(l0, l1, r0, r1, padded, d0, d1);
        lds[2 * q] = d0;
        lds[2 * q + 1] = d1;
    }
    __syncthreads();
    reduce_levels_out<NI>(a, lds, tid, lo1, c2, m2, pair);
}

template __global__ void k_reduce_elem<true>(ReduceArgs);

// Phase-locked element windows (C4 secondary, TreeHash of
// [][32]byte): lane m of wave w hashes window g * 1024 + 64 w + m of group g
// -- its 8 element digests K(le32(32) || e) (1 permutation each) and the
// window K(d0 || .. || d7) (2) -- with phase-locked permutations and writes
// the window digest (a level-1 node of the tree; the host finishes the tree
// from those nodes).  n windows in all; a partial last group's lanes past n
// hash copies of window n - 1 and store nothing.  The window's two halves
// (elements 0..3, 4..7: 128 B = 8 units each) are staged in the wave's 9 KB
// of LDS by coalesced non-temporal DMA in a stride-9 image (the 9th
// position repeats unit 7); digests 0..3 wait in VGPRs, digests 4..7 replace
// their elements in LDS, and the next window's first half goes out once
// block 2 of this window's message has been read.
__device__ __forceinline__ void elem_dma_half(uint4* Bw, const uint4* __restrict__ W0, uint64_t m0, uint64_t nwin,
                                              int half, uint32_t lane) {
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const uint32_t U = 64u * i + lane;
        const uint32_t m = U / 9, u = U - m * 9;
        const uint64_t win = m0 + m < nwin ? m0 + m : nwin - 1;
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(W0 + win * 16 + 8 * half + (u < 8 ? u : 7)),
                                         (__attribute__((address_space(3))) void*)(Bw + 64 * i), 16, 0, kLockAux);
    }
}
__device__ __forceinline__ void elem_digest_lock(uint4 a, uint4 b, uint32_t (&d)[8]) {
    State s;
    s.lo[0] = 32u;  // le32(len)
    s.hi[0] = a.x;
    s.lo[1] = a.y;
    s.hi[1] = a.z;
    s.lo[2] = a.w;
    s.hi[2] = b.x;
    s.lo[3] = b.y;
    s.hi[3] = b.z;
    s.lo[4] = b.w;
    s.hi[4] = 1u;  // domain pad at byte 36
#pragma unroll
    for (int k = 5; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
    s.hi[16] = 0x80000000u;
    keccak_f_digest_lock(s);
    d[0] = s.lo[0]; d[1] = s.hi[0]; d[2] = s.lo[1]; d[3] = s.hi[1];
    d[4] = s.lo[2]; d[5] = s.hi[2]; d[6] = s.lo[3]; d[7] = s.hi[3];
}
__global__ __launch_bounds__(kLockThreads, 1) void k_elem_lock(const uint4* __restrict__ elems, uint64_t nwin,
                                                               uint4* __restrict__ out) {
    __shared__ uint4 buf[kLockThreads / 64][9 * 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* Bw = buf[wave];
    const uint4* Rl = Bw + 9 * lane;  // this lane's 8 staged units (+1 repeat)
    const uint64_t ngroups = (nwin + kLockThreads - 1) / kLockThreads;
    uint64_t g = blockIdx.x;
    if (g < ngroups) elem_dma_half(Bw, elems, g * kLockThreads + 64 * wave, nwin, 0, lane);
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    uint64_t qi = 0;
    bool pend = false;
#pragma unroll 1
    for (; g < ngroups; g += gridDim.x) {
        const uint64_t m0 = g * kLockThreads + 64 * wave;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first half landed
        if (pend && qi < nwin) {
            out[2 * qi] = q0;
            out[2 * qi + 1] = q1;
        }
        uint32_t dlo[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 a = Rl[2 * k], b = Rl[2 * k + 1];
            if (k == 3) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // first half read: the second may land
                elem_dma_half(Bw, elems, m0, nwin, 1, lane);
            }
            elem_digest_lock(a, b, dlo[k]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // second half landed
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 a = Rl[2 * k], b = Rl[2 * k + 1];
            uint32_t d[8];
            elem_digest_lock(a, b, d);
            // digest 4 + k replaces element 4 + k (same 32 B, already absorbed)
            uint4* R = Bw + 9 * lane;
            R[2 * k] = make_uint4(d[0], d[1], d[2], d[3]);
            R[2 * k + 1] = make_uint4(d[4], d[5], d[6], d[7]);
        }
        // the window message d0..d7 (256 B): block 1 = d0..d3 + the first 8 B of d4
        State s;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                s.lo[4 * k + w] = dlo[k][2 * w];
                s.hi[4 * k + w] = dlo[k][2 * w + 1];
            }
        const uint4 t4a = Rl[0];
        s.lo[16] = t4a.x;
        s.hi[16] = t4a.y;
#pragma unroll
        for (int k = 17; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
        keccak_f_lock(s);
        // block 2 = d4[8..32) + d5 + d6 + d7 + padding at byte 256 = byte 120
        s.lo[0] ^= t4a.z;
        s.hi[0] ^= t4a.w;
        {
            const uint4 t = Rl[1];
            s.lo[1] ^= t.x; s.hi[1] ^= t.y; s.lo[2] ^= t.z; s.hi[2] ^= t.w;
        }
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const uint4 a = Rl[2 * k], b = Rl[2 * k + 1];
            s.lo[4 * k - 1] ^= a.x; s.hi[4 * k - 1] ^= a.y; s.lo[4 * k] ^= a.z; s.hi[4 * k] ^= a.w;
            s.lo[4 * k + 1] ^= b.x; s.hi[4 * k + 1] ^= b.y; s.lo[4 * k + 2] ^= b.z; s.hi[4 * k + 2] ^= b.w;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // digests read: the next window's first half may land
        if (g + gridDim.x < ngroups)
            elem_dma_half(Bw, elems, (g + gridDim.x) * kLockThreads + 64 * wave, nwin, 0, lane);
        s.lo[15] ^= 1u;  // byte 256 = byte 120 of block 2
        s.hi[16] ^= 0x80000000u;
        keccak_f_digest_lock(s);
        digest(s, q0, q1);
        qi = g * kLockThreads + threadIdx.x;
        pend = true;
    }
    if (pend && qi < nwin) {
        out[2 * qi] = q0;
        out[2 * qi + 1] = q1;
    }
}


template __global__ void k_reduce_elem<false>(ReduceArgs);

// Element digests K(le32(elem_len) || element i) -> out[i] (32 B): the first
// half of the two-phase form, for trees too small for k_reduce_elem's
// throughput pass and for element lengths other than 32.
// FAST32: 32-B elements at a 16-B aligned base (one block, 16-B loads);
// otherwise any length and alignment (the general sponge, its own kernel so
// the fast form keeps its few VGPRs).
template <bool FAST32>
__global__ __launch_bounds__(256) void k_elem_digests(const uint8_t* __restrict__ elems, uint64_t n, uint32_t elem_len,
                                                      uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8];
    if constexpr (FAST32)
        elem32_digest(reinterpret_cast<const uint4*>(elems) + 2 * i, d);
    else
        elem_digest_any(elems + i * (uint64_t)elem_len, elem_len, d);
    out[2 * i] = make_uint4(d[0], d[1], d[2], d[3]);
    out[2 * i + 1] = make_uint4(d[4], d[5], d[6], d[7]);
}
template __global__ void k_elem_digests<true>(const uint8_t*, uint64_t, uint32_t, uint4*);
template __global__ void k_elem_digests<false>(const uint8_t*, uint64_t, uint32_t, uint4*);


// ----------------------------------------------------------------------------
// Node pass of the latency form with BIT-INTERLEAVED lane pairs
// (keccak_dev.hpp, mk::ilv): lane p of pair k owns the parity-p words of node
// k.  Nodes in LDS and, between consecutive wave3 passes, in HBM stay in
// that form ("ilv nodes": dword 2w + p = parity-p word of digest lane w);
// a.in_ilv / a.out_ilv select conversion from / to plain 32-B digests at the
// pass boundary, so a chain of passes converts once at each end.
// NT = 64..1024 threads own NT/2 lane pairs and reduce them through
// log2(NT/2) more levels in LDS.  The host picks NT so the first level's
// workgroups spread over all 256 CUs (NT = 1024 for 2^17 pairs): the first,
// throughput-bound level fills the chip, and each later level halves the
// number of waves that still issue (waves with no active lane skip the
// permutation and wait at the barrier), so one launch covers up to 10 levels
// at close to one permutation latency each.
// Levels of k_wave3 once a level has at most one parent per wave: ONE
// STATE PER WAVE (mk::spread, ilv words, ~6.4 k cycles per lone-wave
// permutation against ~12.8 k for a lane pair).  Wave w hashes parent w; the
// nodes stay in k_wave3's LDS layout (lds[8 node + 2 word + parity]).  GPU
// lane L holds Keccak lane i = lane_consts(L).i: i < 4 the left node's word
// i, 4..7 the right node's, 8 / 16 (3 / 16 in the second block of a padded
// node) the padding bits.
template <uint32_t NT>
__device__ __forceinline__ void wave3_spread_levels(uint32_t* lds, uint64_t& c, uint64_t& m, int& left, int& done,
                                                    uint32_t pad_at_one) {
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    const spread::Lane cst = spread::lane_consts(L);
    const uint32_t i = cst.i;
    while (left > 0 && (c > 1 || pad_at_one)) {
        const uint64_t mn = (m + 1) / 2;
        uint32_t e = 0u, o = 0u;
        if (w < mn) {  // wave-uniform
            const bool padded = !(2 * (uint64_t)w + 1 < m);
            if (i < 4u) {
                e = lds[16 * w + 2 * i];
                o = lds[16 * w + 2 * i + 1];
            } else if (i < 8u && !padded) {
                e = lds[16 * w + 8 + 2 * (i - 4u)];
                o = lds[16 * w + 8 + 2 * (i - 4u) + 1];
            }
            if (padded) {  // K(l || 0^128): 160 bytes, two blocks
                spread::keccak_f(e, o, cst);
                if (i == 3u) e ^= 1u;
            } else if (i == 8u) {
                e ^= 1u;
            }
            if (i == 16u) o ^= 0x80000000u;
            spread::keccak_f(e, o, cst);
        }
        __syncthreads();
        if (w < mn && L < 4u) {
            lds[8 * w + 2 * L] = e;
            lds[8 * w + 2 * L + 1] = o;
        }
        __syncthreads();
        c = (c + 1) / 2;
        m = mn;
        --left;
        ++done;
    }
}

// K(root || le64(n) || 0^24) by wave 0 in spread form; plain digest to out.
// With `pair` (a two-field struct root, hash.go:141-159: the State{registry,
// balances} of BASELINE config 3): out is this field's slot of the pair
// block, and the second of the two finishers to arrive -- they run as
// separate launches on two streams, neither waits for the other -- hashes
// K(slot 0 || slot 1) into pair[64..96).  Arrival word pair[24] = epoch << 2 |
// arrived-slot bits (epochs are 30-bit and wrap; "newer" = ahead by less than
// 2^29): a finisher of a newer epoch than the word's starts the mask afresh,
// so a pair left half-done (a failed launch) cannot pair with the next one; a
// finisher of an OLDER epoch (a late one) is ignored -- it writes neither its
// slot nor the arrival word -- so it cannot clear the current pair's bits.
// Best-effort: the epoch is read before the slot store, so a finisher that
// falls behind while it runs may still overwrite its slot; callers never run
// two epochs' finishers of one slot concurrently (include/prysm_merkle.h).  The first finisher of an epoch zeroes pair[64..96)
// before it sets its bit, so a pair that never completes reads back as
// zeros, never as the previous epoch's root.
// How far `epoch` is ahead of an arrival word's epoch (mod 2^30; >= 2^29:
// behind).  A word whose epoch is 0 was never used (valid epochs are >= 1):
// every epoch is ahead of it.
__device__ __forceinline__ uint32_t epoch_ahead(uint32_t epoch, uint32_t word) {
    return (word >> 2) == 0u ? 1u : (epoch - (word >> 2)) & 0x3FFFFFFFu;
}
__device__ __forceinline__ void spread_store_digest(uint32_t e, uint32_t o, uint32_t L, uint32_t* out) {
    if (L < 4u) {
        out[2 * L] = ilv::spread16(e) | (ilv::spread16(o) << 1);
        out[2 * L + 1] = ilv::spread16(e >> 16) | (ilv::spread16(o >> 16) << 1);
    }
}
__device__ __forceinline__ void wave3_spread_final(const uint32_t* lds, uint64_t n_items, uint32_t* out,
                                                   uint32_t* pair = nullptr, uint32_t slot = 0, uint32_t epoch = 0) {
    const uint32_t L = threadIdx.x & 63u;
    const spread::Lane cst = spread::lane_consts(L);
    const uint32_t i = cst.i;
    uint32_t e = 0u, o = 0u;
    if (i < 4u) {
        e = lds[2 * i];
        o = lds[2 * i + 1];
    } else if (i == 4u) {
        e = ilv::to_ilv((uint32_t)n_items, (uint32_t)(n_items >> 32), 0);
        o = ilv::to_ilv((uint32_t)n_items, (uint32_t)(n_items >> 32), 1);
    } else if (i == 8u) {
        e = 1u;
    }
    if (i == 16u) o ^= 0x80000000u;
    spread::keccak_f(e, o, cst);
    if (pair) {  // a late finisher of an older epoch than the word's leaves the block alone
        uint32_t stale = 0;
        if (L == 0) stale = epoch_ahead(epoch, atomicAdd(pair + 24, 0u)) >= (1u << 29);
        if (__shfl(stale, 0)) return;
    }
    spread_store_digest(e, o, L, out);
    if (!pair) return;
    __threadfence();  // this field's root is visible before its arrival bit
    uint32_t second = 0;
    if (L == 0) {
        uint32_t* word = pair + 24;
        uint32_t old = atomicAdd(word, 0u);  // an atomic read of the arrival word
        for (;;) {
            const uint32_t ahead = epoch_ahead(epoch, old);
            if (ahead >= (1u << 29)) break;  // an older epoch than the word's: a late finisher, ignored
            if (ahead != 0u || (old & 3u) == 0u) {  // first of this epoch (so far): clear the pair root
                for (uint32_t w = 16; w < 24; ++w) pair[w] = 0u;
                __threadfence();
            }
            const uint32_t nw = (ahead == 0u ? old : epoch << 2) | (1u << slot);
            const uint32_t seen = atomicCAS(word, old, nw);
            if (seen == old) {
                second = (nw & 3u) == 3u;
                break;
            }
            old = seen;
        }
    }
    if (!__shfl(second, 0)) return;  // the other field's finisher is still running: it completes the pair
    __threadfence();
    const volatile uint32_t* both = pair;
    uint32_t e2 = 0u, o2 = 0u;
    if (i < 8u) {  // lanes 0..3: field 0's root, 4..7: field 1's
        const uint32_t lo = both[2 * i], hi = both[2 * i + 1];
        e2 = ilv::to_ilv(lo, hi, 0);
        o2 = ilv::to_ilv(lo, hi, 1);
    } else if (i == 8u) {
        e2 = 1u;  // byte 64
    }
    if (i == 16u) o2 ^= 0x80000000u;
    spread::keccak_f(e2, o2, cst);
    spread_store_digest(e2, o2, L, pair + 16);
}

template <uint32_t NT, bool LEAF>
__global__ __launch_bounds__(NT) void k_wave3(ReduceArgs a) {
    constexpr uint32_t kSpan = NT / 2;  // first-level nodes (lane pairs) per workgroup
    __shared__ uint32_t lds[8 * kSpan];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = tid >> 1;
    const uint32_t p = tid & 1u;
    const uint64_t wg = a.wg_base + blockIdx.x;
    const uint64_t lo1 = wg * kSpan;
    const uint64_t c1 = a.c1;
    const uint64_t m1 = (c1 - lo1) < kSpan ? (c1 - lo1) : kSpan;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(a.items);
    if (LEAF && k < m1) {  // window j of the item bytes
        const uint64_t j = lo1 + k;
        uint32_t d[4];
        if (j < a.c1_full) {
            hash_window3(reinterpret_cast<const uint4*>(a.items) + j * 16, p, d);
        } else {  // ragged window: both lanes run the full-state sponge
            uint4 d0, d1;
            first_level_generic<true>(a, j, d0, d1);
            d[0] = ilv::to_ilv(d0.x, d0.y, p);
            d[1] = ilv::to_ilv(d0.z, d0.w, p);
            d[2] = ilv::to_ilv(d1.x, d1.y, p);
            d[3] = ilv::to_ilv(d1.z, d1.w, p);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) lds[8 * k + 2 * w + p] = d[w];
    } else if (!LEAF && k < m1) {
        const uint64_t j = lo1 + k;
        uint32_t l[4], r[4] = {0, 0, 0, 0}, d[4];
        load_node3(in, 2 * j, a.in_ilv, p, l);
        if (a.cin == 1 && !a.pad_at_one) {  // single node: it is the root
#pragma unroll
            for (int w = 0; w < 4; ++w) d[w] = l[w];
        } else {
            const bool padded = !(2 * j + 1 < a.cin);
            if (!padded) load_node3(in, 2 * j + 1, a.in_ilv, p, r);
            hash_pair3(l, r, padded, p, d);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) lds[8 * k + 2 * w + p] = d[w];
    }
    __syncthreads();
    uint64_t c = c1, m = m1;
    int left = a.finalize ? 64 : (int)a.levels - 1;
    int done = 0;
    while (left > 0 && (c > 1 || a.pad_at_one)) {
        const uint64_t mn = (m + 1) / 2;
        if (mn <= NT / 64) break;  // one parent per wave from here
        const bool act = k < mn;
        uint32_t l[4], r[4] = {0, 0, 0, 0};
        bool padded = false;
        if (act) {
            padded = !(2 * (uint64_t)k + 1 < m);
#pragma unroll
            for (int w = 0; w < 4; ++w) l[w] = lds[16 * k + 2 * w + p];
            if (!padded) {
#pragma unroll
                for (int w = 0; w < 4; ++w) r[w] = lds[16 * k + 8 + 2 * w + p];
            }
        }
        __syncthreads();
        if (act) {
            uint32_t d[4];
            hash_pair3(l, r, padded, p, d);
#pragma unroll
            for (int w = 0; w < 4; ++w) lds[8 * k + 2 * w + p] = d[w];
        }
        __syncthreads();
        c = (c + 1) / 2;
        m = mn;
        --left;
        ++done;
    }
    wave3_spread_levels<NT>(lds, c, m, left, done, a.pad_at_one);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out);
    if (a.finalize) {
        if (tid < 64)
            wave3_spread_final(lds, a.n_items, out, reinterpret_cast<uint32_t*>(a.pair_block), a.pair_slot,
                               a.pair_epoch);
    } else if (k < m) {
        const uint64_t lo_out = lo1 >> done;
        uint32_t d[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) d[w] = lds[8 * k + 2 * w + p];
        store_node3(out, lo_out + k, a.out_ilv, p, d);
    }
}

template __global__ void k_wave3<64, false>(ReduceArgs);
template __global__ void k_wave3<128, false>(ReduceArgs);
template __global__ void k_wave3<256, false>(ReduceArgs);
template __global__ void k_wave3<512, false>(ReduceArgs);
template __global__ void k_wave3<1024, false>(ReduceArgs);
template __global__ void k_wave3<64, true>(ReduceArgs);
template __global__ void k_wave3<128, true>(ReduceArgs);
template __global__ void k_wave3<256, true>(ReduceArgs);
template __global__ void k_wave3<512, true>(ReduceArgs);
template __global__ void k_wave3<1024, true>(ReduceArgs);

// Wave priority of the trie's latency-bound top kernels (s_setprio): they run
// beside a phase-locked front at one wave per SIMD (the pipelined C5 stream),
// where the locked waves otherwise take most of the issue slots and the top's
// dependent chain, not the front, sets the step.  One
// process A/B (profiles/r05/c5_front_ab/ab_knobs.txt): the pipelined stream
// 0.4386 -> 0.4231 ms/step at priority 1 (0.4239 at 3, 0.4386 at the default 0).
constexpr int kTrieTopPrio = 1;
// Narrow top of the deposit trie, bit-interleaved lane pairs (mk::ilv): the
// workgroup owns NT input nodes of level d (NT/2 lane pairs) and writes
// `levels` levels to the (plain) level array; once the count is 1 it goes on
// with node = K(node || 0^32), the zero-sibling levels of
// deposit_trie.go:33-38.  The host picks NT so a launch has <= ~256
// workgroups; the last launch (one workgroup) runs to the top of the trie.
template <uint32_t NT>
__global__ __launch_bounds__(NT) void k_trie_top3(const uint32_t* __restrict__ in, uint64_t cin,
                                                  uint32_t* __restrict__ lv_out, uint32_t levels, uint64_t capn) {
    __builtin_amdgcn_s_setprio(kTrieTopPrio);
    constexpr uint32_t kPairs = NT / 2;
    __shared__ uint32_t lds[8 * kPairs];
    const uint32_t tid = threadIdx.x, k = tid >> 1, p = tid & 1u;
    uint64_t c = cin;
    uint64_t lo = (uint64_t)blockIdx.x * NT;  // first input node of this workgroup
    uint64_t m = (c - lo) < NT ? (c - lo) : NT;
    uint32_t* dst = lv_out;
    for (uint32_t l = 0; l < levels; ++l) {
        const uint64_t cn = (c + 1) / 2, mn = (m + 1) / 2;
        const bool act = k < mn;
        uint32_t a[4], b[4] = {0, 0, 0, 0};
        if (act) {
            const bool right = 2 * (uint64_t)k + 1 < m;
            if (l == 0) {
                load_node3(in, lo + 2 * (uint64_t)k, false, p, a);
                if (right) load_node3(in, lo + 2 * (uint64_t)k + 1, false, p, b);
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) a[w] = lds[16 * k + 2 * w + p];
                if (right) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) b[w] = lds[16 * k + 8 + 2 * w + p];
                }
            }
        }
        __syncthreads();
        if (act) {
            uint32_t d[4];
            hash_pair3(a, b, false, p, d);
#pragma unroll
            for (int w = 0; w < 4; ++w) lds[8 * k + 2 * w + p] = d[w];
            store_node3(dst, lo / 2 + k, false, p, d);
        }
        __syncthreads();
        dst += 8 * capn;  // next level's slot of the level array (capacity layout)
        capn = (capn + 1) / 2;
        c = cn;
        m = mn;
        lo /= 2;
    }
}

template __global__ void k_trie_top3<64>(const uint32_t*, uint64_t, uint32_t*, uint32_t, uint64_t);
template __global__ void k_trie_top3<128>(const uint32_t*, uint64_t, uint32_t*, uint32_t, uint64_t);
template __global__ void k_trie_top3<256>(const uint32_t*, uint64_t, uint32_t*, uint32_t, uint64_t);
template __global__ void k_trie_top3<512>(const uint32_t*, uint64_t, uint32_t*, uint32_t, uint64_t);
template __global__ void k_trie_top3<1024>(const uint32_t*, uint64_t, uint32_t*, uint32_t, uint64_t);

// ----------------------------------------------------------------------------
// Final hash for trees with <= 1 chunk: K(bytes[0,total) || [0^128 if n==0] || lenc)
__global__ void k_final_small(const uint8_t* __restrict__ items, uint64_t total, uint64_t n, uint8_t* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint4 d0, d1;
    sponge_generic(items, total, n == 0 ? 128u : 0u, true, n, d0, d1);
    reinterpret_cast<uint4*>(out)[0] = d0;
    reinterpret_cast<uint4*>(out)[1] = d1;
}

// ----------------------------------------------------------------------------
// Batched hashutil.Hash: n messages of 64 B (one permutation each).
// 6 waves/SIMD (73 VGPRs, no spill): 2^24 messages 1.804 -> 1.749 ms against
// the unconstrained 82 VGPRs / 5 waves (8 waves spills and halves the rate)
#define MK_K64_WAVES 6
__global__ __launch_bounds__(256, MK_K64_WAVES) void k_keccak64(const uint4* __restrict__ in, uint64_t n,
                                                               uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* p = in + 4 * i;
    const uint4 v0 = ld_stream(p), v1 = ld_stream(p + 1);
    const uint4 v2 = ld_stream(p + 2), v3 = ld_stream(p + 3);
    uint4 d0, d1;
    hash_pair(v0, v1, v2, v3, false, d0, d1);
    out[2 * i] = d0;
    out[2 * i + 1] = d1;
}

// digest outputs nobody in this kernel reads again (a non-temporal store was tried and not kept)
__device__ __forceinline__ void st_out(uint4* p, uint4 v) { *p = v; }

// Phase-locked 64-B messages (C2 and 64-B node pairs) for n =
// 1024 * ngroups messages, the rest by k_keccak64.  1024-thread workgroups,
// one per CU, persistent; lane m of wave w hashes message g * 1024 + 64 w + m
// (one phase-locked permutation).  The wave's 64 messages (4 KB, contiguous)
// land in its 5 KB of LDS by coalesced DMA in a stride-5 image: position
// 5 m + u holds unit u of message m (u = 4 repeats unit 3), so consecutive
// lanes of an instruction read consecutive 16-B units and lane m reads its
// 4 units back at an odd stride, conflict-free.  The next group's copy goes
// out as soon as the message is read (one permutation ahead).
__global__ __launch_bounds__(kLockThreads, 1) void k_keccak64_lock(const uint4* __restrict__ in, uint64_t n,
                                                                   uint4* __restrict__ out) {
    __shared__ uint4 buf[kLockThreads / 64][5 * 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* Bw = buf[wave];
    // a partial last group: lanes past n hash a copy of message n - 1 and store nothing
    const uint64_t ngroups = (n + kLockThreads - 1) / kLockThreads;
    // instructions [i0, i1) of the 5 (issued in parts over the permutation)
    auto dma = [&](uint64_t g, uint32_t i0, uint32_t i1) {
        const uint64_t m0 = g * kLockThreads + 64 * wave;
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t p = 64 * i + ln, m = p / 5, u = p - 5 * m;
            const uint64_t msg = m0 + m < n ? m0 + m : n - 1;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(in + 4 * msg + (u < 4 ? u : 3)),
                                             (__attribute__((address_space(3))) void*)(Bw + 64 * i), 16, 0,
                                             kSideAux);
        }
    };
    uint64_t g = blockIdx.x;
    if (g < ngroups) dma(g, 0, 5);
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;  // the previous group's digest, stored after the next wait
    uint64_t qi = 0;
    bool pend = false;
#pragma unroll 1
    for (; g < ngroups; g += gridDim.x) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the wave's messages have landed
        if (pend && qi < n) {
            st_out(out + 2 * qi, q0);
            st_out(out + 2 * qi + 1, q1);
        }
        State s;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 v = Bw[5 * lane + u];
            s.lo[2 * u] = v.x;
            s.hi[2 * u] = v.y;
            s.lo[2 * u + 1] = v.z;
            s.hi[2 * u + 1] = v.w;
        }
#pragma unroll
        for (int k = 8; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
        s.lo[8] = 1u;  // byte 64
        s.hi[16] = 0x80000000u;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read: the next group's copy may land
        // one burst (5 instructions; in three parts over the permutation:
        // 1.476 -> 1.483 ms at 2^24, within noise, profiles/r05/side_dma_split/)
        if (g + gridDim.x < ngroups) dma(g + gridDim.x, 0, 5);
        keccak_f_digest_lock(s);
        digest(s, q0, q1);
        qi = g * kLockThreads + threadIdx.x;
        pend = true;
    }
    if (pend && qi < n) {
        st_out(out + 2 * qi, q0);
        st_out(out + 2 * qi + 1, q1);
    }
}

// Phase-locked node pass (the wide node pass of a whole tree, planner.cpp):
// 1024-thread workgroups, one per CU, persistent.  Thread t of group g folds
// the 16 node pairs [16 (1024 g + t), +16) -- 32 consecutive nodes, a subtree
// -- through 5 levels in registers (16 + 8 + 4 + 2 + 1 = 31 locked
// permutations) into output node 1024 g + t: the spans of k_reduce<NODE>
// workgroups 16 g .. 16 g + 15 with a.levels == 5, same output order.  Pair j
// of every lane of a wave (64 B, lanes 1 KB apart) lands in the wave's 5 KB
// of LDS by coalesced DMA in k_keccak64_lock's stride-5 image, issued as soon
// as pair j - 1 has been read (one permutation or more ahead); pairs j and
// j + 1 share a 128-B line, the second read an L2 hit.  All pairs are
// complete (no odd padding): the host launches whole groups of full pairs.
// Stores go right after a wait, as in k_leaf_lock_sc.
__global__ __launch_bounds__(kLockThreads, 1) void k_node_lock(ReduceArgs a, uint64_t ngroups) {
    __shared__ uint4 buf[kLockThreads / 64][5 * 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* Bw = buf[wave];
    const uint4* in = reinterpret_cast<const uint4*>(a.items);
    uint4* out = reinterpret_cast<uint4*>(a.out);
    auto dma = [&](uint64_t g, uint32_t j) {
        const uint64_t p0 = (g * kLockThreads + 64 * wave) * kNodeLockPairs + j;  // lane 0's pair j
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (uint32_t i = 0; i < 5; ++i) {
            const uint32_t p = 64 * i + ln, m = p / 5, u = p - 5 * m;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const void*>(in + 4 * (p0 + (uint64_t)kNodeLockPairs * m) + (u < 4 ? u : 3)),
                (__attribute__((address_space(3))) void*)(Bw + 64 * i), 16, 0, 0);
        }
    };
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;  // the previous group's node, stored one group late
    uint64_t qi = 0;
    bool pend = false;
    uint64_t g = blockIdx.x;
    if (g < ngroups) dma(g, 0);
    // pair j of group g: wait for its DMA, read it, send the next pair's
    // DMA (pair j + 1, or pair 0 of the workgroup's next group), hash it
    auto pair = [&](uint64_t gg, uint32_t j, uint4& d0, uint4& d1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (j == 0 && pend) {
            out[2 * qi] = q0;
            out[2 * qi + 1] = q1;
            pend = false;
        }
        const uint4 l0 = Bw[5 * lane], l1 = Bw[5 * lane + 1], r0 = Bw[5 * lane + 2], r1 = Bw[5 * lane + 3];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read: the next pair may land
        if (j + 1 < kNodeLockPairs)
            dma(gg, j + 1);
        else if (gg + gridDim.x < ngroups)
            dma(gg + gridDim.x, 0);
        hash_node_lock(l0, l1, r0, r1, d0, d1);
    };
#pragma unroll 1
    for (; g < ngroups; g += gridDim.x) {
        uint4 a0 = q0, a1 = q1;  // level-3 node of the even quarter (the value is never read before it is set)
        uint4 b0 = q0, b1 = q1;  // level-4 node of the first half
#pragma unroll 1
        for (uint32_t k = 0; k < kNodeLockPairs / 4; ++k) {
            uint4 l0, l1, r0, r1, e0, e1;
            pair(g, 4 * k, l0, l1);
            pair(g, 4 * k + 1, r0, r1);
            hash_node_lock(l0, l1, r0, r1, e0, e1);
            pair(g, 4 * k + 2, l0, l1);
            pair(g, 4 * k + 3, r0, r1);
            hash_node_lock(l0, l1, r0, r1, l0, l1);
            hash_node_lock(e0, e1, l0, l1, e0, e1);  // level 3
            if ((k & 1) == 0) {
                a0 = e0;
                a1 = e1;
            } else {
                hash_node_lock(a0, a1, e0, e1, e0, e1);  // level 4
                if (k == 1) {
                    b0 = e0;
                    b1 = e1;
                } else {
                    hash_node_lock(b0, b1, e0, e1, q0, q1);  // level 5: the thread's output node
                }
            }
        }
        qi = g * kLockThreads + threadIdx.x;
        pend = true;
    }
    if (pend) {
        out[2 * qi] = q0;
        out[2 * qi + 1] = q1;
    }
}

// n messages of fixed msg_len bytes (any length / alignment).
__global__ __launch_bounds__(256) void k_keccak_fixed(const uint8_t* __restrict__ in, uint64_t n, uint32_t msg_len,
                                                      uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 d0, d1;
    sponge_generic(in + i * msg_len, msg_len, 0, false, 0, d0, d1);
    out[2 * i] = d0;
    out[2 * i + 1] = d1;
}

// n variable-length messages: message i = in[offs[i], offs[i+1]).
__global__ __launch_bounds__(256) void k_keccak_var(const uint8_t* __restrict__ in, const uint64_t* __restrict__ offs,
                                                    uint64_t n, uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = offs[i], b = offs[i + 1];
    uint4 d0, d1;
    sponge_generic(in + a, b - a, 0, false, 0, d0, d1);
    out[2 * i] = d0;
    out[2 * i + 1] = d1;
}

// struct hashing: k_struct_fields, _fused, _nested, _reg, _lock, _split and their helpers
#include "kernels_struct.hip"

// ----------------------------------------------------------------------------
// n messages of msg_len bytes, msg_len % 8 == 0, 8-byte aligned: whole-word
// loads only (deposit leaves: 280 B = 35 words = 3 blocks).
__global__ __launch_bounds__(256) void k_keccak_words(const uint2* __restrict__ in, uint64_t n, uint32_t nwords,
                                                      uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2* p = in + i * nwords;
    const uint32_t nb = nwords / 17 + 1;
    State s;
    zero(s);
    if ((((uintptr_t)p) & 7u) == 0) {
        // 16-B loads: a message starts 16-B aligned or 8 bytes past it; each
        // block reads the 9 aligned 16-B units that cover its 17 words and
        // selects per lane (deposit leaves: 35 words, 3 blocks)
        const uint32_t so = (((uintptr_t)p) & 15u) ? 1u : 0u;
        const uint4* q = reinterpret_cast<const uint4*>(p - so);
        const uint32_t nq = (nwords + so + 1) / 2;
#pragma unroll 1
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t first = 17 * b + so;  // aligned word index of block word 0
            const uint32_t pb = first >> 1, odd = first & 1u;
            uint2 e[18];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const uint4 t = (pb + k) < nq ? ld_stream(q + pb + k) : make_uint4(0, 0, 0, 0);
                e[2 * k] = make_uint2(t.x, t.y);
                e[2 * k + 1] = make_uint2(t.z, t.w);
            }
#pragma unroll
            for (int w = 0; w < 17; ++w) {
                const uint32_t idx = 17 * b + w;
                // static-index select (a conditional index would spill e[] to scratch)
                const uint32_t msk = 0u - odd;
                uint2 v = make_uint2(__builtin_amdgcn_bitop3_b32(e[w].x, e[w + 1].x, msk, 0xD8),
                                     __builtin_amdgcn_bitop3_b32(e[w].y, e[w + 1].y, msk, 0xD8));
                if (idx >= nwords) v = make_uint2(idx == nwords ? 1u : 0u, 0u);  // zero / domain pad
                s.lo[w] ^= v.x;
                s.hi[w] ^= v.y;
            }
            if (b == nb - 1) s.hi[16] ^= 0x80000000u;
            if (b + 1 < nb)  // nb is uniform (fixed message length)
                keccak_f(s);
            else
                keccak_f_digest(s);
        }
    } else {
#pragma unroll 1
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t base = b * 17;
#pragma unroll
            for (int w = 0; w < 17; ++w) {
                const uint32_t idx = base + w;
                if (idx < nwords) {
                    const uint2 v = ld_stream(p + idx);
                    s.lo[w] ^= v.x;
                    s.hi[w] ^= v.y;
                } else if (idx == nwords) {
                    s.lo[w] ^= 1u;  // domain pad byte right after the message
                }
            }
            if (b == nb - 1) s.hi[16] ^= 0x80000000u;
            if (b + 1 < nb)  // nb is uniform (fixed message length)
                keccak_f(s);
            else
                keccak_f_digest(s);
        }
    }
    uint4 d0, d1;
    digest(s, d0, d1);
    out[2 * i] = d0;
    out[2 * i + 1] = d1;
}

// Fixed-size records of NW 8-byte words (8-B aligned; deposit leaves: 280 B
// = 35 words = 3 blocks), grid-stride; each block is loaded right before it
// is absorbed.  8-B loads need no per-lane alignment select (k_keccak_words
// spends 2 VALU per word on it).  Prefetching block b+1 into 34 VGPRs while
// block b permutes was 1-2 % slower on the 2^20-deposit trie (0.588 vs
// 0.582 ms, profiles/r02d/ab_rec_prefetch.log): the other resident waves
// hide the load as well.  At 5 waves/SIMD (96 VGPRs, 4 dwords spilled) the
// stream of 2^20-deposit tries got 3 % slower (profiles/r02m/rejected/).
#define MK_REC_WAVES 1
template <int NW>
__global__ __launch_bounds__(kRecThreads, MK_REC_WAVES) void k_keccak_rec(const uint2* __restrict__ in, uint64_t n,
                                                                          uint4* __restrict__ out) {
    constexpr int NB = NW / 17 + 1;
    const uint64_t stride = (uint64_t)gridDim.x * kRecThreads;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x; i < n; i += stride) {
        const uint2* p = in + i * NW;
        State s;
        zero(s);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int w = 0; w < 17; ++w) {
                const int idx = 17 * b + w;
                if (idx < NW) {
                    const uint2 v = p[idx];
                    s.lo[w] ^= v.x;
                    s.hi[w] ^= v.y;
                } else if (idx == NW) {
                    s.lo[w] ^= 1u;  // domain pad byte right after the message
                }
            }
            if (b == NB - 1) s.hi[16] ^= 0x80000000u;
            if (b + 1 < NB)
                keccak_f(s);
            else
                keccak_f_digest(s);
        }
        uint4 d0, d1;
        digest(s, d0, d1);
        out[2 * i] = d0;
        out[2 * i + 1] = d1;
    }
}
template __global__ void k_keccak_rec<35>(const uint2*, uint64_t, uint4*);

// Phase-locked deposit-trie front: the leaf hashes of 280-B
// deposits (deposit_trie.go:32, Hash(depositData)) AND the trie levels above
// them up to the node over DPT leaves (deposit_trie.go:33-38), in one launch.
// Every thread owns DPT consecutive deposits: 3 permutations each (2 full
// rate blocks + the 8-B tail), then DPT - 1 node permutations, all phase-
// locked (two s_barriers per round) -- DPT = 4: 15 permutations,
// levels 1-2.  Thread t of group g holds deposits DPT (g NT + t) + i; it
// writes its leaves and nodes to levels 0..log2(DPT) of the trie (all kept:
// GenerateMerkleBranch reads them), so the 2^20-leaf round trip through HBM
// and the level launches of the free-running form go away.
// Staging (the k_leaf_lock_sc scheme): block b of slot i of the wave's 64
// lanes is DMA'd into the wave's 9 KB of LDS, the 9 16-B units covering each
// lane's 136-B block flattened U = 9 m + u (consecutive lanes on consecutive
// units of one deposit).  Deposit DPT m + i starts 8 (i & 1) bytes into a
// 16-B unit (280 = 17.5 x 16, DPT even), so lane m's 17 words sit at byte
// 144 m + 8 ((i + b) & 1) of the image.  Block 1 of slot i is in flight
// during block 0's permutation, block 0 of slot i + 1 (or of the next group)
// during block 1's; the 8-B tail words are loaded per lane one slot ahead.
// Whole groups only (the host runs the rest with k_keccak_rec + k_trie_level).
// global_load_lds policy of the deposit DMA: 0 (nt = 2: +0.7 % on the
// pipelined stream, profiles/r05/c5_front_ab/)
constexpr int kTrieLockAux = 0;
// The next block's 9-unit DMA goes out in parts spread over the current
// block's permutation: units 0-2, 3-5, 6-8 after rounds MK_TRIE_DMA_SPLIT,
// MK_TRIE_DMA_SPLIT3 and MK_TRIE_DMA_ROUND (SPLIT3 = 0: units 0-4 / 5-8
// after SPLIT / ROUND; SPLIT = 0: all after ROUND).  Issued all at once, 16
// waves' DMA instructions burst together and the locked waves wait on the
// slowest issue.  One process A/B (profiles/r05/c5_front_ab/ab_dma_split*.txt,
// 9 interleaved rounds each, two boxes): pipelined stream 0.4086 -> 0.4017
// and 0.4163 -> 0.4092 ms/step (4/10/16 against all after 12), one trie
// 0.543 -> 0.515 and 0.561 -> 0.534 ms; two parts -1.1 %, one unit per round
// or two -0.4 to -1.1 %.
#define MK_TRIE_DMA_SPLIT 4
#define MK_TRIE_DMA_SPLIT3 10
// round of a block's permutation after which the next block's DMA (its last
// part) goes out; as one part: 12 (mid-permutation) over 0, one trie 1.2-2.3
// % faster on two boxes (profiles/r04/trie_dma_ab/); in three parts: 16
#define MK_TRIE_DMA_ROUND 16

// PIPE (a stream of tries, pipeline.TriePipeline): workgroup b also takes the
// previous trie's subtree over its level-2 nodes [1024 b, 1024 b + 1024) up
// to level 7: 512 + 256 + 128 + 64 + 32 node permutations.  Each wave does
// ONE of them (level 3 on waves 0-7, 4 on 8-11, 5 on 12-13, 6 on 14, 7 on
// 15, one node per lane) as an extra lock-step permutation inserted into its
// own sequence, so every wave runs 16 permutations and the same barriers; a
// level is inserted at least one whole permutation after the level it reads
// was stored (slots 0, 3, 7, 10, 15: between deposits, where no state is
// live), through L2 (same CU, lines it never read).  The 15 per-thread permutations of the front cost 15 slots alone;
// the previous trie's wide top levels cost one more instead of a separate
// latency-bound pass beside the front.
template <uint32_t NT, int DPT, bool PIPE>
__global__ __launch_bounds__(NT, 1) void k_trie_rec_lock(const uint2* __restrict__ in, uint64_t ngroups,
                                                         uint4* __restrict__ L0, uint4* __restrict__ L1,
                                                         uint4* __restrict__ L2, uint4* __restrict__ L3,
                                                         TriePrev prev) {
    static_assert(!PIPE || (NT == 1024 && DPT == 4), "the previous-trie slots assume 16 waves x 4 deposits");
    constexpr uint32_t NW = 35;  // 8-B words per deposit
    constexpr int NLV = DPT == 8 ? 3 : DPT == 4 ? 2 : 1;
    static_assert(DPT == 2 || DPT == 4 || DPT == 8, "deposits per thread");
    __shared__ uint4 buf[NT / 64][9 * 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* Bw = buf[wave];
    uint4* const lv[4] = {L0, L1, L2, L3};
    auto first = [&](uint64_t g) { return (g * NT + 64 * wave) * DPT; };  // lane 0's first deposit
    // units [k0, k1) of the 9 (MK_TRIE_DMA_SPLIT: issued in two parts)
    auto dma = [&](uint64_t g, int i, int b, int k0 = 0, int k1 = 9) {
        const uint8_t* region = reinterpret_cast<const uint8_t*>(in + first(g) * NW);
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));  // recompute the offsets here (see lock_dma_c)
#pragma unroll
        for (int k = k0; k < k1; ++k) {
            const uint32_t U = 64u * k + ln;
            const uint32_t m = U / 9, u = U - m * 9;
            const uint32_t start = (DPT * m + i) * (8 * NW) + 136 * b;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(region + (start & ~15u) + 16 * u),
                                             (__attribute__((address_space(3))) void*)(Bw + 64 * k), 16, 0,
                                             kTrieLockAux);
        }
    };
    // a node is stored after the next slot's first wait, so no wait covers a
    // store issued just before it (stores count in vmcnt)
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    uint4* qp = nullptr;
    auto flush = [&] {
        if (qp) {
            qp[0] = q0;
            qp[1] = q1;
        }
    };
    // the previous trie's level k node of this lane (waves of level k only)
    const uint32_t wv = __builtin_amdgcn_readfirstlane(wave);
    auto prev_slot = [&](int k) {
        const uint32_t w0 = 16u - (16u >> (k - 3)), per = 512u >> (k - 3);  // first wave, nodes per workgroup
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));  // computed here, not hoisted and kept live across the loop
        const uint32_t j = 64u * (wv - w0) + ln;
        const bool act = prev.live && j < per;
        const uint32_t jg = blockIdx.x * per + j;  // < 2^19: 32-bit offsets from the uniform bases
        const uint4* src = k == 3 ? prev.l2 : prev.l[k - 4];
        asm volatile("" ::: "memory");
        State s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = act ? src[4 * jg + q] : make_uint4(0, 0, 0, 0);
            s.lo[2 * q] = v.x;
            s.hi[2 * q] = v.y;
            s.lo[2 * q + 1] = v.z;
            s.hi[2 * q + 1] = v.w;
        }
#pragma unroll
        for (int w = 8; w < 25; ++w) s.lo[w] = s.hi[w] = 0;
        s.lo[8] = 1u;  // byte 64
        s.hi[16] = 0x80000000u;
        keccak_f_digest_lock(s);
        if (act) {
            uint4 d0, d1;
            digest(s, d0, d1);
            prev.l[k - 3][2 * jg] = d0;
            prev.l[k - 3][2 * jg + 1] = d1;
        }
        asm volatile("" ::: "memory");
    };
    // Absorb lane m's staged block (17 8-B words) into s (XOR; SET: assign)
    // from its 9 16-B units, read as rows at the odd stride 9 (conflict-free
    // ds_read_b128: a b64 read of 8 B from each lane's own 16-B unit needs two
    // LDS cycles per 32 lanes whatever the layout).  The block starts `o8`
    // words (0 or 1, wave-uniform) into unit 0, so word w is half (w + o8) & 1
    // of unit (w + o8) / 2: one select per dword, every state index static
    // (the slot loop stays rolled).  Units are consumed one at a time (a
    // compiler fence between) so few data VGPRs are live beside the state.
    // Returns word 17 (the word after the block when o8 = 0).
    auto absorb = [&](State& st, uint32_t o8, auto setc) {
        constexpr bool SET = decltype(setc)::value;
        const bool sh = o8 != 0;
        uint4 prev = Bw[9 * lane];
        uint2 w17 = make_uint2(0, 0);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            // words 2k and 2k + 1: unshifted (x, y) (z, w) of unit k; shifted
            // (z, w) of unit k and (x, y) of unit k + 1
            const uint4 cur = k + 1 < 9 ? Bw[9 * lane + k + 1] : make_uint4(0, 0, 0, 0);
            const uint32_t a0 = sh ? prev.z : prev.x, a1 = sh ? prev.w : prev.y;
            const uint32_t b0 = sh ? cur.x : prev.z, b1 = sh ? cur.y : prev.w;
            const int wa = 2 * k, wb = 2 * k + 1;
            st.lo[wa] = SET ? a0 : st.lo[wa] ^ a0;
            st.hi[wa] = SET ? a1 : st.hi[wa] ^ a1;
            if (wb < 17) {
                st.lo[wb] = SET ? b0 : st.lo[wb] ^ b0;
                st.hi[wb] = SET ? b1 : st.hi[wb] ^ b1;
            } else {
                w17 = make_uint2(prev.z, prev.w);
            }
            prev = cur;
            asm volatile("" ::: "memory");
        }
        return w17;
    };
    using Set = std::true_type;
    using Xor = std::false_type;
    uint64_t g = blockIdx.x;
    if (g < ngroups) dma(g, 0, 0);
#pragma unroll 1
    for (; g < ngroups; g += gridDim.x) {
        const uint64_t gn = g + gridDim.x;
        const uint64_t r0 = first(g) + DPT * lane;  // this lane's first deposit (leaf index)
        uint4 kl0[NLV], kl1[NLV];                   // the pending left node of each level
#pragma unroll
        for (int i = 0; i < DPT; ++i) {
            // the previous trie's slots sit between deposits (no state live)
            if (PIPE && i == 0 && wv < 8) prev_slot(3);                // slot 0
            if (PIPE && i == 1 && (wv >> 2) == 2) prev_slot(4);        // slot 3
            if (PIPE && i == 2 && (wv == 12 || wv == 13)) prev_slot(5);  // slot 7
            if (PIPE && i == 3 && wv == 14) prev_slot(6);              // slot 10
            State s;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // block 0 landed
            flush();
            qp = nullptr;
            absorb(s, i & 1, Set{});
#pragma unroll
            for (int w = 17; w < 25; ++w) s.lo[w] = s.hi[w] = 0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // rows read: block 1 may land
            if constexpr (MK_TRIE_DMA_SPLIT3 > 0)
                keccak_f_lock_mid3<MK_TRIE_DMA_SPLIT, MK_TRIE_DMA_SPLIT3, MK_TRIE_DMA_ROUND>(
                    s, [&] { dma(g, i, 1, 0, 3); }, [&] { dma(g, i, 1, 3, 6); }, [&] { dma(g, i, 1, 6, 9); });
            else if constexpr (MK_TRIE_DMA_SPLIT > 0)
                keccak_f_lock_mid2<MK_TRIE_DMA_SPLIT, MK_TRIE_DMA_ROUND>(s, [&] { dma(g, i, 1, 0, 5); },
                                                                         [&] { dma(g, i, 1, 5, 9); });
            else
                keccak_f_lock_mid<MK_TRIE_DMA_ROUND>(s, [&] { dma(g, i, 1); });
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // block 1 landed
            // the 8-B tail word (deposit bytes 272..279): an odd slot's block 1
            // image ends with it (the block starts 16-B aligned, 9 units = 144
            // B); an even slot's is the first word of the NEXT slot's block 0
            // image (that deposit starts 8 B into the unit holding it), read
            // after its DMA lands below -- no per-lane load of its own
            // an odd slot's block 1 starts 16-B aligned and ends with the tail word
            uint2 tl = absorb(s, (i + 1) & 1, Xor{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            auto next_dma = [&](int k0, int k1) {
                if (i + 1 < DPT)
                    dma(g, i + 1, 0, k0, k1);
                else if (gn < ngroups)
                    dma(gn, 0, 0, k0, k1);
            };
            if constexpr (MK_TRIE_DMA_SPLIT3 > 0)
                keccak_f_lock_mid3<MK_TRIE_DMA_SPLIT, MK_TRIE_DMA_SPLIT3, MK_TRIE_DMA_ROUND>(
                    s, [&] { next_dma(0, 3); }, [&] { next_dma(3, 6); }, [&] { next_dma(6, 9); });
            else if constexpr (MK_TRIE_DMA_SPLIT > 0)
                keccak_f_lock_mid2<MK_TRIE_DMA_SPLIT, MK_TRIE_DMA_ROUND>(s, [&] { next_dma(0, 5); },
                                                                         [&] { next_dma(5, 9); });
            else
                keccak_f_lock_mid<MK_TRIE_DMA_ROUND>(s, [&] { next_dma(0, 9); });
            if (!(i & 1)) {  // slot i + 1 < DPT of this group: its block 0 holds the tail
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const uint4 v = Bw[9 * lane];
                tl = make_uint2(v.x, v.y);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            s.lo[0] ^= tl.x;  // word 34, then the domain pad byte (word 35 = lane 1)
            s.hi[0] ^= tl.y;
            s.lo[1] ^= 1u;
            s.hi[16] ^= 0x80000000u;
            keccak_f_digest_lock(s);
            uint4 d0, d1;
            digest(s, d0, d1);
            // fold: level l + 1 gets a node once slot i closes a pair at level l
            uint4* dst = lv[0] + 2 * (r0 + i);
#pragma unroll
            for (int l = 0; l <= NLV; ++l) {
                if (l == NLV || ((i >> l) & 1) == 0) {
                    if (l < NLV) {
                        kl0[l] = d0;
                        kl1[l] = d1;
                    }
                    q0 = d0;  // stored after the next wait
                    q1 = d1;
                    qp = dst;
                    break;
                }
                dst[0] = d0;  // covered by the node permutation below
                dst[1] = d1;
                hash_node_lock(kl0[l], kl1[l], d0, d1, d0, d1);
                dst = lv[l + 1] + 2 * ((r0 + i) >> (l + 1));
            }
        }
        if (PIPE && wv == 15) prev_slot(7);  // slot 15
    }
    flush();
}
template __global__ void k_trie_rec_lock<1024, 4, true>(const uint2*, uint64_t, uint4*, uint4*, uint4*, uint4*,
                                                        TriePrev);

// Slot-major form of the whole-trie front (round 6, the verdict's A/B; the
// one-trie front since, profiles/r06/c5_slot_major/): lane m of wave w hashes deposits base + 64 i + m
// (slot i = 0..3, base = the wave's first of 256), so a DMA phase reads 64
// consecutive deposits and the lines two consecutive deposits share are
// fetched by adjacent parts, where the row form fetches every fourth such
// line seven phases apart.  The blocks are staged and read exactly as in
// k_trie_rec_lock (9 units per lane, rows at stride 9), with the 8-B offset
// now per lane (deposit parity = lane parity).  An even lane's tail word is
// the first word of the NEXT lane's block-0 image (read before block 1's
// copy lands); an odd lane's block-1 image ends with it.  Leaves sit in
// consecutive lanes, so the folds move them with ds_bpermute: after slots 1
// and 3 one locked permutation hashes the 64 level-1 nodes of the two slots
// (lane m: slot pair half m >> 5, pair m & 31), after slot 3 one more the 64
// level-2 nodes (lane m: level-1 nodes 2m, 2m + 1) -- 15 locked permutations
// per thread, as in the row form; levels 0-2 are stored as consecutive
// nodes per wave.
#if MK_TOP_STAMPS
// diagnostic build only (tools/top_probe.hip): s_memrealtime at the start and
// the end of each workgroup of the slot-major front
__device__ uint64_t g_front_stamps[2 * 1024];
#endif
template <uint32_t NT>
__global__ __launch_bounds__(NT, 1) void k_trie_rec_lock_sm(const uint2* __restrict__ in, uint64_t ngroups,
                                                            uint4* __restrict__ L0, uint4* __restrict__ L1,
                                                            uint4* __restrict__ L2) {
#if MK_TOP_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_front_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
    constexpr uint32_t NW = 35;  // 8-B words per deposit
    __shared__ uint4 buf[NT / 64][9 * 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* Bw = buf[wave];
    auto first = [&](uint64_t g) { return (g * NT + 64 * wave) * 4; };  // the wave's first deposit
    // units [k0, k1) of slot i's block b (the slot's 64 deposits start 16-B aligned)
    auto dma = [&](uint64_t g, int i, int b, int k0, int k1) {
        const uint8_t* region = reinterpret_cast<const uint8_t*>(in + (first(g) + 64u * i) * NW);
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int k = k0; k < k1; ++k) {
            const uint32_t U = 64u * k + ln;
            const uint32_t m = U / 9, u = U - m * 9;
            const uint32_t start = m * (8 * NW) + 136 * b;
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(region + (start & ~15u) + 16 * u),
                                             (__attribute__((address_space(3))) void*)(Bw + 64 * k), 16, 0,
                                             kTrieLockAux);
        }
    };
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;  // a node stored after the next wait
    uint4* qp = nullptr;
    auto flush = [&] {
        if (qp) {
            qp[0] = q0;
            qp[1] = q1;
        }
        qp = nullptr;
    };
    // 17 words of this lane's staged block into st (rows at stride 9; the
    // block starts o8 words into unit 0); returns word 17
    auto absorb = [&](State& st, uint32_t o8, auto setc) {
        constexpr bool SET = decltype(setc)::value;
        const bool sh = o8 != 0;
        uint4 prev = Bw[9 * lane];
        uint2 w17 = make_uint2(0, 0);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const uint4 cur = k + 1 < 9 ? Bw[9 * lane + k + 1] : make_uint4(0, 0, 0, 0);
            const uint32_t a0 = sh ? prev.z : prev.x, a1 = sh ? prev.w : prev.y;
            const uint32_t b0 = sh ? cur.x : prev.z, b1 = sh ? cur.y : prev.w;
            const int wa = 2 * k, wb = 2 * k + 1;
            st.lo[wa] = SET ? a0 : st.lo[wa] ^ a0;
            st.hi[wa] = SET ? a1 : st.hi[wa] ^ a1;
            if (wb < 17) {
                st.lo[wb] = SET ? b0 : st.lo[wb] ^ b0;
                st.hi[wb] = SET ? b1 : st.hi[wb] ^ b1;
            } else {
                w17 = make_uint2(prev.z, prev.w);
            }
            prev = cur;
            asm volatile("" ::: "memory");
        }
        return w17;
    };
    // node (x, y of two uint4) of lane `src` (8 bpermutes)
    auto bperm8 = [](uint32_t src, const uint4& a, const uint4& b, uint4& ra, uint4& rb) {
        const int ad = (int)(4u * src);
        ra.x = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)a.x);
        ra.y = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)a.y);
        ra.z = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)a.z);
        ra.w = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)a.w);
        rb.x = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)b.x);
        rb.y = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)b.y);
        rb.z = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)b.z);
        rb.w = (uint32_t)__builtin_amdgcn_ds_bpermute(ad, (int)b.w);
    };
    auto sel4 = [](bool c, const uint4& a, const uint4& b) {
        return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
    };
    // level-1 nodes of slots (i0, i0 + 1) from their leaves in (xa, ya) / (xb, yb):
    // lane m hashes pair m & 31 of slot i0 + (m >> 5)
    auto level1 = [&](const uint4& xa, const uint4& ya, const uint4& xb, const uint4& yb, uint4& n0, uint4& n1) {
        const uint32_t p = lane & 31u;
        const bool hi_half = lane >= 32u;
        uint4 la0, la1, lb0, lb1, ra0, ra1, rb0, rb1;
        bperm8(2 * p, xa, ya, la0, la1);
        bperm8(2 * p, xb, yb, lb0, lb1);
        bperm8(2 * p + 1, xa, ya, ra0, ra1);
        bperm8(2 * p + 1, xb, yb, rb0, rb1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        hash_node_lock(sel4(hi_half, lb0, la0), sel4(hi_half, lb1, la1), sel4(hi_half, rb0, ra0),
                       sel4(hi_half, rb1, ra1), n0, n1);
    };
    using Set = std::true_type;
    using Xor = std::false_type;
    uint64_t g = blockIdx.x;
    if (g < ngroups) {
        dma(g, 0, 0, 0, 9);
    }
#pragma unroll 1
    for (; g < ngroups; g += gridDim.x) {
        const uint64_t gn = g + gridDim.x;
        const uint64_t base = first(g);
        uint4 xa = make_uint4(0, 0, 0, 0), ya = xa;  // leaf of the even slot of a pair
        uint4 n10 = xa, n11 = xa;                    // level-1 node of slots 0, 1
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            State s;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // block 0 landed
            flush();
            // an even lane's tail word: the first word of the next lane's block-0 image
            uint2 te = make_uint2(0, 0);
            if (!(lane & 1u)) {
                const uint4 v = Bw[9 * (lane + 1)];
                te = make_uint2(v.x, v.y);
            }
            absorb(s, lane & 1u, Set{});
#pragma unroll
            for (int w = 17; w < 25; ++w) s.lo[w] = s.hi[w] = 0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // rows read: block 1 may land
            keccak_f_lock_mid3<MK_TRIE_DMA_SPLIT, MK_TRIE_DMA_SPLIT3, MK_TRIE_DMA_ROUND>(
                s, [&] { dma(g, i, 1, 0, 3); }, [&] { dma(g, i, 1, 3, 6); }, [&] { dma(g, i, 1, 6, 9); });
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // block 1 landed
            const uint2 to = absorb(s, (lane + 1) & 1u, Xor{});
            const uint2 tl = (lane & 1u) ? to : te;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            auto next_dma = [&](int k0, int k1) {
                if (i + 1 < 4)
                    dma(g, i + 1, 0, k0, k1);
                else if (gn < ngroups)
                    dma(gn, 0, 0, k0, k1);
            };
            keccak_f_lock_mid3<MK_TRIE_DMA_SPLIT, MK_TRIE_DMA_SPLIT3, MK_TRIE_DMA_ROUND>(
                s, [&] { next_dma(0, 3); }, [&] { next_dma(3, 6); }, [&] { next_dma(6, 9); });
            s.lo[0] ^= tl.x;  // word 34, then the domain pad byte
            s.hi[0] ^= tl.y;
            s.lo[1] ^= 1u;
            s.hi[16] ^= 0x80000000u;
            keccak_f_digest_lock(s);
            uint4 d0, d1;
            digest(s, d0, d1);
            uint4* leaf = L0 + 2 * (base + 64u * i + lane);
            if (!(i & 1)) {
                xa = d0;
                ya = d1;
                q0 = d0;  // stored after the next wait
                q1 = d1;
                qp = leaf;
            } else {
                leaf[0] = d0;  // covered by the node permutation below
                leaf[1] = d1;
                uint4 n0, n1;
                level1(xa, ya, d0, d1, n0, n1);
                uint4* nd = L1 + 2 * (base / 2 + 64u * (i >> 1) + lane);
                if (i == 1) {
                    n10 = n0;
                    n11 = n1;
                    q0 = n0;
                    q1 = n1;
                    qp = nd;
                } else {
                    nd[0] = n0;
                    nd[1] = n1;
                    // level 2: lane m hashes level-1 nodes 2m, 2m + 1 (of slots 0-1
                    // for m < 32, of slots 2-3 after)
                    const bool hi_half = lane >= 32u;
                    const uint32_t src = (2u * lane) & 63u;
                    uint4 la0, la1, lb0, lb1, ra0, ra1, rb0, rb1;
                    bperm8(src, n10, n11, la0, la1);
                    bperm8(src, n0, n1, lb0, lb1);
                    bperm8(src + 1, n10, n11, ra0, ra1);
                    bperm8(src + 1, n0, n1, rb0, rb1);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    uint4 m0, m1;
                    hash_node_lock(sel4(hi_half, lb0, la0), sel4(hi_half, lb1, la1), sel4(hi_half, rb0, ra0),
                                   sel4(hi_half, rb1, ra1), m0, m1);
                    q0 = m0;
                    q1 = m1;
                    qp = L2 + 2 * (base / 4 + lane);
                }
            }
        }
    }
    flush();
#if MK_TOP_STAMPS
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_front_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
#endif
}
template __global__ void k_trie_rec_lock_sm<1024>(const uint2*, uint64_t, uint4*, uint4*, uint4*);

// ----------------------------------------------------------------------------
// Deposit trie level: node j = K(in[2j] || (2j+1 < cin ? in[2j+1] : 0^32)),
// the map-miss-reads-zero rule of deposit_trie.go:35-37.
#define MK_TRIE_LEVEL_WAVES 1
__global__ __launch_bounds__(256, MK_TRIE_LEVEL_WAVES) void k_trie_level(const uint4* __restrict__ in, uint64_t cin,
                                                                        uint4* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t cout = (cin + 1) / 2;
    if (j >= cout) return;
    const uint4 l0 = in[4 * j], l1 = in[4 * j + 1];
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
    if (2 * j + 1 < cin) {
        r0 = in[4 * j + 2];
        r1 = in[4 * j + 3];
    }
    uint4 d0, d1;
    hash_pair(l0, l1, r0, r1, false, d0, d1);
    out[2 * j] = d0;
    out[2 * j + 1] = d1;
}

// Batched VerifyMerkleBranch (deposit_trie.go:68-81): thread i folds its
// `depth` siblings into leaf i and compares with root i.
__global__ __launch_bounds__(256) void k_verify_branches(const uint4* __restrict__ leaves, const uint4* __restrict__ branches,
                                                         const uint64_t* __restrict__ indices, uint32_t depth,
                                                         uint32_t tree_depth, const uint4* __restrict__ roots,
                                                         uint64_t n, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t idx = indices[i] + (tree_depth >= 64 ? 0ull : (1ull << tree_depth));
    uint4 v0 = leaves[2 * i], v1 = leaves[2 * i + 1];
    const uint4* br = branches + 2 * (uint64_t)depth * i;
    for (uint32_t d = 0; d < depth; ++d) {
        const uint4 b0 = br[2 * d], b1 = br[2 * d + 1];
        if (idx & 1)
            hash_pair(b0, b1, v0, v1, false, v0, v1);
        else
            hash_pair(v0, v1, b0, b1, false, v0, v1);
        idx >>= 1;
    }
    const uint4 r0 = roots[2 * i], r1 = roots[2 * i + 1];
    ok[i] = (v0.x == r0.x && v0.y == r0.y && v0.z == r0.z && v0.w == r0.w && v1.x == r1.x && v1.y == r1.y &&
             v1.z == r1.z && v1.w == r1.w);
}

// ----------------------------------------------------------------------------
// Synthetic SplitMix64 stream: word k = mix(seed + k*gamma),
// byte b of the stream = byte b%8 (LE) of word b/8.  Writes words
// [word0, word0 + nwords) to dst.  Identical to oracle/merkle_ref.c.
__device__ __forceinline__ uint64_t splitmix(uint64_t seed, uint64_t k) {
    uint64_t z = seed + k * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_synth(uint64_t* __restrict__ dst, uint64_t nwords, uint64_t seed, uint64_t word0) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nwords; k += stride)
        dst[k] = splitmix(seed, word0 + k);
}


// ----------------------------------------------------------------------------
// Incremental deposit trie (UpdateDepositTrie, deposit_trie.go:29-40, for a
// batch of appended leaves): level d0 of the level array already holds the
// new nodes [lo, c) (c = count at d0 after the append).  For every level d0+1
// .. depth the workgroup recomputes the right edge [lo/2, ceil(c/2)) with
// node = K(left || right), a missing right child read as 0^32 (map miss).
// The only child left of the changed range (index lo-1 when lo is odd) is
// old and read from the level array; the changed children are carried from
// level to level in LDS (bit-interleaved lane pairs, mk::ilv).  One
// workgroup, one parent per lane pair: the host keeps c - lo <= NT - 4.
// Level d starts at node trie_level_off(cap, d) = sum_{i<d} ceil(cap/2^i).
template <uint32_t NT>
__global__ __launch_bounds__(NT) void k_trie_append(uint32_t* __restrict__ levels, uint64_t cap, uint32_t d0,
                                                    uint64_t lo, uint64_t c, uint32_t d_end, uint32_t depth,
                                                    uint32_t* __restrict__ root_out) {
    constexpr uint32_t kPairs = NT / 2;
    __shared__ uint32_t lds[2][8 * kPairs];
    const uint32_t tid = threadIdx.x, k = tid >> 1, p = tid & 1u;
    uint64_t off = 0, capd = cap;  // node offset and capacity of level d0
    for (uint32_t i = 0; i < d0; ++i) {
        off += capd;
        capd = (capd + 1) / 2;
    }
    int buf = 0;
    for (uint32_t d = d0; d < d_end; ++d) {
        const uint32_t* cur = levels + 8 * off;
        uint32_t* nxt = levels + 8 * (off + capd);
        const uint64_t plo = lo >> 1, cp = (c + 1) >> 1, np = cp - plo;
        const uint64_t j = plo + k;
        if (k < np) {
            uint32_t a[4], b[4] = {0, 0, 0, 0};
            const uint64_t il = 2 * j, ir = 2 * j + 1;
            if (d == d0 || il < lo)
                load_node3(cur, il, false, p, a);
            else
#pragma unroll
                for (int w = 0; w < 4; ++w) a[w] = lds[buf][8 * (il - lo) + 2 * w + p];
            if (ir < c) {
                if (d == d0)
                    load_node3(cur, ir, false, p, b);
                else
#pragma unroll
                    for (int w = 0; w < 4; ++w) b[w] = lds[buf][8 * (ir - lo) + 2 * w + p];
            }
            uint32_t h[4];
            hash_pair3(a, b, false, p, h);
#pragma unroll
            for (int w = 0; w < 4; ++w) lds[buf ^ 1][8 * k + 2 * w + p] = h[w];
            store_node3(nxt, j, false, p, h);
            if (d + 1 == depth && k == 0) store_node3(root_out, 0, false, p, h);
        }
        __syncthreads();
        buf ^= 1;
        off += capd;
        capd = (capd + 1) / 2;
        lo = plo;
        c = cp;
    }
}
template __global__ void k_trie_append<64>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                           uint32_t*);
template __global__ void k_trie_append<256>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                            uint32_t*);
template __global__ void k_trie_append<1024>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                             uint32_t*);

// The narrow right edge / top of the deposit trie with ONE STATE PER WAVE
// (mk::spread, lo/hi form: ~6.3 k cycles per permutation on a lone wave
// against ~12.8 k for a lane pair, profiles/r02d/lat_probe_spread.json).
// Wave w hashes parent plo + w of every level d0 .. d_end-1 (the host
// guarantees at most NW parents per level); level d0 and the untouched left
// neighbours come from the level array, later children from LDS.  A missing
// right child is 0^32 (deposit_trie.go:33-38), so once the count is 1 the
// levels above are the zero-sibling tail.  GPU lane L holds Keccak lane i
// (mk::spread::lane_consts): lanes i < 8 load the message words (left node
// words 0-3, right node 4-7), i = 8 / 16 carry the 0x01 / 0x80 padding, and
// lanes 0..3 hold the digest.
// Keccak-256 of p[0, la) || 0^lz (a deposit, deposit_trie.go:32; a merkleHash
// window, hash.go:205-222) in spread form: per 136-B block, lane i < 17
// absorbs message word i (0x01 at byte la + lz, 0x80 at byte 135 of the
// last block).
// Result (lo, hi) on the lanes of Keccak lanes 0..3.  W8: p and len are
// 8-byte aligned, so whole words load at once.
template <bool W8>
__device__ __forceinline__ void spread_sponge(const uint8_t* __restrict__ p, uint64_t la, const spread::LaneLH& c,
                                              uint32_t& lo, uint32_t& hi, uint64_t lz = 0) {
    const uint64_t len = la + lz;  // the message is p[0, la) || 0^lz
    const uint64_t nb = len / 136 + 1;
    lo = hi = 0u;
    for (uint64_t b = 0; b < nb; ++b) {  // nb is wave-uniform
        if (c.i < 17u) {
            const uint64_t base = 136 * b + 8 * c.i;
            uint64_t v = 0;
            if (W8 && base + 8 <= la) {
                v = *reinterpret_cast<const uint64_t*>(p + base);
            } else {
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint64_t o = base + k;
                    const uint64_t byte = o < la ? p[o] : 0u;
                    v |= byte << (8 * k);
                }
            }
            if (len >= base && len < base + 8) v |= 1ull << (8 * (len - base));
            if (b + 1 == nb && c.i == 16u) v |= 0x8000000000000000ull;
            lo ^= (uint32_t)v;
            hi ^= (uint32_t)(v >> 32);
        }
        spread::keccak_f_lh(lo, hi, c);
    }
}

template <uint32_t NW>
__global__ __launch_bounds__(64 * NW) void k_trie_spread(uint32_t* __restrict__ levels, uint64_t cap, uint32_t d0,
                                                         uint64_t lo, uint64_t c, uint32_t d_end, uint32_t depth,
                                                         uint32_t* __restrict__ root_out, SpreadLeaves lv) {
    __builtin_amdgcn_s_setprio(kTrieTopPrio);
    __shared__ uint2 lds[2][4 * NW];
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    const spread::LaneLH cst = spread::lane_consts_lh(L);
    const uint32_t i = cst.i;
    if (w < lv.k) {  // wave w hashes new deposit w into level-0 node lo + w (d0 == 0)
        const uint64_t a = lv.offs ? lv.offs[w] : (uint64_t)w * lv.fixed_len;
        const uint64_t len = lv.offs ? lv.offs[w + 1] - a : lv.fixed_len;
        uint32_t hlo, hhi;
        if (lv.aligned8)
            spread_sponge<true>(lv.data + a, len, cst, hlo, hhi);
        else
            spread_sponge<false>(lv.data + a, len, cst, hlo, hhi);
        if (L < 4u) reinterpret_cast<uint2*>(levels)[4 * (lo + w) + L] = make_uint2(hlo, hhi);
    }
    __syncthreads();
    uint64_t off = 0, capd = cap;  // node offset and capacity of level d0
    for (uint32_t k = 0; k < d0; ++k) {
        off += capd;
        capd = (capd + 1) / 2;
    }
    int buf = 0;
    for (uint32_t d = d0; d < d_end; ++d) {
        const uint2* cur = reinterpret_cast<const uint2*>(levels) + 4 * off;
        uint2* nxt = reinterpret_cast<uint2*>(levels) + 4 * (off + capd);
        const uint64_t plo = lo >> 1, cp = (c + 1) >> 1;
        if (w < cp - plo) {  // wave-uniform: the permutation needs every lane
            const uint64_t j = plo + w;
            uint32_t slo = 0u, shi = 0u;
            if (i < 8u) {
                const uint64_t ch = 2 * j + (i >> 2);
                if (ch < c) {
                    const uint2 v = (d == d0 || ch < lo) ? cur[4 * ch + (i & 3u)] : lds[buf][4 * (ch - lo) + (i & 3u)];
                    slo = v.x;
                    shi = v.y;
                }
            }
            if (i == 8u) slo = 1u;
            if (i == 16u) shi = 0x80000000u;
            spread::keccak_f_lh(slo, shi, cst);
            if (L < 4u) {
                const uint2 h = make_uint2(slo, shi);
                lds[buf ^ 1][4 * w + L] = h;
                nxt[4 * j + L] = h;
                if (d + 1 == depth && root_out) reinterpret_cast<uint2*>(root_out)[L] = h;
            }
        }
        __syncthreads();
        buf ^= 1;
        off += capd;
        capd = (capd + 1) / 2;
        lo = plo;
        c = cp;
    }
}
template __global__ void k_trie_spread<1>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                          uint32_t*, SpreadLeaves);
template __global__ void k_trie_spread<2>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                          uint32_t*, SpreadLeaves);
template __global__ void k_trie_spread<4>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                          uint32_t*, SpreadLeaves);
template __global__ void k_trie_spread<16>(uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                                           uint32_t*, SpreadLeaves);

// ONE deposit appended to a trie of `count` (powchain's one log at a time,
// powchain/service.go:379-386 -> UpdateDepositTrie, deposit_trie.go:29-40): the
// leaf hash and its whole path to the root on one wave as a register chain
// (lo/hi spread form).  The path's left siblings (node (count >> d) - 1 of
// level d wherever count >> d is odd; a missing right sibling is 0^32) are all
// loaded into LDS up front, so no level waits on a global load; the new node
// moves to the right half of the next message (Keccak lanes 4..7) with one
// ds_bpermute pair when it is a right child.  Every node of the path is
// stored (GenerateMerkleBranch reads them).  Replaces k_trie_spread<1> for
// k = 1 (one LDS exchange, one dependent load of a sibling and a barrier per
// level there).
__global__ __launch_bounds__(64) void k_trie_append1(uint32_t* __restrict__ levels, uint64_t cap, uint64_t count,
                                                     uint32_t depth, uint32_t* __restrict__ root_out,
                                                     SpreadLeaves lv) {
    __builtin_amdgcn_s_setprio(kTrieTopPrio);
    __shared__ uint2 sib[64][4];
    const uint32_t L = threadIdx.x;
    const spread::LaneLH cst = spread::lane_consts_lh(L);
    const uint32_t i = cst.i;
    const uint2* lv2 = reinterpret_cast<const uint2*>(levels);
    // the path's left siblings, 4 words per level, one word per thread a pass
    for (uint32_t q = L; q < 4 * depth; q += 64) {
        const uint32_t d = q >> 2, w = q & 3u;
        uint64_t off = 0, capd = cap;
        for (uint32_t k = 0; k < d; ++k) {
            off += capd;
            capd = (capd + 1) / 2;
        }
        const uint64_t j = count >> d;
        sib[d][w] = (j & 1u) ? lv2[4 * (off + j - 1) + w] : make_uint2(0, 0);
    }
    uint32_t lo = 0u, hi = 0u;
    const uint64_t len = lv.offs ? lv.offs[1] - lv.offs[0] : lv.fixed_len;
    const uint8_t* dep = lv.data + (lv.offs ? lv.offs[0] : 0);
    if (lv.aligned8)
        spread_sponge<true>(dep, len, cst, lo, hi);
    else
        spread_sponge<false>(dep, len, cst, lo, hi);
    uint2* lvw = reinterpret_cast<uint2*>(levels);
    if (L < 4u) lvw[4 * count + L] = make_uint2(lo, hi);
    __syncthreads();  // the siblings are in LDS
    uint64_t off = 0, capd = cap;
    for (uint32_t d = 0; d < depth; ++d) {
        const uint64_t j = count >> d;
        const bool right = (j & 1u) != 0;  // wave-uniform
        // the node, from the digest lanes (Keccak lanes 0..3 = GPU lanes 0..3)
        // to Keccak lanes 4..7 when it is the right child
        uint32_t rlo = 0u, rhi = 0u;
        if (right) {
            const uint32_t src = 4u * (i >= 4u && i < 8u ? i - 4u : 0u);
            rlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)lo);
            rhi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)hi);
        }
        uint32_t mlo = 0u, mhi = 0u;
        if (i < 4u) {
            const uint2 sv = sib[d][i];
            mlo = right ? sv.x : lo;
            mhi = right ? sv.y : hi;
        } else if (i < 8u && right) {
            mlo = rlo;
            mhi = rhi;
        }
        if (i == 8u) mlo ^= 1u;  // byte 64
        if (i == 16u) mhi ^= 0x80000000u;
        lo = mlo;
        hi = mhi;
        spread::keccak_f_lh(lo, hi, cst);
        off += capd;
        capd = (capd + 1) / 2;
        if (L < 4u) lvw[4 * (off + (j >> 1)) + L] = make_uint2(lo, hi);
    }
    if (L < 4u) reinterpret_cast<uint2*>(root_out)[L] = make_uint2(lo, hi);
}

// fused tops: the arrival counters and every kernel that touches them (k_trie_top_fused, k_merkle_top_fused,
// k_struct_list_fused), k_spread_leaf; no other file names the counters
#include "kernels_top.hip"

// Root() after each of m deposits appended at count0 (powchain's saveInTrie
// reads Root() before every UpdateDepositTrie, service.go:379-386): wave g
// walks leaf i = count0 + g to the top in spread form.  At level d the path
// node p = i >> d is a right child (p odd: its left sibling p - 1 covers only
// leaves < i, a complete subtree, so the level array holds its final value)
// or a left child (the right sibling lies past the prefix: 0^32), so the m
// prefix roots are m independent 32-permutation chains over the level array
// the batched append left behind.  The left siblings of a chain go to LDS
// first (lane d loads level d's), then the chain runs with no global loads.
template <uint32_t NW>
__global__ __launch_bounds__(64 * NW) void k_trie_prefix_roots(const uint4* __restrict__ levels, uint64_t cap,
                                                               uint64_t count0, uint64_t m, uint32_t depth,
                                                               uint4* __restrict__ roots) {
    __shared__ uint4 sib[NW][64][2];
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    const uint64_t g = (uint64_t)blockIdx.x * NW + w;
    const bool live = g < m;  // wave-uniform
    const uint64_t i = count0 + (live ? g : 0);
    if (live && L < depth && ((i >> L) & 1u)) {
        uint64_t off = 0, capd = cap;
        for (uint32_t d = 0; d < L; ++d) {
            off += capd;
            capd = (capd + 1) / 2;
        }
        const uint64_t node = off + (i >> L) - 1;
        sib[w][L][0] = levels[2 * node];
        sib[w][L][1] = levels[2 * node + 1];
    }
    __syncthreads();
    if (!live) return;
    const spread::LaneLH cst = spread::lane_consts_lh(L);
    const uint32_t ci = cst.i;
    uint32_t plo = 0u, phi = 0u;  // the path node's word ci on lanes ci < 4
    if (ci < 4u) {
        const uint2 v = reinterpret_cast<const uint2*>(levels)[4 * i + ci];
        plo = v.x;
        phi = v.y;
    }
    for (uint32_t d = 0; d < depth; ++d) {
        const bool right = ((i >> d) & 1u) != 0;  // wave-uniform
        // path words moved to Keccak lanes 4..7 (GPU lanes 0..3 hold 0..3)
        const uint32_t src = 4u * ((ci - 4u) & 3u);
        const uint32_t mlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)plo);
        const uint32_t mhi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)phi);
        uint32_t lo = 0u, hi = 0u;
        if (ci < 4u) {
            if (right) {
                const uint4 h = sib[w][d][ci >> 1];
                lo = (ci & 1u) ? h.z : h.x;
                hi = (ci & 1u) ? h.w : h.y;
            } else {
                lo = plo;
                hi = phi;
            }
        } else if (ci < 8u && right) {
            lo = mlo;
            hi = mhi;
        } else if (ci == 8u) {
            lo = 1u;
        }
        if (ci == 16u) hi = 0x80000000u;
        spread::keccak_f_lh(lo, hi, cst);
        plo = lo;
        phi = hi;
    }
    if (L < 4u) reinterpret_cast<uint2*>(roots)[4 * g + L] = make_uint2(plo, phi);
}
template __global__ void k_trie_prefix_roots<4>(const uint4*, uint64_t, uint64_t, uint64_t, uint32_t, uint4*);

// GenerateMerkleBranch (deposit_trie.go:43-58): branch[d] = the sibling of
// index's ancestor at level d, 0^32 when that node does not exist.
__global__ void k_trie_branch(const uint4* __restrict__ levels, uint64_t cap, uint64_t count, uint32_t depth,
                              uint64_t index, uint4* __restrict__ branch) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= depth) return;
    uint64_t off = 0, capd = cap, cd = count;
    for (uint32_t i = 0; i < d; ++i) {
        off += capd;
        capd = (capd + 1) / 2;
        cd = (cd + 1) / 2;
    }
    const uint64_t sib = (index >> d) ^ 1ull;
    uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
    if (sib < cd) {
        v0 = levels[2 * (off + sib)];
        v1 = levels[2 * (off + sib) + 1];
    }
    branch[2 * d] = v0;
    branch[2 * d + 1] = v1;
}

// GenerateMerkleBranch for k indices, and Root(), AS OF a past deposit count
// c = as_of <= count: what the reference's trie answered right after its c-th
// UpdateDepositTrie (deposit_trie.go:29-63), from the level array the later
// appends left behind.  The trie is append-only, so a node whose leaves all
// lie below c still holds its value of that moment, a node whose leaves all
// lie at or above c did not exist (0^32, the map miss), and per level only the
// ancestor of leaf c - 1 can straddle c.  Those straddling nodes E_d are one
// dependent chain: with p = (c - 1) >> d, E_{d+1} = K(level_d[p - 1] || E_d)
// for odd p, else K(E_d || 0^32).  Level d straddles iff 2^d does not divide c
// (and count > c), so the chain starts from the stored node of level
// d0 - 1 = ctz(c) and is empty when c == count.
// Every workgroup runs the chain itself, on wave 0 in spread form with the left
// siblings prefetched into LDS (the walk of k_trie_prefix_roots), so nothing
// is handed from one workgroup to another; then each wave writes one branch
// per turn as one contiguous block: lane pair (2d, 2d + 1) takes the two 16-B
// halves of level d's sibling s = (index >> d) ^ 1, which is 0^32 for s > p,
// E_d for s == p on a straddling level, the stored node otherwise.
__global__ __launch_bounds__(64 * kBranchWaves) void k_trie_branches_at(
    const uint4* __restrict__ levels, uint64_t cap, uint64_t count, uint64_t as_of, uint32_t depth,
    const uint64_t* __restrict__ indices, uint64_t k, uint4* __restrict__ branches, uint4* __restrict__ root_at) {
    __shared__ uint4 sib[64][2];    // chain: level d's left sibling
    __shared__ uint4 edge[64][2];   // E_d for d0 <= d <= depth
    __shared__ uint64_t lvoff[64];  // first node of level d in the level array
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    const uint64_t c = as_of, last = c - 1;
    const bool chain = c != 0 && count > c && (uint32_t)__ffsll((long long)c) <= depth;  // block-uniform
    const uint32_t d0 = chain ? (uint32_t)__ffsll((long long)c) : 64u;  // lowest straddling level
    if (L <= depth && (w == 0 ? chain : w == 1)) {
        uint64_t off = 0, capd = cap;
        for (uint32_t d = 0; d < L; ++d) {
            off += capd;
            capd = (capd + 1) / 2;
        }
        if (w == 1) {
            lvoff[L] = off;
        } else if (L + 1 >= d0 && L < depth && ((last >> L) & 1u)) {
            const uint64_t node = off + (last >> L) - 1;
            sib[L][0] = levels[2 * node];
            sib[L][1] = levels[2 * node + 1];
        }
    }
    __syncthreads();
    if (w == 0 && chain) {
        const spread::LaneLH cst = spread::lane_consts_lh(L);
        const uint32_t ci = cst.i;
        uint32_t plo = 0u, phi = 0u;  // the path node's word ci on lanes ci < 4
        if (ci < 4u) {
            const uint2 v = reinterpret_cast<const uint2*>(levels)[4 * (lvoff[d0 - 1] + (last >> (d0 - 1))) + ci];
            plo = v.x;
            phi = v.y;
        }
        for (uint32_t d = d0 - 1; d < depth; ++d) {
            const bool right = ((last >> d) & 1u) != 0;  // wave-uniform
            // path words moved to Keccak lanes 4..7 (GPU lanes 0..3 hold 0..3)
            const uint32_t src = 4u * ((ci - 4u) & 3u);
            const uint32_t mlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)plo);
            const uint32_t mhi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)phi);
            uint32_t lo = 0u, hi = 0u;
            if (ci < 4u) {
                if (right) {
                    const uint4 h = sib[d][ci >> 1];
                    lo = (ci & 1u) ? h.z : h.x;
                    hi = (ci & 1u) ? h.w : h.y;
                } else {
                    lo = plo;
                    hi = phi;
                }
            } else if (ci < 8u && right) {
                lo = mlo;
                hi = mhi;
            } else if (ci == 8u) {
                lo = 1u;
            }
            if (ci == 16u) hi = 0x80000000u;
            spread::keccak_f_lh(lo, hi, cst);
            plo = lo;
            phi = hi;
            if (L < 4u) reinterpret_cast<uint2*>(&edge[d + 1][0])[L] = make_uint2(lo, hi);
        }
    }
    __syncthreads();
    if (root_at && blockIdx.x == 0 && threadIdx.x < 2u) {  // E_depth; the stored root when no level straddles
        uint4 r = make_uint4(0, 0, 0, 0);
        if (chain)
            r = edge[depth][threadIdx.x];
        else if (c != 0)
            r = levels[2 * lvoff[depth] + threadIdx.x];
        root_at[threadIdx.x] = r;
    }
    const uint64_t stride = (uint64_t)gridDim.x * kBranchWaves;
    for (uint64_t g = (uint64_t)blockIdx.x * kBranchWaves + w; g < k; g += stride) {
        const uint64_t index = indices[g];
        for (uint32_t q = L; q < 2 * depth; q += 64) {
            const uint32_t d = q >> 1, h = q & 1u;
            const uint64_t s = (index >> d) ^ 1ull, p = last >> d;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (c != 0 && s <= p) v = (s == p && d >= d0) ? edge[d][h] : levels[2 * (lvoff[d] + s) + h];
            branches[2 * (uint64_t)depth * g + q] = v;
        }
    }
}

// verifyDeposit for a batch (core/blocks/block_operations.go:624-641): thread
// i hashes deposit data i = data[offs[i], offs[i+1]) into its leaf (the sponge
// of k_keccak_var), folds its `depth` siblings into it (the fold of
// k_verify_branches) and compares with the batch's one root (root_stride == 0:
// a block's deposits against the state's deposit root) or with root i
// (root_stride == 32).
__global__ __launch_bounds__(256) void k_verify_deposits(const uint8_t* __restrict__ data,
                                                         const uint64_t* __restrict__ offs,
                                                         const uint4* __restrict__ branches,
                                                         const uint64_t* __restrict__ indices, uint32_t depth,
                                                         uint32_t tree_depth, const uint4* __restrict__ roots,
                                                         uint32_t root_stride, uint64_t n,
                                                         uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = offs[i], b = offs[i + 1];
    uint4 v0, v1;
    sponge_generic(data + a, b - a, 0, false, 0, v0, v1);
    uint64_t idx = indices[i] + (tree_depth >= 64 ? 0ull : (1ull << tree_depth));
    const uint4* br = branches + 2 * (uint64_t)depth * i;
    for (uint32_t d = 0; d < depth; ++d) {
        const uint4 b0 = br[2 * d], b1 = br[2 * d + 1];
        if (idx & 1)
            hash_pair(b0, b1, v0, v1, false, v0, v1);
        else
            hash_pair(v0, v1, b0, b1, false, v0, v1);
        idx >>= 1;
    }
    const uint4* rt = roots + (root_stride ? 2 * i : 0);
    const uint4 r0 = rt[0], r1 = rt[1];
    ok[i] = (v0.x == r0.x && v0.y == r0.y && v0.z == r0.z && v0.w == r0.w && v1.x == r1.x && v1.y == r1.y &&
             v1.z == r1.z && v1.w == r1.w);
}

// ----------------------------------------------------------------------------
// Many lists (segmented merkleHash, hash.go:194-239 per list): one launch per
// level for all lists with nodes at that level.  Thread t of the launch maps
// to (list, node j) by binary search over the level's act table (exclusive
// prefix sums of the per-list node counts).  LEAF: node j = K(window j of the
// list's chunks) (256-B contiguous windows on the streaming path, the generic
// sponge for odd item sizes and ragged / padded windows); NODE: K(n[2j] ||
// n[2j+1]) or K(n[2j] || 0^128) on an odd count.
__device__ __forceinline__ uint32_t many_find(const ManyAct* __restrict__ act, uint32_t cnt, uint64_t t) {
    uint32_t lo = 0, hi = cnt;  // act[lo].out_first <= t < act[hi].out_first
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (act[mid].out_first <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <bool LEAF>
__global__ __launch_bounds__(256) void k_many_level(const uint8_t* __restrict__ items,
                                                    const ManyList* __restrict__ lists,
                                                    const ManyAct* __restrict__ act, uint32_t nact, uint64_t nodes,
                                                    const uint4* __restrict__ in, uint4* __restrict__ out,
                                                    uint4* __restrict__ tops) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nodes) return;
    const ManyAct A = act[many_find(act, nact, t)];
    const ManyList L = lists[A.list];
    const uint64_t j = t - A.out_first;
    uint4 d0, d1;
    if constexpr (LEAF) {
        const uint8_t* base = items + L.items_off;
        if (L.fast && j < L.total / 256) {
            hash_window256(reinterpret_cast<const uint4*>(base) + j * 16, d0, d1);
        } else {
            const uint64_t lo = j * 2 * L.cb;
            uint64_t la;
            uint32_t lz;
            if (2 * j + 1 < L.nchunks) {
                la = (lo + 2 * L.cb < L.total ? lo + 2 * L.cb : L.total) - lo;
                lz = 0;
            } else {
                la = L.total - lo;
                lz = 128;
            }
            sponge_generic(base + lo, la, lz, false, 0, d0, d1);
        }
    } else {
        const uint64_t cprev = (L.c1 + (1ull << (A.level - 2)) - 1) >> (A.level - 2);  // nodes at level - 1
        const uint4* src = in + 2 * (A.in_first + 2 * j);
        const bool padded = !(2 * j + 1 < cprev);
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
        if (!padded) {
            r0 = src[2];
            r1 = src[3];
        }
        hash_pair(src[0], src[1], r0, r1, padded, d0, d1);
    }
    if (A.level == L.levels) {  // the list's top node (its only node at this level)
        tops[2 * A.list] = d0;
        tops[2 * A.list + 1] = d1;
    } else {
        out[2 * (A.out_first + j)] = d0;
        out[2 * (A.out_first + j) + 1] = d1;
    }
}
template __global__ void k_many_level<true>(const uint8_t*, const ManyList*, const ManyAct*, uint32_t, uint64_t,
                                            const uint4*, uint4*, uint4*);
template __global__ void k_many_level<false>(const uint8_t*, const ManyList*, const ManyAct*, uint32_t, uint64_t,
                                             const uint4*, uint4*, uint4*);

// Root of every list that is not a big list: K(top || le64(n) || 0^24), or
// for <= 1 chunk K(bytes || [0^128 if n == 0] || le64(n) || 0^24).
__global__ __launch_bounds__(256) void k_many_final(const uint8_t* __restrict__ items,
                                                    const ManyList* __restrict__ lists, uint32_t nlists,
                                                    const uint4* __restrict__ tops, uint4* __restrict__ roots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlists) return;
    const ManyList L = lists[i];
    if (L.levels == 0xFFFFFFFFu) return;  // big list: its own plan wrote the root
    uint4 d0, d1;
    if (L.levels == 0) {
        sponge_generic(items + L.items_off, L.total, L.n == 0 ? 128u : 0u, true, L.n, d0, d1);
    } else {
        hash_final(tops[2 * i], tops[2 * i + 1], L.n, d0, d1);
    }
    roots[2 * i] = d0;
    roots[2 * i + 1] = d1;
}

}  // namespace mk

// the resident trees: a file of their own, built in this translation unit ("Kernel files")
#include "kernels_tree.hip"
// the deposit trie's roll back, fork point, audit and copy; after kernels_tree.hip: its audit helpers
#include "kernels_trie_admin.hip"
// records with list fields; k_struct_nested's column helpers
#include "kernels_struct_list.hip"
// hashutil.RepeatHash in batches: chains, onions, the RANDAO check
#include "kernels_repeat.hip"
