// hashutil.RepeatHash (hash.go:29-34) in batches: chains, hash onions and the RANDAO check of
// verifyBlockRandao (block_operations.go:109-123) against records in HBM (the helpers:
// repeat_dev.hpp).  A part of the one kernel translation unit: merkle_kernels.hip includes it last.  Built as an
// object of its own it would emit other code for the same text ("Kernel files").
#ifndef MK_KERNEL_UNIT
#error "kernels_repeat.hip is built through merkle_kernels.hip"
#endif

#include "repeat_dev.hpp"

namespace mk {

// A chain is Keccak-256 of its own 32-B digest, over and over: the state never leaves registers and nothing is
// read or written between two permutations (the onion stores each layer, and waits for nothing).  Two forms do
// the same three jobs (RepeatMode):
//   chain   out[i] = RepeatHash(seeds[i], layers[i]); 0 layers copy the seed
//   onion   out[i][t] = RepeatHash(seeds[i], t), t = 0 .. max_layers, row t stored as layer t completes
//   verify  out[i] = RepeatHash(seeds[i], le64(rec + layers_off)) == rec[commit_off, +32), rec = record idx[i]
// No input makes a chain run more than max_layers permutations: a trip count above it is never entered (chain:
// 32 zero bytes and the status word; verify: verdict 2, the 64-bit count compared whole; index past the
// records: verdict 3), and the host refuses max_layers > MK_REPEAT_MAX_LAYERS.

// One chain per GPU lane: the per-lane State (50 VGPRs), plain round 0, the digest-only last round in every
// iteration (the re-pad overwrites lanes 4..24).  The layer loop is rolled, so the kernel holds one
// permutation's code.  The trip count is PER LANE: a wave runs for as long as its longest chain and the lanes
// of shorter chains sit masked off; nothing here is phase-locked (a locked form needs equal trip counts in the
// whole workgroup).
template <int MODE>
__global__ __launch_bounds__(kRepeatThreads) void k_repeat_lane(RepeatArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kRepeatThreads + threadIdx.x;
    if (i >= a.n) return;
    const bool io16 = a.io16 != 0, rec4 = a.rec4 != 0;
    uint32_t T = a.max_layers;
    const uint8_t* rec = nullptr;
    State s;
    if constexpr (MODE == kRepeatChain) {
        T = a.layers[i];
        if (T > a.max_layers) {
#pragma unroll
            for (int w = 0; w < 4; ++w) s.lo[w] = s.hi[w] = 0u;
            rep::st_digest(s, a.out + 32 * i, io16);
            if (a.status) atomicOr(a.status, 1u);
            return;
        }
    }
    if constexpr (MODE == kRepeatVerify) {
        const uint64_t r = a.idx[i];
        if (r >= a.n_records) {
            a.out[i] = rep::kNoRecord;
            return;
        }
        rec = a.records + r * a.stride;
        if (!rep::layers_ok(rep::ld_word(rec + a.layers_off, rec4), a.max_layers, T)) {
            a.out[i] = rep::kTooDeep;
            return;
        }
    }
    rep::ld_digest(s, a.seeds + 32 * i, io16);
    uint8_t* row = nullptr;
    if constexpr (MODE == kRepeatOnion) {
        row = a.out + 32 * i * ((uint64_t)T + 1);
        rep::st_digest(s, row, io16);
    }
#pragma unroll 1
    for (uint32_t t = 0; t < T; ++t) {
        rep::repad(s);
        keccak_f_digest(s);
        if constexpr (MODE == kRepeatOnion) {
            row += 32;
            rep::st_digest(s, row, io16);
        }
    }
    if constexpr (MODE == kRepeatChain) rep::st_digest(s, a.out + 32 * i, io16);
    if constexpr (MODE == kRepeatVerify) {
        bool eq = true;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint2 c = rep::ld_word(rec + a.commit_off + 8 * w, rec4);
            eq = eq && c.x == s.lo[w] && c.y == s.hi[w];
        }
        a.out[i] = eq ? rep::kOk : rep::kBad;
    }
}

// One chain per wave, for few chains: the wave-spread permutation on lo/hi halves (spread::keccak_f_lh, the
// faster of the two spread forms on a lone wave, DESIGN.md section 4.5, and its digest is plain 64-bit words: no
// bit (de)interleave at either end).  GPU lane L holds Keccak lane c.i; between two permutations a lane keeps
// its word when c.i < 4 and takes the pad constant otherwise (rep::repad, two v_bitop3).  The digest is on
// lanes 0..3.  Everything a branch depends on is the same in all 64 lanes (the chain index, its trip count,
// its record), so the DPP moves and swaps of the rounds always run with the whole wave on.
template <int MODE>
__global__ __launch_bounds__(kRepeatThreads) void k_repeat_wave(RepeatArgs a) {
    const uint32_t L = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kRepeatWaves + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const bool io8 = a.io16 != 0, rec4 = a.rec4 != 0;
    uint32_t T = a.max_layers;
    const uint8_t* rec = nullptr;
    if constexpr (MODE == kRepeatChain) {
        T = a.layers[i];
        if (T > a.max_layers) {
            if (L < 4u) rep::st_word(a.out + 32 * i + 8 * L, make_uint2(0u, 0u), io8);
            if (L == 0u && a.status) atomicOr(a.status, 1u);
            return;
        }
    }
    if constexpr (MODE == kRepeatVerify) {
        const uint64_t r = a.idx[i];
        if (r >= a.n_records) {
            if (L == 0u) a.out[i] = rep::kNoRecord;
            return;
        }
        rec = a.records + r * a.stride;
        if (!rep::layers_ok(rep::ld_word(rec + a.layers_off, rec4), a.max_layers, T)) {
            if (L == 0u) a.out[i] = rep::kTooDeep;
            return;
        }
    }
    T = (uint32_t)__builtin_amdgcn_readfirstlane((int)T);
    const spread::LaneLH cst = spread::lane_consts_lh(L);
    const rep::SpreadPad pad = rep::spread_pad(cst.i);
    uint32_t lo = 0u, hi = 0u;
    if (cst.i < 4u) {
        const uint2 v = rep::ld_word(a.seeds + 32 * i + 8 * cst.i, io8);
        lo = v.x;
        hi = v.y;
    }
    uint8_t* row = nullptr;
    if constexpr (MODE == kRepeatOnion) {
        row = a.out + 32 * i * ((uint64_t)T + 1) + 8 * L;
        if (L < 4u) rep::st_word(row, make_uint2(lo, hi), io8);
    }
#pragma unroll 1
    for (uint32_t t = 0; t < T; ++t) {
        rep::repad(lo, hi, pad);
        spread::keccak_f_lh(lo, hi, cst);
        if constexpr (MODE == kRepeatOnion) {
            row += 32;
            if (L < 4u) rep::st_word(row, make_uint2(lo, hi), io8);
        }
    }
    if constexpr (MODE == kRepeatChain) {
        if (L < 4u) rep::st_word(a.out + 32 * i + 8 * L, make_uint2(lo, hi), io8);
    }
    if constexpr (MODE == kRepeatVerify) {
        bool ne = false;
        if (L < 4u) {
            const uint2 c = rep::ld_word(rec + a.commit_off + 8 * L, rec4);
            ne = c.x != lo || c.y != hi;
        }
        const bool bad = __ballot(ne) != 0;
        if (L == 0u) a.out[i] = bad ? rep::kBad : rep::kOk;
    }
}

template __global__ void k_repeat_lane<kRepeatChain>(RepeatArgs);
template __global__ void k_repeat_lane<kRepeatOnion>(RepeatArgs);
template __global__ void k_repeat_lane<kRepeatVerify>(RepeatArgs);
template __global__ void k_repeat_wave<kRepeatChain>(RepeatArgs);
template __global__ void k_repeat_wave<kRepeatOnion>(RepeatArgs);
template __global__ void k_repeat_wave<kRepeatVerify>(RepeatArgs);

}  // namespace mk
