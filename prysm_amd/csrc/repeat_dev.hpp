// hashutil.RepeatHash (hash.go:29-34) on the device: what both forms of kernels_repeat.hip share and no launch
// shape enters.  One iteration is Keccak-256 of a 32-B message: Keccak lanes 0..3 are the
// previous digest, lane 4 is the 0x01 domain byte, lane 16 the 0x80 << 56 closing bit, every other lane zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keccak_dev.hpp"

namespace mk {
namespace rep {

// ---- the re-pad between two permutations -------------------------------------------------------------
// One state per GPU lane: lanes 4..24 are overwritten, never read, so whatever the digest-only last round
// (keccak_f_digest) left there is dead and that round is legal in every iteration.
__device__ __forceinline__ void repad(State& s) {
#pragma unroll
    for (int i = 4; i < 25; ++i) {
        s.lo[i] = 0u;
        s.hi[i] = 0u;
    }
    s.lo[4] = 1u;
    s.hi[16] = 0x80000000u;
}

// One state per wave (mk::spread, lo/hi halves): a GPU lane keeps its word when its Keccak lane index is below 4
// and takes the pad constant otherwise.  The rule goes by the lane's c.i, so the repeats of a row (positions
// 5..7) and the mirrors of row 4 (groups 5..7) get what their canonical lane gets.
struct SpreadPad {
    uint32_t keep;  // all-ones on the lanes of Keccak lanes 0..3
    uint32_t lo;    // 1 on the lanes of Keccak lane 4
    uint32_t hi;    // 0x80000000 on the lanes of Keccak lane 16
};
__device__ __forceinline__ SpreadPad spread_pad(uint32_t ci) {
    SpreadPad p;
    p.keep = ci < 4u ? 0xFFFFFFFFu : 0u;
    p.lo = ci == 4u ? 1u : 0u;
    p.hi = ci == 16u ? 0x80000000u : 0u;
    return p;
}
__device__ __forceinline__ void repad(uint32_t& lo, uint32_t& hi, const SpreadPad& p) {
    lo = spread::sel(p.keep, lo, p.lo);
    hi = spread::sel(p.keep, hi, p.hi);
}

// ---- loads and stores at any alignment ----------------------------------------------------------------
// `wide`: the address is a multiple of the access (4 B for a dword, 8 B for a word); else byte by byte.
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p, bool wide) {
    if (wide) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// little-endian 64-bit word as (lo, hi); wide: 4-B aligned
__device__ __forceinline__ uint2 ld_word(const uint8_t* p, bool wide) {
    return make_uint2(ld_u32(p, wide), ld_u32(p + 4, wide));
}
__device__ __forceinline__ void st_word(uint8_t* p, uint2 v, bool wide) {
    if (wide) {
        reinterpret_cast<uint32_t*>(p)[0] = v.x;
        reinterpret_cast<uint32_t*>(p)[1] = v.y;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k] = (uint8_t)(v.x >> (8 * k));
        p[4 + k] = (uint8_t)(v.y >> (8 * k));
    }
}

// 32 bytes into / out of Keccak lanes 0..3 of a per-lane state; wide16: 16-B aligned, else byte by byte
__device__ __forceinline__ void ld_digest(State& s, const uint8_t* p, bool wide16) {
    if (wide16) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        s.lo[0] = a.x, s.hi[0] = a.y, s.lo[1] = a.z, s.hi[1] = a.w;
        s.lo[2] = b.x, s.hi[2] = b.y, s.lo[3] = b.z, s.hi[3] = b.w;
        return;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint2 v = ld_word(p + 8 * w, false);
        s.lo[w] = v.x;
        s.hi[w] = v.y;
    }
}
__device__ __forceinline__ void st_digest(const State& s, uint8_t* p, bool wide16) {
    if (wide16) {
        uint4 a, b;
        digest(s, a, b);
        reinterpret_cast<uint4*>(p)[0] = a;
        reinterpret_cast<uint4*>(p)[1] = b;
        return;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) st_word(p + 8 * w, make_uint2(s.lo[w], s.hi[w]), false);
}

// ---- the verdict of a verify -------------------------------------------------------------------------
// MK_REPEAT_OK / _BAD / _TOO_DEEP / _NO_RECORD of prysm_merkle.h
constexpr uint8_t kBad = 0, kOk = 1, kTooDeep = 2, kNoRecord = 3;

// The layer count of a record is 64 bits of data: it is compared whole, and only a count that passed is
// narrowed (max_layers fits 32 bits).  false: the chain is not run.
__device__ __forceinline__ bool layers_ok(uint2 cnt, uint32_t max_layers, uint32_t& layers) {
    layers = cnt.x;
    return cnt.y == 0u && cnt.x <= max_layers;
}

}  // namespace rep
}  // namespace mk
