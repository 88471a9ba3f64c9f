// Device helpers shared by the kernel files: the byte sponge, the 64-B node hash, the length mix-in.
#ifndef MK_HASH_DEV_HPP
#define MK_HASH_DEV_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keccak_dev.hpp"
#include "merkle_kernels.hpp"

// Diagnostic build only (tools/top_probe.hip: -DMK_TOP_STAMPS=1): in-kernel time stamps; never in the shipped library.
#ifndef MK_TOP_STAMPS
#define MK_TOP_STAMPS 0
#endif

namespace mk {

// ----------------------------------------------------------------------------
// Generic byte-addressed sponge (edge windows, odd sizes, var-len messages).
// Message = A (global bytes [p, p+la)) || 0^lz || (lenc ? le64(nval)||0^24 : -)
__device__ inline __noinline__ void sponge_generic(const uint8_t* __restrict__ p, uint64_t la, uint32_t lz,
                                            bool lenc, uint64_t nval, uint4& d0, uint4& d1) {
    const uint64_t len = la + lz + (lenc ? 32u : 0u);
    const uint64_t nb = len / 136 + 1;
    const bool aligned = (((uintptr_t)p) & 7u) == 0;
    State s;
    zero(s);
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t base = b * 136;
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            const uint64_t m0 = base + 8u * w;
            uint32_t lo = 0, hi = 0;
            if (aligned && m0 + 8 <= la) {
                const uint2 v = *reinterpret_cast<const uint2*>(p + m0);
                lo = v.x;
                hi = v.y;
            } else if (m0 < len) {
#pragma unroll 1
                for (int k = 0; k < 8; ++k) {
                    const uint64_t m = m0 + k;
                    uint32_t byte = 0;
                    if (m < la) {
                        byte = p[m];
                    } else if (m >= la + lz && m < len) {
                        const uint64_t e = m - la - lz;  // lenc byte
                        byte = e < 8 ? (uint32_t)((nval >> (8 * e)) & 0xFF) : 0u;
                    }
                    if (k < 4)
                        lo |= byte << (8 * k);
                    else
                        hi |= byte << (8 * (k - 4));
                }
            }
            if (m0 <= len && len < m0 + 8) {  // domain pad byte 0x01
                const uint32_t k = (uint32_t)(len - m0);
                if (k < 4)
                    lo ^= 1u << (8 * k);
                else
                    hi ^= 1u << (8 * (k - 4));
            }
            if (b == nb - 1 && w == 16) hi ^= 0x80000000u;
            s.lo[w] ^= lo;
            s.hi[w] ^= hi;
        }
        keccak_f(s);
    }
    digest(s, d0, d1);
}

// K(L || R) (64 B, 1 permutation) or K(L || 0^128) (160 B, 2 permutations);
// `padded` may differ between lanes (the block-1 permutation then diverges).
// The final permutation computes only the digest lanes (keccak_f_digest).
__device__ __forceinline__ void hash_pair(uint4 l0, uint4 l1, uint4 r0, uint4 r1, bool padded,
                                          uint4& d0, uint4& d1) {
    State s;
    zero(s);
    xor_lane(s, 0, make_uint2(l0.x, l0.y));
    xor_lane(s, 1, make_uint2(l0.z, l0.w));
    xor_lane(s, 2, make_uint2(l1.x, l1.y));
    xor_lane(s, 3, make_uint2(l1.z, l1.w));
    if (!padded) {
        xor_lane(s, 4, make_uint2(r0.x, r0.y));
        xor_lane(s, 5, make_uint2(r0.z, r0.w));
        xor_lane(s, 6, make_uint2(r1.x, r1.y));
        xor_lane(s, 7, make_uint2(r1.z, r1.w));
    }
    if (padded) keccak_f(s);  // block 1 = L || 0^104; block 2 = 0^24 || padding
    if (padded)
        s.lo[3] ^= 1u;  // byte 160 = byte 24 of block 1
    else
        s.lo[8] ^= 1u;  // byte 64
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, d0, d1);
}

// K(root || le64(n) || 0^24)
__device__ __forceinline__ void hash_final(uint4 r0, uint4 r1, uint64_t n, uint4& d0, uint4& d1) {
    State s;
    zero(s);
    xor_lane(s, 0, make_uint2(r0.x, r0.y));
    xor_lane(s, 1, make_uint2(r0.z, r0.w));
    xor_lane(s, 2, make_uint2(r1.x, r1.y));
    xor_lane(s, 3, make_uint2(r1.z, r1.w));
    xor_lane(s, 4, make_uint2((uint32_t)n, (uint32_t)(n >> 32)));
    s.lo[8] ^= 1u;
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, d0, d1);
}

}  // namespace mk
#endif
