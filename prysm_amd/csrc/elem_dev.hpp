// Element digests K(le32(len) || element) shared by the list, struct and resident-tree kernels.
#ifndef MK_ELEM_DEV_HPP
#define MK_ELEM_DEV_HPP
#include "hash_dev.hpp"

namespace mk {

// K(le32(32) || e), e = 32 B at a 16-B aligned address: one block.
__device__ __forceinline__ void elem32_digest(const uint4* __restrict__ e, uint32_t (&d)[8]) {
    asm volatile("" ::: "memory");  // the loads stay here (not hoisted over earlier permutations)
    const uint4 v0 = ld_stream(e), v1 = ld_stream(e + 1);
    State s;
    s.lo[0] = 32u;  // le32(len)
    s.hi[0] = v0.x;
    s.lo[1] = v0.y;
    s.hi[1] = v0.z;
    s.lo[2] = v0.w;
    s.hi[2] = v1.x;
    s.lo[3] = v1.y;
    s.hi[3] = v1.z;
    s.lo[4] = v1.w;
    s.hi[4] = 1u;  // domain pad at byte 36
#pragma unroll
    for (int k = 5; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
    s.hi[16] = 0x80000000u;
    keccak_f_digest(s);
    d[0] = s.lo[0];
    d[1] = s.hi[0];
    d[2] = s.lo[1];
    d[3] = s.hi[1];
    d[4] = s.lo[2];
    d[5] = s.hi[2];
    d[6] = s.lo[3];
    d[7] = s.hi[3];
}

// Keccak(le32(L) || A[0, L)) with 32-bit loads (A 4-byte aligned).
__device__ inline __noinline__ void sponge_prefix4(const uint8_t* __restrict__ A, uint32_t L, uint4& d0, uint4& d1) {
    const uint32_t* A32 = reinterpret_cast<const uint32_t*>(A);
    const uint32_t len = L + 4;
    const uint32_t nb = len / 136 + 1;
    State s;
    zero(s);
    for (uint32_t b = 0; b < nb; ++b) {
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            const uint32_t m0 = b * 136 + 8u * w;  // message byte of this word
            uint32_t half[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t m = m0 + 4u * h;  // 4-byte group [m, m+4) of the message
                uint32_t v = 0;
                if (m == 0) {
                    v = L;
                } else if (m + 4 <= len) {
                    v = A32[(m - 4) / 4];
                } else if (m < len) {
                    for (uint32_t k = 0; k < len - m; ++k) v |= (uint32_t)A[m - 4 + k] << (8 * k);
                }
                if (m <= len && len < m + 4) v ^= 1u << (8 * (len - m));  // pad 0x01
                half[h] = v;
            }
            if (b == nb - 1 && w == 16) half[1] ^= 0x80000000u;
            s.lo[w] ^= half[0];
            s.hi[w] ^= half[1];
        }
        keccak_f(s);
    }
    digest(s, d0, d1);
}

// K(le32(L) || p[0, L)) for any length and alignment (byte loads).
__device__ inline __noinline__ void elem_digest_any(const uint8_t* __restrict__ p, uint32_t L, uint32_t (&d)[8]) {
    uint4 d0, d1;
    if ((((uintptr_t)p) & 3u) == 0) {
        sponge_prefix4(p, L, d0, d1);
    } else {
        const uint64_t len = (uint64_t)L + 4;
        const uint64_t nb = len / 136 + 1;
        State s;
        zero(s);
        for (uint64_t b = 0; b < nb; ++b) {
#pragma unroll 1
            for (int w = 0; w < 17; ++w) {
                uint32_t h[2] = {0u, 0u};
#pragma unroll 1
                for (int k = 0; k < 8; ++k) {
                    const uint64_t m = b * 136 + 8u * w + k;
                    uint32_t byte = 0;
                    if (m < 4)
                        byte = (L >> (8 * m)) & 0xFFu;
                    else if (m < len)
                        byte = p[m - 4];
                    else if (m == len)
                        byte = 1u;  // domain pad
                    h[k >> 2] |= byte << (8 * (k & 3));
                }
                if (b == nb - 1 && w == 16) h[1] ^= 0x80000000u;
                s.lo[w] ^= h[0];
                s.hi[w] ^= h[1];
            }
            keccak_f(s);
        }
        digest(s, d0, d1);
    }
    d[0] = d0.x, d[1] = d0.y, d[2] = d0.z, d[3] = d0.w;
    d[4] = d1.x, d[5] = d1.y, d[6] = d1.z, d[7] = d1.w;
}

}  // namespace mk
#endif
