// Lane-pair (mk::ilv) node helpers shared by the latency-bound kernels and the resident trees.
#ifndef MK_SPREAD3_DEV_HPP
#define MK_SPREAD3_DEV_HPP
#include "hash_dev.hpp"

namespace mk {

namespace {

__device__ __forceinline__ void hash_pair3(const uint32_t (&l)[4], const uint32_t (&r)[4], bool padded, uint32_t p,
                                           uint32_t (&d)[4]) {
    ilv::Half s;
    ilv::zero(s);
#pragma unroll
    for (int w = 0; w < 4; ++w) s.v[w] = l[w];
    if (!padded) {
#pragma unroll
        for (int w = 0; w < 4; ++w) s.v[4 + w] = r[w];
    }
    const int nperm = padded ? 2 : 1;
#pragma unroll 1
    for (int k = 0; k < nperm; ++k) {
        if (k == nperm - 1) {  // bit 0 of a lane is even (p = 0), bit 63 odd (p = 1)
            if (p == 1)
                s.v[16] ^= 0x80000000u;
            else if (padded)  // (two static indices: a runtime one sent the state to scratch)
                s.v[3] ^= 1u;
            else
                s.v[8] ^= 1u;
        }
        ilv::keccak_f(s, p);
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) d[w] = s.v[w];
}

// full 256-B window (two blocks) on this lane's parity words; each 64-bit
// message lane is split into its even / odd bits on the way in
__device__ __forceinline__ void hash_window3(const uint4* __restrict__ w, uint32_t p, uint32_t (&d)[4]) {
    uint4 v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = ld_stream(w + k);
    uint32_t m[32];  // message lanes 0..31 as parity-p words
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        m[2 * k] = ilv::to_ilv(v[k].x, v[k].y, p);
        m[2 * k + 1] = ilv::to_ilv(v[k].z, v[k].w, p);
    }
    ilv::Half s;
    ilv::zero(s);
#pragma unroll 1
    for (int b = 0; b < 2; ++b) {
        if (b == 0) {
#pragma unroll
            for (int i = 0; i < 17; ++i) s.v[i] ^= m[i];
        } else {
#pragma unroll
            for (int i = 0; i < 15; ++i) s.v[i] ^= m[17 + i];
            if (p == 0)
                s.v[15] ^= 1u;  // byte 256 = byte 120 of block 1: bit 0 of lane 15
            else
                s.v[16] ^= 0x80000000u;
        }
        ilv::keccak_f(s, p);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = s.v[k];
}

// node j of a plain or ilv node array -> this lane's parity words
__device__ __forceinline__ void load_node3(const uint32_t* __restrict__ in, uint64_t j, bool is_ilv, uint32_t p,
                                           uint32_t (&w4)[4]) {
    if (is_ilv) {
#pragma unroll
        for (int w = 0; w < 4; ++w) w4[w] = in[8 * j + 2 * w + p];
    } else {
        const uint4 a = reinterpret_cast<const uint4*>(in)[2 * j];
        const uint4 b = reinterpret_cast<const uint4*>(in)[2 * j + 1];
        w4[0] = ilv::to_ilv(a.x, a.y, p);
        w4[1] = ilv::to_ilv(a.z, a.w, p);
        w4[2] = ilv::to_ilv(b.x, b.y, p);
        w4[3] = ilv::to_ilv(b.z, b.w, p);
    }
}

// this lane's dwords (2w + p) of a node, plain or ilv
__device__ __forceinline__ void store_node3(uint32_t* __restrict__ out, uint64_t j, bool is_ilv, uint32_t p,
                                            const uint32_t (&w4)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) out[8 * j + 2 * w + p] = is_ilv ? w4[w] : ilv::from_ilv(w4[w], p);
}

}  // namespace

}  // namespace mk
#endif
