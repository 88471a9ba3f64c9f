// Round 0 of a Keccak-f[1600] permutation whose input state is mostly zero:
// the mirror image of the digest-only last round (keccak_dev.hpp).  The
// zero lanes drop out of theta's column parities, and after theta a zero
// lane simply IS its column's D = C[x-1] ^ rotl(C[x+1], 1), so D is computed
// once per column and only the live lanes are XORed with it.  rho, pi, chi
// and iota are the full round's.
//
//   round0_node     K(L || R) of two 32-B nodes: lanes 0..7 are data, lane 8
//                   is the pad byte 0x01, lane 16 the closing 0x80 << 56.
//                   7 + 10 + 28 + 48 + 52 = 145 VALU instead of 180.
//   round0_block17  the first block of a longer message: lanes 0..16 live.
//                   14 + 10 + 44 + 48 + 52 = 168 instead of 180.
//
// The instruction sequence is written once, over an `Ops` policy: the device
// policy (keccak_dev.hpp, AsmOps) is one asm volatile per instruction and the
// locked round's two s_barriers at round_asm<true>'s positions; the host
// policy of tests/c_abi/sparse_round_host.cpp is plain C++, so the lane map
// below is what the host test checks against a textbook round.
//   Ops::x2(a, b) a ^ b            Ops::x3(a, b, c) a ^ b ^ c
//   Ops::xk(a, k) a ^ constant k   Ops::x3k(a, b, k) a ^ b ^ constant k
//   Ops::rot<N>(lo, hi, olo, ohi)  64-bit rotate left by N of (lo, hi)
//   Ops::chi(a, b, c) a ^ (~b & c)
//   Ops::bar_theta(), Ops::bar_chi()  the barriers before theta-apply and chi
// S is any struct with uint32_t lo[25], hi[25] (the halves of the 25 lanes).
#pragma once
#include <stdint.h>

#include <utility>

#if defined(__HIPCC__)
#define MK_SPARSE_FN __device__ __forceinline__
#else
#define MK_SPARSE_FN inline
#endif

namespace mk {
namespace sparse {

// rho offsets r[x][y], lane index x + 5y
constexpr int rho(int i) {
    constexpr int r[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return r[i];
}

template <class Ops, class S, int I>
MK_SPARSE_FN void rho_pi_one(const S& a, uint32_t (&blo)[25], uint32_t (&bhi)[25]) {
    constexpr int x = I % 5, y = I / 5;
    constexpr int dst = y + 5 * ((2 * x + 3 * y) % 5);
    Ops::template rot<rho(I)>(a.lo[I], a.hi[I], blo[dst], bhi[dst]);
}
template <class Ops, class S, int... Is>
MK_SPARSE_FN void rho_pi_all(const S& a, uint32_t (&blo)[25], uint32_t (&bhi)[25], std::integer_sequence<int, Is...>) {
    (rho_pi_one<Ops, S, Is>(a, blo, bhi), ...);
}

// rho, pi, chi, iota on the 25 lanes theta has produced
template <class Ops, class S>
MK_SPARSE_FN void tail(S& s, uint32_t rclo, uint32_t rchi) {
    uint32_t blo[25], bhi[25];
    rho_pi_all<Ops>(s, blo, bhi, std::make_integer_sequence<int, 25>{});
    Ops::bar_chi();
#pragma unroll
    for (int y = 0; y < 5; ++y) {
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const int i = x + 5 * y;
            const int i1 = (x + 1) % 5 + 5 * y, i2 = (x + 2) % 5 + 5 * y;
            s.lo[i] = Ops::chi(blo[i], blo[i1], blo[i2]);
            s.hi[i] = Ops::chi(bhi[i], bhi[i1], bhi[i2]);
        }
    }
    s.lo[0] = Ops::xk(s.lo[0], rclo);
    s.hi[0] = Ops::xk(s.hi[0], rchi);
}

// D of every column from the column parities (rotations, barrier, 10 XORs)
template <class Ops>
MK_SPARSE_FN void theta_d(const uint32_t (&clo)[5], const uint32_t (&chi_)[5], uint32_t (&dlo)[5], uint32_t (&dhi)[5]) {
    uint32_t rlo[5], rhi[5];
#pragma unroll
    for (int x = 0; x < 5; ++x) Ops::template rot<1>(clo[x], chi_[x], rlo[x], rhi[x]);
    Ops::bar_theta();
#pragma unroll
    for (int x = 0; x < 5; ++x) {
        dlo[x] = Ops::x2(clo[(x + 4) % 5], rlo[(x + 1) % 5]);
        dhi[x] = Ops::x2(chi_[(x + 4) % 5], rhi[(x + 1) % 5]);
    }
}

// In: s lanes 0..7 (lanes 8..24 are not read).  Out: all 25 lanes, equal to
// the full round on lanes 0..7 | 0x01 in lane 8 | 0x80 << 56 in lane 16 | 0.
template <class Ops, class S>
MK_SPARSE_FN void round0_node(S& s, uint32_t rclo, uint32_t rchi) {
    uint32_t clo[5], chi_[5];
    clo[0] = Ops::x2(s.lo[0], s.lo[5]);
    chi_[0] = Ops::x2(s.hi[0], s.hi[5]);
    clo[1] = Ops::x2(s.lo[1], s.lo[6]);
    chi_[1] = Ops::x3k(s.hi[1], s.hi[6], 0x80000000u);  // lane 16
    clo[2] = Ops::x2(s.lo[2], s.lo[7]);
    chi_[2] = Ops::x2(s.hi[2], s.hi[7]);
    clo[3] = Ops::xk(s.lo[3], 1u);  // lane 8
    chi_[3] = s.hi[3];
    clo[4] = s.lo[4];
    chi_[4] = s.hi[4];
    uint32_t dlo[5], dhi[5];
    theta_d<Ops>(clo, chi_, dlo, dhi);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s.lo[i] = Ops::x2(s.lo[i], dlo[i % 5]);
        s.hi[i] = Ops::x2(s.hi[i], dhi[i % 5]);
    }
#pragma unroll
    for (int i = 8; i < 25; ++i) {
        s.lo[i] = dlo[i % 5];
        s.hi[i] = dhi[i % 5];
    }
    s.lo[8] = Ops::xk(s.lo[8], 1u);
    s.hi[16] = Ops::xk(s.hi[16], 0x80000000u);
    tail<Ops>(s, rclo, rchi);
}

// In: s lanes 0..16 (lanes 17..24 are not read).  Out: all 25 lanes, equal
// to the full round on lanes 0..16 | 0.
template <class Ops, class S>
MK_SPARSE_FN void round0_block17(S& s, uint32_t rclo, uint32_t rchi) {
    uint32_t clo[5], chi_[5];
#pragma unroll
    for (int x = 0; x < 5; ++x) {
        clo[x] = Ops::x3(s.lo[x], s.lo[x + 5], s.lo[x + 10]);
        chi_[x] = Ops::x3(s.hi[x], s.hi[x + 5], s.hi[x + 10]);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {  // lanes 15, 16
        clo[x] = Ops::x2(clo[x], s.lo[x + 15]);
        chi_[x] = Ops::x2(chi_[x], s.hi[x + 15]);
    }
    uint32_t dlo[5], dhi[5];
    theta_d<Ops>(clo, chi_, dlo, dhi);
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        s.lo[i] = Ops::x2(s.lo[i], dlo[i % 5]);
        s.hi[i] = Ops::x2(s.hi[i], dhi[i % 5]);
    }
#pragma unroll
    for (int i = 17; i < 25; ++i) {
        s.lo[i] = dlo[i % 5];
        s.hi[i] = dhi[i % 5];
    }
    tail<Ops>(s, rclo, rchi);
}

}  // namespace sparse
}  // namespace mk
