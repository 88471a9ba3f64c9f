// The index map of a stable erase: k strictly ascending
// removed indices r_0 < .. < r_{k-1} of a list of n_old values; destination
// position q of the n_old - k survivors takes the value of source q + j, j the
// number of i with r_i - i <= q (r_i - i is non-decreasing: the survivors in
// front of r_i).  Positions below r_0 do not move (j == 0).  Shared by
// k_tree_compact (kernels_tree.hip) and the host fuzz
// (tests/c_abi/tree_compact_fuzz.cpp); no HIP in it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_COMPACT_HD __host__ __device__
#else
#define MK_COMPACT_HD
#endif

namespace mk {

// j for destination q, searched in [lo, hi] (0 <= lo <= hi <= k): the caller
// knows that at least lo and at most hi of the r_i - i are <= q.  A bisection
// of at most 64 steps that only reads rm[lo .. hi): bounded, and j <= hi, for
// any contents of rm (a list that is not ascending gives a wrong j, never an
// index outside rm).
MK_COMPACT_HD inline uint64_t compact_skip_in(const uint64_t* rm, uint64_t lo, uint64_t hi, uint64_t q) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (rm[mid] - mid <= q)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

MK_COMPACT_HD inline uint64_t compact_skip(const uint64_t* rm, uint64_t k, uint64_t q) {
    return compact_skip_in(rm, 0, k, q);
}

// the source position of destination q < n_old - k: below n_old for any rm
MK_COMPACT_HD inline uint64_t compact_src(const uint64_t* rm, uint64_t k, uint64_t q) {
    return q + compact_skip(rm, k, q);
}

}  // namespace mk
