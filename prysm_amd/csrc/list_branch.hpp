// The index arithmetic of a list tree's Merkle proof: for a
// list of n items of s bytes (1 <= s <= 128) whose levels lie in the layout of
// mk_ssz_list_tree_levels_bytes(capacity, s), which list bytes the 256-byte
// window of item i holds, which stored node is the sibling at level d and
// whether it exists, and the record stride.  Shared by k_list_tree_branches
// and k_verify_list_branches (kernels_tree.hip), the host side
// (tree_branch_api.cpp) and the host fuzz (tests/c_abi/list_branch_fuzz.cpp);
// no HIP in it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_BRANCH_HD __host__ __device__
#else
#define MK_BRANCH_HD
#endif

namespace mk {

constexpr uint32_t kBranchItemMax = 128;  // a longer item has a window of 2 x item_len: no proof record
constexpr uint32_t kBranchWindow = 256;

struct BranchShape {
    uint32_t s, p, cb;    // item bytes, items per chunk, chunk bytes (p * s)
    uint32_t D;           // levels: the smallest d with ceil(nchunks / 2^d) == 1
    uint64_t n, total;    // items, list bytes (n * s)
    uint64_t nchunks;     // ceil(n / p)
    uint64_t cap_chunks;  // chunks of the capacity: fixes where a level starts
};

// s in 1..128, n <= capacity, capacity * s < 2^64 (the caller's checks)
MK_BRANCH_HD inline BranchShape branch_shape(uint64_t n, uint64_t capacity, uint32_t s) {
    BranchShape b{};
    b.s = s;
    b.p = kBranchItemMax / s;
    b.cb = b.p * s;
    b.n = n;
    b.total = n * s;
    b.nchunks = n / b.p + (n % b.p != 0);
    b.cap_chunks = capacity / b.p + (capacity % b.p != 0);
    for (uint64_t c = b.nchunks; c > 1; c = (c + 1) / 2) ++b.D;
    return b;
}

// bytes of one record: the window, then sib[1] .. sib[D - 1]
MK_BRANCH_HD inline uint64_t branch_record_bytes(const BranchShape& b) {
    return kBranchWindow + 32ull * (b.D > 1 ? b.D - 1 : 0);
}

// nodes of level d >= 1 of the current list: ceil(nchunks / 2^d)
MK_BRANCH_HD inline uint64_t branch_level_count(const BranchShape& b, uint32_t d) {
    if (d >= 64) return b.nchunks != 0;
    const uint64_t m = (1ull << d) - 1;
    return (b.nchunks >> d) + ((b.nchunks & m) != 0);
}

// first node of level d >= 1 in the level array: sum over 1 <= i < d of ceil(cap_chunks / 2^i)
MK_BRANCH_HD inline uint64_t branch_level_off(const BranchShape& b, uint32_t d) {
    uint64_t off = 0, capd = (b.cap_chunks + 1) / 2;
    for (uint32_t i = 1; i < d; ++i) {
        off += capd;
        capd = (capd + 1) / 2;
    }
    return off;
}

// the level-1 node (window) of item i < n; 0 for a list of at most one chunk
MK_BRANCH_HD inline uint64_t branch_window_index(const BranchShape& b, uint64_t i) {
    return b.nchunks >= 2 ? (i / b.p) / 2 : 0;
}

// the list bytes [*lo, *lo + *len) the window of level-1 node j holds: *len <= 256, *lo + *len <= total
MK_BRANCH_HD inline void branch_window(const BranchShape& b, uint64_t j, uint64_t* lo, uint32_t* len) {
    if (b.nchunks < 2) {
        *lo = 0;
        *len = (uint32_t)b.total;  // at most one chunk
        return;
    }
    const uint64_t a = 2 * j * b.cb, rest = b.total - a;  // j < ceil(nchunks / 2): a < total
    *lo = a;
    *len = rest < 2ull * b.cb ? (uint32_t)rest : 2 * b.cb;
}

// K(window) takes a 0^128 after the window's bytes: its second chunk does not exist
MK_BRANCH_HD inline bool branch_window_padded(const BranchShape& b, uint64_t j) {
    return b.nchunks >= 2 && 2 * j + 1 == b.nchunks;
}

// where item i lies in its window
MK_BRANCH_HD inline uint32_t branch_item_pos(const BranchShape& b, uint64_t i) {
    return (uint32_t)(i * b.s - 2 * branch_window_index(b, i) * b.cb);
}

// The sibling at level d (1 <= d < D) of window j's ancestor q = j >> (d - 1):
// true and *node = q ^ 1 when that node is below the level's count (a stored
// node of the current list), false when it does not exist (the slot is 0^32;
// q is then even and the fold pads with 0^128).
MK_BRANCH_HD inline bool branch_sibling(const BranchShape& b, uint64_t j, uint32_t d, uint64_t* node) {
    const uint64_t sib = (j >> (d - 1)) ^ 1ull;
    *node = sib;
    return sib < branch_level_count(b, d);
}

}  // namespace mk
