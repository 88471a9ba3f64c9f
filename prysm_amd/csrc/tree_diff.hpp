// The diff of two resident trees by Merkle descent: which
// stored nodes of tree a and tree b are compared, which are descended without
// a compare and which leaves are compared in the end.  Both trees lie over
// leaves of len0 bytes (the item of a list tree, the 32-B struct root / element
// digest of the other two kinds, 1 <= len0 <= 128), p leaves per chunk, tree X
// holding n_X values in the layout of cap_X; m = min(n_a, n_b).  Node (d, j),
// d >= 1, covers chunks [j 2^d, (j + 1) 2^d); in chunk units, with mch =
// ceil(m / p) and mfull = floor(m / p):
//   visited     (j 2^d) < mch          -- it covers a value below m, so it exists in both trees;
//   comparable  n_a == n_b or (j + 1) 2^d <= mfull  -- it covers the same values in both trees.
// A comparable node whose 32 bytes are equal ends the descent.  A node that
// is not comparable (the one straddler per level when the counts differ) is
// never read and always descended: K(c || 0^128) is both "c was the last chunk"
// and "c is followed by an all-zero chunk", so a straddler can be equal in two
// trees whose values below m differ elsewhere under it -- and equal or not, it
// says nothing about them.  Under a level-1 node j come the values [2 j p,
// min(2 (j + 1) p, m)), compared leaf by leaf.  A work item is one subtree of
// height h0 = min(h, D_a, D_b): the nodes (h0, j) with j < ceil(mch / 2^h0);
// with h0 == 0 the one item compares the at most p values below m directly.
// Every count comes from n_a and n_b; a capacity only places its tree's levels
// (tree_copy.hpp's closed form, per side).  No node at or beyond a level's count,
// no level above min(D_a, D_b) and no leaf byte at or beyond m len0 is read.
// Shared by k_trees_diff (kernels_tree.hip), the host side (tree_diff_api.cpp)
// and the host fuzz (tests/c_abi/tree_diff_fuzz.cpp); no HIP in it.
#pragma once
#include <stdint.h>

#include "tree_copy.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_DIFF_HD __host__ __device__
#else
#define MK_DIFF_HD
#endif

namespace mk {

// Subtree height of one work item: 2^10 chunks.  Its widest frontier is the 2^9 level-1 nodes (2 KB of
// 32-bit local indices, two turns of a 256-thread workgroup), and a registry of 2^20 validators is 256 items.
constexpr uint32_t kDiffHeight = 10;
constexpr uint32_t kDiffFrontMax = 1u << (kDiffHeight - 1);
constexpr uint32_t kDiffItemMax = 128;  // len0: one leaf is at most a chunk

struct DiffShape {
    uint32_t len0, p;     // leaf bytes, leaves per chunk
    uint32_t Da, Db, h0;  // stored levels of the two trees, the height of a work item
    uint32_t same_n;      // n_a == n_b: every visited node is comparable
    uint64_t m;           // min(n_a, n_b)
    uint64_t mch, mfull;  // ceil(m / p), floor(m / p)
    uint64_t cap_chunks_a, cap_chunks_b;
};

// len0 in 1 .. 128, n_X <= cap_X, cap_X * len0 < 2^64 (the caller's checks); h in 1 .. kDiffHeight
MK_DIFF_HD inline DiffShape diff_shape(uint64_t n_a, uint64_t cap_a, uint64_t n_b, uint64_t cap_b, uint32_t len0,
                                       uint32_t h = kDiffHeight) {
    DiffShape s{};
    s.len0 = len0;
    s.p = kDiffItemMax / len0;
    const uint64_t p = s.p;
    const uint64_t ca = n_a / p + (n_a % p != 0), cb = n_b / p + (n_b % p != 0);
    s.Da = ca > 1 ? 64u - (uint32_t)__builtin_clzll(ca - 1) : 0u;
    s.Db = cb > 1 ? 64u - (uint32_t)__builtin_clzll(cb - 1) : 0u;
    const uint32_t Dm = s.Da < s.Db ? s.Da : s.Db;
    s.h0 = h < Dm ? h : Dm;
    s.same_n = n_a == n_b;
    s.m = n_a < n_b ? n_a : n_b;
    s.mfull = s.m / p;
    s.mch = s.mfull + (s.m % p != 0);
    s.cap_chunks_a = cap_a / p + (cap_a % p != 0);
    s.cap_chunks_b = cap_b / p + (cap_b % p != 0);
    return s;
}

// work items of the pair: the visited nodes of level h0 (one item for h0 == 0 and m > 0)
MK_DIFF_HD inline uint64_t diff_items(const DiffShape& s) {
    return (s.mch >> s.h0) + ((s.mch & ((1ull << s.h0) - 1)) != 0);
}

// d <= 58 for any chunk count the checks let through: the shifts do not overflow
MK_DIFF_HD inline bool diff_visited(const DiffShape& s, uint32_t d, uint64_t j) { return (j << d) < s.mch; }

MK_DIFF_HD inline bool diff_comparable(const DiffShape& s, uint32_t d, uint64_t j) {
    return s.same_n || ((j + 1) << d) <= s.mfull;
}

// node j of level d >= 1 in the two level arrays (nodes, not bytes)
MK_DIFF_HD inline uint64_t diff_node_a(const DiffShape& s, uint32_t d, uint64_t j) {
    return copy_level_off(s.cap_chunks_a, d) + j;
}
MK_DIFF_HD inline uint64_t diff_node_b(const DiffShape& s, uint32_t d, uint64_t j) {
    return copy_level_off(s.cap_chunks_b, d) + j;
}

// the values under level-1 node j1 (h0 == 0: j1 == 0, the values of chunk 0): [*lo, *lo + *cnt), *cnt <= 2 p
MK_DIFF_HD inline void diff_leaves(const DiffShape& s, uint64_t j1, uint64_t* lo, uint32_t* cnt) {
    const uint64_t a = j1 * 2 * s.p, rest = s.m - a;  // j1 is visited: a < m
    *lo = a;
    *cnt = rest < 2ull * s.p ? (uint32_t)rest : 2 * s.p;
}

// The descent of work item q < diff_items(s), one node after the other (the
// kernel takes a level's frontier in parallel; the nodes and leaves it touches
// are these).  node_ne(d, j): the 32 bytes of node (d, j) differ between the
// trees -- called for comparable nodes only; leaf_ne(i): leaf i differs;
// emit(i): value i < m is part of the result.  The frontier holds at most
// 2^(h0 - 1) <= kDiffFrontMax nodes.
template <class NodeNe, class LeafNe, class Emit>
inline void diff_walk(const DiffShape& s, uint64_t q, NodeNe node_ne, LeafNe leaf_ne, Emit emit) {
    uint64_t front[2][kDiffFrontMax];
    uint32_t cnt = 1, cur = 0;
    front[0][0] = q;
    for (uint32_t d = s.h0; d >= 1; --d) {
        uint32_t next = 0;
        for (uint32_t f = 0; f < cnt; ++f) {
            const uint64_t j = front[cur][f];
            if (diff_comparable(s, d, j) && !node_ne(d, j)) continue;
            if (d == 1) {
                front[cur ^ 1][next++] = j;
            } else {
                front[cur ^ 1][next++] = 2 * j;
                if (diff_visited(s, d - 1, 2 * j + 1)) front[cur ^ 1][next++] = 2 * j + 1;
            }
        }
        cnt = next;
        cur ^= 1;
    }
    for (uint32_t f = 0; f < cnt; ++f) {
        uint64_t lo;
        uint32_t k;
        diff_leaves(s, s.h0 ? front[cur][f] : 0, &lo, &k);
        for (uint32_t v = 0; v < k; ++v)
            if (leaf_ne(lo + v)) emit(lo + v);
    }
}

}  // namespace mk
