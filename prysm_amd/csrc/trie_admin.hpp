// Roll back, fork point, audit and copy of the resident deposit trie (DESIGN.md
// §5p): which stored nodes each of them reads and writes.  The level array is
// the one of mk_deposit_trie_levels_bytes: level d of a trie laid out for `cap`
// leaves starts at node sum_{i<d} ceil(cap / 2^i) and has cnt(c, d) =
// ceil(c / 2^d) LIVE nodes when the trie holds c deposits; a node at or beyond
// its level's live count is DEAD: no rule below reads one, and only the copy's
// destination may hold one that differs from what an append left there.
//
//   roll back to c <= count   every level d in 1 .. depth that 2^d does not divide c into (and count > c) has
//                             one node p_d = (c - 1) >> d that straddles c; it gets E_d, the as-of chain of
//                             §5i: E_d = K(level_{d-1}[q - 1] || E_{d-1}) for odd q = (c - 1) >> (d - 1),
//                             K(E_{d-1} || 0^32) for even q, from the stored node of level ctz(c).  The root
//                             is E_depth, the stored level-`depth` node 0 when no level straddles, 0^32 for
//                             c == 0 (level `depth` node 0 is then zeroed too).  Nothing else is written.
//   fork point of A and B     m = min(count_a, count_b); node (d, j) is comparable when (j + 1) 2^d <= m.
//                             [0, m) is the left-to-right row of the complete subtrees (d, (m >> d) - 1) of
//                             the set bits d of m; the first whose stored roots differ is walked down (left
//                             child differs: left, else right) to the leaf.  None differs: m.
//   audit                     level d = 1 .. depth, node j < cnt(count, d): K(level_{d-1}[2j] || R), R the
//                             node 2j + 1 when it is live, else 0^32; the root against level `depth` node 0
//                             (0^32 for count == 0).  Level 0 is never checked.
//   copy                      the live nodes of level 0 .. depth from the layout of one capacity to another.
//
// Shared by the kernels (kernels_trie_admin.hip), the host side
// (trie_admin_api.cpp) and the host fuzz (tests/c_abi/trie_admin_fuzz.cpp); no
// HIP in it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_TRIE_HD __host__ __device__
#else
#define MK_TRIE_HD
#endif

namespace mk {

constexpr uint32_t kTrieDepthMax = 63;  // so that 2^depth and every (level, index) key fit

// live nodes of level d <= 63 of a trie of c deposits
MK_TRIE_HD inline uint64_t ta_count(uint64_t c, uint32_t d) { return (c >> d) + ((c & ((1ull << d) - 1)) != 0); }

// first node of level d <= depth + 1 in the level array of capacity cap (d == depth + 1: the array's nodes)
MK_TRIE_HD inline uint64_t ta_level_off(uint64_t cap, uint32_t d) {
    uint64_t off = 0;
    for (uint32_t i = 0; i < d; ++i) off += ta_count(cap, i);
    return off;
}

// ---- roll back ---------------------------------------------------------------------------------
// The lowest straddling level d0 = ctz(c) + 1 (the chain starts from the stored node of level d0 - 1), or 0
// when no level straddles: c == 0, c == count, or 2^depth divides c.
MK_TRIE_HD inline uint32_t ta_chain_first(uint64_t count, uint64_t c, uint32_t depth) {
    if (c == 0 || count <= c) return 0;
    const uint32_t d0 = (uint32_t)__builtin_ctzll(c) + 1;
    return d0 <= depth ? d0 : 0;
}

// the node of level d on the path of leaf c - 1 (c >= 1): the straddler of a straddling level
MK_TRIE_HD inline uint64_t ta_path_node(uint64_t c, uint32_t d) { return (c - 1) >> d; }

// the path's node of level d is a right child: its left sibling, node ta_path_node(c, d) - 1, is complete below c
MK_TRIE_HD inline bool ta_path_right(uint64_t c, uint32_t d) { return (((c - 1) >> d) & 1u) != 0; }

// A 32-byte node as the host forms move it.
struct TrieNode {
    uint8_t b[32];
};

// The roll back, one node after the other (the kernel runs the same chain on
// one wave).  load(d, j): the stored node j of level d, called for live nodes
// only; store(d, j, v); hash(l, r) = K(l || r); the new root is returned.
template <class Load, class Store, class Hash>
inline TrieNode ta_truncate(uint64_t count, uint64_t c, uint32_t depth, Load load, Store store, Hash hash) {
    TrieNode zero{};
    if (c == 0) {
        store(depth, 0, zero);
        return zero;
    }
    const uint32_t d0 = ta_chain_first(count, c, depth);
    if (d0 == 0) return load(depth, 0);
    TrieNode e = load(d0 - 1, ta_path_node(c, d0 - 1));
    for (uint32_t d = d0 - 1; d < depth; ++d) {
        e = ta_path_right(c, d) ? hash(load(d, ta_path_node(c, d) - 1), e) : hash(e, zero);
        store(d + 1, ta_path_node(c, d + 1), e);
    }
    return e;
}

// ---- fork point -------------------------------------------------------------------------------
// bit d <= depth of m names the complete subtree (d, ta_fork_sub(m, d)) of the row that covers [0, m)
MK_TRIE_HD inline bool ta_fork_has(uint64_t m, uint32_t d) { return ((m >> d) & 1u) != 0; }
MK_TRIE_HD inline uint64_t ta_fork_sub(uint64_t m, uint32_t d) { return (m >> d) - 1; }

// ne(d, j): the stored nodes (d, j) of the two tries differ -- called for comparable nodes only
template <class Ne>
inline uint64_t ta_fork_point(uint64_t count_a, uint64_t count_b, uint32_t depth, Ne ne) {
    const uint64_t m = count_a < count_b ? count_a : count_b;
    for (uint32_t d = depth + 1; d-- > 0;) {
        if (!ta_fork_has(m, d)) continue;
        uint64_t j = ta_fork_sub(m, d);
        if (!ne(d, j)) continue;
        for (uint32_t e = d; e > 0; --e) j = ne(e - 1, 2 * j) ? 2 * j : 2 * j + 1;
        return j;
    }
    return m;
}

// ---- audit ------------------------------------------------------------------------------------
// Work items: the live nodes of level 1, then level 2, .. level depth, the root last.  Slot s < depth is level
// s + 1, slot depth the root; ta_audit_first(count, depth, depth + 1) is the item total.
MK_TRIE_HD inline uint64_t ta_audit_first(uint64_t count, uint32_t depth, uint32_t s) {
    uint64_t a = 0;
    for (uint32_t i = 1; i <= s && i <= depth; ++i) a += ta_count(count, i);
    return s > depth ? a + 1 : a;
}
MK_TRIE_HD inline uint64_t ta_audit_items(uint64_t count, uint32_t depth) {
    return ta_audit_first(count, depth, depth + 1);
}
// node j of level d >= 1 has a live right child
MK_TRIE_HD inline bool ta_audit_right(uint64_t count, uint32_t d, uint64_t j) {
    return 2 * j + 1 < ta_count(count, d - 1);
}

// bad(level, j) for every mismatch, level 1 .. depth and root_level for the root; returns their number
template <class Load, class Hash, class Bad>
inline uint64_t ta_audit(uint64_t count, uint32_t depth, const TrieNode& root, uint32_t root_level, Load load,
                         Hash hash, Bad bad) {
    auto differ = [](const TrieNode& x, const TrieNode& y) {
        for (int k = 0; k < 32; ++k)
            if (x.b[k] != y.b[k]) return true;
        return false;
    };
    TrieNode zero{};
    uint64_t n = 0;
    for (uint32_t d = 1; d <= depth; ++d)
        for (uint64_t j = 0; j < ta_count(count, d); ++j) {
            const TrieNode want = hash(load(d - 1, 2 * j), ta_audit_right(count, d, j) ? load(d - 1, 2 * j + 1) : zero);
            if (differ(want, load(d, j))) bad(d, j), ++n;
        }
    if (differ(root, count ? load(depth, 0) : zero)) bad(root_level, 0), ++n;
    return n;
}

// ---- copy -------------------------------------------------------------------------------------
// Pieces of 16 bytes: the two halves of every live node, level after level; ta_copy_first(count, depth + 1):
// the pieces of the levels (the root's two follow when it travels).
MK_TRIE_HD inline uint64_t ta_copy_first(uint64_t count, uint32_t d) {
    uint64_t a = 0;
    for (uint32_t i = 0; i < d; ++i) a += ta_count(count, i);
    return 2 * a;
}

}  // namespace mk
