// The slot map of a resident tree's undo journal: what an
// update of a tree (mk_tree_update: n_old -> n_new values, k_idx listed
// indices) may overwrite of the state the old counts specify, saved at fixed
// positions, one slot per (work item, piece).
// Work item w < W: listed index w for w < k_idx (an index >= n_old stands for
// the last old value, as in the climb), then ONE more when n_new > n_old > 0,
// the last old value: every ancestor of an appended chunk that exists in the
// old tree lies on the old right edge.  W = 0 for n_old == 0: an empty tree
// specifies its root only.
// A tree's region of the journal, every part at a multiple of 16 bytes:
//   [0, 8 W)            the work items' value indices (clamped), 8 B each
//   [idx, +32)          the tree's root
//   [recs + w R, +R)    the record of work item w, R = up16(item_len) + 32 L0 + 32 D:
//        [0, item_len)            the old value
//        [up16(item_len), +32)    its level-0 entry (L0 = 1: a struct / bytes tree)
//        [.. + 32 (d - 1), +32)   node (chunk >> d) of level d = 1 .. D, D the old tree's
//                                 stored levels; it exists under the old counts for
//                                 every work item (chunk < nchunks), so no slot is idle
// Two work items under one node both save it: nothing is compacted, so no slot
// depends on another work item.  The regions of a call's trees follow each
// other; behind them the container message (up16(container_len) bytes) and the
// container root (32 bytes).
// A thread of k_trees_journal / k_trees_restore moves one piece: `unit` bytes of
// a value (16 or 8 when the length and the value buffer's address allow, else
// 1), 16 bytes of a level-0 entry or of a node, 8 bytes of the index list, 4
// bytes of the root (roots are 4-B aligned by contract).
// Shared by the two kernels (kernels_tree.hip), the host side
// (tree_journal_api.cpp) and the host fuzz (tests/c_abi/tree_journal_fuzz.cpp);
// no HIP in it.
#pragma once
#include <stdint.h>

#include "tree_copy.hpp"

namespace mk {

enum JournalPieceKind : uint32_t {
    kJournalNone = 0,    // beyond the tree's pieces
    kJournalItem = 1,    // `unit` bytes of a value
    kJournalLevel0 = 2,  // 16 bytes of a level-0 entry
    kJournalNode = 3,    // 16 bytes of a stored node
    kJournalIndex = 4,   // a work item's value index (journal side only)
    kJournalRoot = 5     // 4 bytes of the root
};

struct JournalShape {
    uint32_t item_len;  // 1 .. 2^30
    uint32_t level0;    // a 32-B entry per value under the levels (struct roots, element digests)
    uint32_t D;         // stored levels of the OLD tree: the smallest d with ceil(nchunks / 2^d) == 1
    uint32_t p;         // leaves per chunk
    uint64_t n_old;
    uint64_t k_idx;     // listed work items; W - k_idx is 0 or 1
    uint64_t W;         // work items
    uint64_t nchunks;   // of the old tree
    uint64_t cap_chunks;
};

// one piece: where it lies in the tree's region of the journal, and in which buffer of the tree
struct JournalPiece {
    uint32_t kind;
    uint32_t len;      // bytes: unit, 16, 8 or 4
    uint32_t level;    // kJournalNode: d
    uint32_t at;       // bytes into the value, the level-0 entry, the node or the root
    uint64_t w;        // the work item (not for the root)
    uint64_t jr_off;   // bytes into the tree's region
};

MK_COPY_HD inline uint64_t journal_up16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// n_old <= n_new <= capacity, item_len in 1 .. 2^30, k_idx < 2^31 (the update's own checks)
MK_COPY_HD inline JournalShape journal_shape(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint64_t k_idx,
                                             uint32_t item_len, bool level0) {
    JournalShape s{};
    s.item_len = item_len;
    s.level0 = level0 ? 1u : 0u;
    s.n_old = n_old;
    const uint32_t leaf = level0 ? 32u : item_len;
    s.p = leaf < 128u ? 128u / leaf : 1u;
    s.nchunks = n_old / s.p + (n_old % s.p != 0);
    s.cap_chunks = capacity / s.p + (capacity % s.p != 0);
    s.D = s.nchunks > 1 ? 64u - (uint32_t)__builtin_clzll(s.nchunks - 1) : 0u;
    s.k_idx = n_old ? k_idx : 0;
    s.W = n_old ? k_idx + (n_new > n_old ? 1u : 0u) : 0;
    return s;
}

// the value a work item stands for: listed index w (idx_w; at or beyond n_old: the last old value), or the last
// old value itself.  W > 0 implies n_old > 0.
MK_COPY_HD inline uint64_t journal_value(const JournalShape& s, uint64_t w, uint64_t idx_w) {
    const uint64_t last = s.n_old - 1;
    return w < s.k_idx && idx_w < last ? idx_w : last;
}

// node (chunk >> d) of value x at level d >= 1, and whether the old counts specify it
MK_COPY_HD inline uint64_t journal_node(const JournalShape& s, uint64_t x, uint32_t d) {
    return d < 64 ? (x / s.p) >> d : 0;
}
MK_COPY_HD inline bool journal_node_exists(const JournalShape& s, uint64_t x, uint32_t d) {
    if (d < 1 || d > s.D || x >= s.n_old) return false;
    const uint64_t m = (1ull << d) - 1;  // D <= 63 whenever a level exists
    return journal_node(s, x, d) < (s.nchunks >> d) + ((s.nchunks & m) != 0);
}
// where that node lies in the level array, in bytes
MK_COPY_HD inline uint64_t journal_node_off(const JournalShape& s, uint64_t x, uint32_t d) {
    return 32 * (copy_level_off(s.cap_chunks, d) + journal_node(s, x, d));
}

MK_COPY_HD inline uint64_t journal_item_slot(const JournalShape& s) { return journal_up16(s.item_len); }
MK_COPY_HD inline uint64_t journal_rec_bytes(const JournalShape& s) {
    return journal_item_slot(s) + 32ull * s.level0 + 32ull * s.D;
}
MK_COPY_HD inline uint64_t journal_root_off(const JournalShape& s) { return journal_up16(8 * s.W); }
MK_COPY_HD inline uint64_t journal_recs_off(const JournalShape& s) { return journal_root_off(s) + 32; }
MK_COPY_HD inline uint64_t journal_tree_bytes(const JournalShape& s) {
    return journal_recs_off(s) + s.W * journal_rec_bytes(s);
}
MK_COPY_HD inline uint64_t journal_container_bytes(uint32_t container_len) {
    return container_len ? journal_up16(container_len) + 32 : 0;
}

// pieces of one work item's record, and of the whole tree (the records, the index list, the root)
MK_COPY_HD inline uint64_t journal_rec_pieces(const JournalShape& s, uint32_t unit) {
    return s.item_len / unit + 2ull * s.level0 + 2ull * s.D;
}
MK_COPY_HD inline uint64_t journal_pieces(const JournalShape& s, uint32_t unit) {
    return s.W * journal_rec_pieces(s, unit) + s.W + 8;
}

// piece g of the tree; unit divides item_len
MK_COPY_HD inline JournalPiece journal_piece(const JournalShape& s, uint32_t unit, uint64_t g) {
    JournalPiece pc{};
    const uint64_t P = journal_rec_pieces(s, unit), in_recs = s.W * P;
    if (g < in_recs) {
        const uint64_t w = g / P;
        uint32_t q = (uint32_t)(g - w * P);
        const uint32_t ipieces = s.item_len / unit;
        const uint64_t rec = journal_recs_off(s) + w * journal_rec_bytes(s);
        pc.w = w;
        if (q < ipieces) {
            pc.kind = kJournalItem, pc.len = unit, pc.at = q * unit;
            pc.jr_off = rec + pc.at;
            return pc;
        }
        q -= ipieces;
        if (s.level0 && q < 2) {
            pc.kind = kJournalLevel0, pc.len = 16, pc.at = 16 * q;
            pc.jr_off = rec + journal_item_slot(s) + pc.at;
            return pc;
        }
        q -= 2 * s.level0;
        pc.kind = kJournalNode, pc.len = 16, pc.level = 1 + (q >> 1), pc.at = 16 * (q & 1u);
        pc.jr_off = rec + journal_item_slot(s) + 32ull * s.level0 + 32ull * (pc.level - 1) + pc.at;
        return pc;
    }
    g -= in_recs;
    if (g < s.W) {
        pc.kind = kJournalIndex, pc.len = 8, pc.w = g;
        pc.jr_off = 8 * g;
        return pc;
    }
    g -= s.W;
    if (g < 8) {
        pc.kind = kJournalRoot, pc.len = 4, pc.at = 4 * (uint32_t)g;
        pc.jr_off = journal_root_off(s) + pc.at;
    }
    return pc;
}

}  // namespace mk
