// The audit of a resident tree: which stored node is checked
// against which bytes.  A tree of n values over leaves of len0 bytes (the item
// of a list tree, the 32-B struct root / element digest of the other two kinds,
// 1 <= len0 <= 128) laid out for `capacity` values has one work item per stored
// node of level 1 .. D and one for the root:
//   level 1, node j < ceil(nchunks / 2):  K(window j) -- list_branch.hpp's window, 0^128 behind it when
//                                         chunk 2 j + 1 does not exist;
//   level d = 2 .. D, node j:             K(child 2j || child 2j+1), K(child 2j || 0^128) when 2j+1 is at
//                                         or beyond level d - 1's count;
//   the root:                             K(top || le64(n) || 0^24), top node 0 of level D, or the raw
//                                         chunk (0^128 for n == 0) when nchunks <= 1.
// The items are numbered level after level (a level's first item is the sum
// of the counts below it: tree_copy.hpp's closed form over nchunks), the root
// last, and a call numbers its trees one after the other.  Every count comes
// from n alone; the capacity only places the levels.  No node at or beyond a
// level's count and no level-0 byte at or beyond n * len0 belongs to any item.
// Shared by k_trees_audit (kernels_tree.hip), the host side
// (tree_audit_api.cpp) and the host fuzz (tests/c_abi/tree_audit_fuzz.cpp); no
// HIP in it.
#pragma once
#include <stdint.h>

#include "list_branch.hpp"
#include "tree_copy.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_AUDIT_HD __host__ __device__
#else
#define MK_AUDIT_HD
#endif

namespace mk {

// the level of a mismatch's key: 0 level 0, 1 .. D the levels (D <= 63 for any 64-bit chunk count)
constexpr uint32_t kAuditRoot = 64;         // the list root
constexpr uint32_t kAuditContainer = 65;    // the container checks (the extra report)
constexpr uint32_t kAuditNone = 0xffffffffu;
// a key as the kernels keep it in one 64-bit word, ordered as (level, index): the audit has < 2^31 work items
constexpr uint32_t kAuditKeyShift = 56;
constexpr uint64_t kAuditKeyNone = ~0ull;
MK_AUDIT_HD inline uint64_t audit_key(uint32_t level, uint64_t index) {
    return ((uint64_t)level << kAuditKeyShift) | index;
}

// the buffer a work item's message / stored node lies in
enum AuditBuf : uint32_t { kAuditLevel0 = 0, kAuditLevels = 1, kAuditRootBuf = 2 };

using AuditShape = BranchShape;  // s = len0; p, cb, D, n, total, nchunks, cap_chunks as in §5l

// len0 in 1 .. 128, n <= capacity, capacity * len0 < 2^64 (the caller's checks)
MK_AUDIT_HD inline AuditShape audit_shape(uint64_t n, uint64_t capacity, uint32_t len0) {
    return branch_shape(n, capacity, len0);
}

// slot s = 0 .. D of a tree: level s + 1 for s < D, the root for s == D
MK_AUDIT_HD inline uint32_t audit_slots(const AuditShape& b) { return b.D + 1; }

// the tree's first work item of slot s <= D + 1 (s == D + 1: its item total)
MK_AUDIT_HD inline uint64_t audit_slot_first(const AuditShape& b, uint32_t s) {
    return s <= b.D ? copy_level_off(b.nchunks, s + 1) : copy_level_off(b.nchunks, b.D + 1) + 1;
}

MK_AUDIT_HD inline uint64_t audit_items(const AuditShape& b) { return audit_slot_first(b, b.D + 1); }

// where slot s's messages start (bytes): the level below it, or level 0
MK_AUDIT_HD inline void audit_slot_child(const AuditShape& b, uint32_t s, uint32_t* buf, uint64_t* off) {
    if (s == 0 || b.D == 0) {  // the windows, or the raw chunk under the root
        *buf = kAuditLevel0;
        *off = 0;
    } else {  // level s (for the root: level D)
        *buf = kAuditLevels;
        *off = 32 * copy_level_off(b.cap_chunks, s);
    }
}

// where slot s's stored nodes start (bytes)
MK_AUDIT_HD inline void audit_slot_node(const AuditShape& b, uint32_t s, uint32_t* buf, uint64_t* off) {
    if (s == b.D) {
        *buf = kAuditRootBuf;
        *off = 0;
    } else {
        *buf = kAuditLevels;
        *off = 32 * copy_level_off(b.cap_chunks, s + 1);
    }
}

// the slot of work item q < audit_items(b): the last s with audit_slot_first(b, s) <= q, by bisection
MK_AUDIT_HD inline uint32_t audit_slot_of(const AuditShape& b, uint64_t q) {
    uint32_t lo = 0, hi = b.D;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (audit_slot_first(b, mid) <= q)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// One work item: the key of its node, the message K is taken of -- msg_len
// bytes at child_off of child_buf, then `zeros` zero bytes, then for the root
// le64(n) || 0^24 -- and the stored node it is compared with.
struct AuditItem {
    uint32_t level;  // 1 .. D, kAuditRoot
    uint32_t child_buf, node_buf;
    uint32_t msg_len;  // <= 256
    uint32_t zeros;    // 0 or 128
    uint32_t mixin;    // the root: the length follows
    uint64_t index;
    uint64_t child_off, node_off;  // bytes from the start of the slot (audit_slot_child / _node)
};

// item j of slot s
MK_AUDIT_HD inline AuditItem audit_item_in(const AuditShape& b, uint32_t s, uint64_t j) {
    AuditItem it{};
    it.index = j;
    uint64_t base;  // the slots' starts are the caller's (looked up once per slot)
    audit_slot_node(b, s, &it.node_buf, &base);
    audit_slot_child(b, s, &it.child_buf, &base);
    it.node_off = 32 * j;
    if (s == b.D) {  // the root
        it.level = kAuditRoot;
        it.mixin = 1;
        it.child_off = 0;
        if (b.D == 0) {  // over the raw chunk
            it.msg_len = (uint32_t)b.total;
            it.zeros = b.n == 0 ? 128u : 0u;
        } else {
            it.msg_len = 32;
        }
    } else if (s == 0) {  // a window
        it.level = 1;
        uint64_t lo;
        branch_window(b, j, &lo, &it.msg_len);
        it.child_off = lo;
        it.zeros = branch_window_padded(b, j) ? 128u : 0u;
    } else {  // children 2j and 2j + 1 of level s
        it.level = s + 1;
        it.child_off = 64 * j;
        const bool pad = 2 * j + 1 >= branch_level_count(b, s);
        it.msg_len = pad ? 32u : 64u;
        it.zeros = pad ? 128u : 0u;
    }
    return it;
}

// work item q < audit_items(b) of the tree; *slot: its slot
MK_AUDIT_HD inline AuditItem audit_item(const AuditShape& b, uint64_t q, uint32_t* slot) {
    const uint32_t s = audit_slot_of(b, q);
    *slot = s;
    return audit_item_in(b, s, q - audit_slot_first(b, s));
}

}  // namespace mk
