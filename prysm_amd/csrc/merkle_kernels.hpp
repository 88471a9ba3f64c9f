// Shared declarations between the HIP kernels and the host planner / C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_types.hpp"
#include "struct_spec.hpp"

namespace mk {

#define MK_STRUCT_THREADS 256
constexpr uint32_t kStructThreads = MK_STRUCT_THREADS;  // k_struct_fused: one record per thread
constexpr uint32_t kStructFusedMaxMsg = 160;          // LDS: kStructThreads * msg_len bytes
constexpr uint32_t kStructFusedMaxField = 64;         // bytes fields held in 16 registers
// StructSpec, NestedSpec: struct_spec.hpp

template <bool LEAF, bool FAST, int NI>
__global__ void k_reduce(ReduceArgs a);
// Phase-locked leaf pass (merkle_kernels.hip): 4096 full windows per
// workgroup -> 1024 nodes three levels above the chunks.
constexpr uint32_t kLockThreads = 1024;
constexpr uint64_t kLockWindows = 4 * kLockThreads;
__global__ void k_leaf_lock_sc(ReduceArgs a, uint64_t ngroups);  // coalesced LDS-DMA staging, persistent grid
#define MK_LOCK_DMA_ROUND 14  // k_leaf_lock_sc: round of a window's second permutation after which the last part of the next block 1 is fetched
#define MK_LOCK_GRID 256
template <bool FAST>
__global__ void k_reduce_elem(ReduceArgs a);
// phase-locked element windows: nwin window digests (level-1 nodes) of 8 x 32-B elements each
__global__ void k_elem_lock(const uint4* elems, uint64_t nwin, uint4* out);
template <bool FAST32>
__global__ void k_elem_digests(const uint8_t* elems, uint64_t n, uint32_t elem_len, uint4* out);
template <bool FAST>
__global__ void k_struct_fields(const uint8_t* rec, uint64_t n, StructSpec sp, uint8_t* msg);
__global__ void k_struct_fused(const uint8_t* rec, uint64_t n, StructSpec sp, uint32_t vec16, uint4* roots);
// nested structs and variable-length byte fields: one record per thread, one launch;
// dynamic LDS NT * ns.peak bytes (NT = ns.threads)
template <uint32_t NT>
__global__ void k_struct_nested(const uint8_t* rec, uint64_t n, NestedSpec ns, uint4* roots);
// the same with list fields (MK_FIELD_LIST): dynamic LDS NT * ls.peak bytes (NT = ls.threads: 128 or 64)
template <uint32_t NT>
__global__ void k_struct_list(const uint8_t* rec, uint64_t n, ListSpec ls, uint4* roots);
template <int NB, int NRAW>
__global__ void k_struct_reg(const uint8_t* rec, uint64_t n, StructSpec sp, uint32_t vec16, uint4* roots);
// validator layout (kValOff/kValLen in kernels_struct.hip), any n (a partial last group);
// gpw > 0: contiguous groups per workgroup plus the level-1 windows of the roots' merkleHash
// (and of a second list of vbytes bytes at vals, when vals != nullptr)
// PREV (a stream of states, gpw == 4): the same launch also builds levels
// 2..10 of the PREVIOUS state's registry tree over its level-1 windows and
// levels 2..4 of its second list's, one extra lock-step permutation per wave
// (see the kernel); workgroup b < nfull takes the complete 512-window
// registry subtree [512 b, 512 b + 512), b < nvfull the 128-window one.
struct StructPrev {
    const uint4* l1;   // the previous state's level-1 windows (complete)
    uint4* lv[9];      // its levels 2..10: level k node j of subtree b at lv[k - 2][(512 >> (k - 1)) b + j]
    const uint4* v1;   // the previous state's second-list level-1 windows (128 per workgroup)
    uint4* vlv[3];     // its levels 2..4: level k node j of subtree b at vlv[k - 2][(128 >> (k - 1)) b + j]
    uint32_t nfull;    // registry subtrees (workgroups) with all 512 windows
    uint32_t nvfull;   // second-list subtrees with all 128 windows
    uint32_t live;     // 0: no previous state (the slots hash zeros, store nothing)
};
template <bool PREV>
__global__ void k_struct_lock(const uint8_t* rec, uint64_t n, uint4* roots, uint32_t gpw, uint4* wins,
                              const uint8_t* vals, uint64_t vbytes, uint4* vwins, StructPrev prev);
template <int NB, int NRAW>
__global__ void k_struct_split(const uint8_t* rec, uint64_t n, StructSpec sp, uint32_t vec16, uint4* roots);
#define MK_STRUCT_SPLIT_MAX_N 32768
constexpr uint64_t kStructSplitMaxN = MK_STRUCT_SPLIT_MAX_N;  // k_struct_split at or below (0: never)
template <uint32_t NT, bool LEAF>
__global__ void k_wave3(ReduceArgs a);
// k_wave3's last levels run one state per wave (the pair finalize needs that form)
__global__ void k_final_small(const uint8_t* items, uint64_t total, uint64_t n, uint8_t* out);
__global__ void k_keccak64(const uint4* in, uint64_t n, uint4* out);
__global__ void k_keccak64_lock(const uint4* in, uint64_t n, uint4* out);  // any n (a partial last group)
// phase-locked node pass: ngroups whole groups of 1024 x kNodeLockPairs complete node pairs, persistent grid
__global__ void k_node_lock(ReduceArgs a, uint64_t ngroups);
__global__ void k_keccak_fixed(const uint8_t* in, uint64_t n, uint32_t msg_len, uint4* out);
__global__ void k_keccak_var(const uint8_t* in, const uint64_t* offs, uint64_t n, uint4* out);
__global__ void k_trie_level(const uint4* in, uint64_t cin, uint4* out);
__global__ void k_keccak_words(const uint2* in, uint64_t n, uint32_t nwords, uint4* out);
template <int NW>
__global__ void k_keccak_rec(const uint2* in, uint64_t n, uint4* out);
// Phase-locked deposit-trie front: leaves + levels 1..log2(DPT) of a trie of
// 280-B deposits, ngroups * NT * DPT deposits (the host runs the rest).
// PIPE: the same launch also builds levels 3..7 of the PREVIOUS trie of a
// stream (one wave-wide permutation per wave, in the lock-step slots, see
// the kernel); one group per workgroup.
struct TriePrev {
    const uint4* l2;  // the previous trie's level 2 (complete)
    uint4* l[5];      // its levels 3..7 (written)
    uint32_t live;    // 0: no previous trie (the slots hash zeros, store nothing)
};
template <uint32_t NT, int DPT, bool PIPE>
__global__ void k_trie_rec_lock(const uint2* in, uint64_t ngroups, uint4* L0, uint4* L1, uint4* L2, uint4* L3,
                                TriePrev prev);
template <uint32_t NT>
__global__ void k_trie_rec_lock_sm(const uint2* in, uint64_t ngroups, uint4* L0, uint4* L1, uint4* L2);
#define MK_TRIE_LOCK_GRID 256  // persistent grid cap
#define MK_TRIE_LOCK_MIN (1u << 18)  // deposits: at least one group per CU

#define MK_REC_THREADS 256
constexpr uint32_t kRecThreads = MK_REC_THREADS;  // k_keccak_rec workgroup size
#define MK_REC_GRID 4096
constexpr uint32_t kRecGridMax = MK_REC_GRID;  // k_keccak_rec grid cap (A/B at 2^20: 512..4096 WGs, 4096 best)
template <uint32_t NT>
__global__ void k_trie_top3(const uint32_t* in, uint64_t cin, uint32_t* lv_out, uint32_t levels, uint64_t capn);
__global__ void k_verify_branches(const uint4* leaves, const uint4* branches, const uint64_t* indices,
                                  uint32_t depth, uint32_t tree_depth, const uint4* roots, uint64_t n,
                                  uint8_t* ok);
template <uint32_t NT>
__global__ void k_trie_append(uint32_t* levels, uint64_t cap, uint32_t d0, uint64_t lo, uint64_t c, uint32_t d_end,
                              uint32_t depth, uint32_t* root_out);
#define MK_SPREAD_WAVES_MAX 16
constexpr uint32_t kSpreadWavesMax = MK_SPREAD_WAVES_MAX;  // k_trie_spread: one state per wave (<= 4 per SIMD)
template <uint32_t SPAN>
__global__ void k_spread_leaf(ReduceArgs a, uint32_t w8);
template <int NB, int NRAW>
__global__ void k_struct_list_fused(const uint8_t* rec, uint64_t n, StructSpec sp, uint32_t vec16, uint4* roots,
                                    ReduceArgs a, uint32_t* sub, uint32_t* out, uint32_t slot);
// new deposits k_trie_spread hashes into level 0 first (k == 0: none)
struct SpreadLeaves {
    const uint8_t* data;
    const uint64_t* offs;  // device, k+1 entries relative to data; NULL: fixed_len records
    uint32_t fixed_len;
    uint32_t k;
    uint32_t aligned8;     // data, offsets / fixed_len multiples of 8
};
template <uint32_t NW>
__global__ void k_trie_spread(uint32_t* levels, uint64_t cap, uint32_t d0, uint64_t lo, uint64_t c, uint32_t d_end,
                              uint32_t depth, uint32_t* root_out, SpreadLeaves lv);
// fused tree tops: arrival counter slots (one per fused launch in flight)
constexpr uint32_t kArriveSlots = 4096;
// k_trie_top_fused, k_merkle_top_fused: the last of each kTopGroup workgroups
// to arrive reduces the group's nodes before the next stage / the last group
// finishes the top (0: the last workgroup alone reduces all the grid's nodes)
#define MK_TOP_GROUP_LOG2 4
constexpr uint32_t kTopGroupLog2 = MK_TOP_GROUP_LOG2, kTopGroup = 1u << kTopGroupLog2;
// upper bound of the arrival slots one launch uses (a 1024-workgroup grid); a
// launch reserves only top_arrive_slots(parts) of them (merkle_api.cpp)
constexpr uint32_t kTopGroupSlots = kTopGroupLog2 ? 1 + 2 * 1024 / kTopGroup : 1;
template <uint32_t NT>
__global__ void k_trie_top_fused(uint32_t* levels, uint64_t cap, uint64_t c0, uint32_t d0, uint32_t depth,
                                 uint32_t* root_out, uint32_t slot);
// k_merkle_top_fused: one list's part of the launch
struct MerkleTopList {
    const uint4* nodes;  // a complete level of the list's tree (plain 32-B nodes)
    uint64_t c;          // its node count
    uint64_t n_items;    // the length mix-in (hash.go:237-238)
    uint32_t* sub;       // workspace: one published node per workgroup (32 B each)
    uint32_t* out;       // the list root (32 B; with a pair: its slot of the pair block)
    uint32_t wg0, nwg;   // this list's workgroups
    uint32_t span_log2;  // level nodes per workgroup
    uint32_t slot;       // first of its arrival counters (g_arrive; merkle_api.cpp top_arrive_slots)
};
struct MerkleTopArgs {
    MerkleTopList l[2];
    uint32_t nlists;
    uint32_t* pair;      // two lists: the pair block (roots at [0, 64), the struct root at [64, 96)), else NULL
    uint32_t pair_slot;  // two lists: the arrival counter of the two finishers
};
template <uint32_t NT>
__global__ void k_merkle_top_fused(MerkleTopArgs a);
__global__ void k_trie_append1(uint32_t* levels, uint64_t cap, uint64_t count, uint32_t depth, uint32_t* root_out,
                               SpreadLeaves lv);
template <uint32_t NW>
__global__ void k_trie_prefix_roots(const uint4* levels, uint64_t cap, uint64_t count0, uint64_t m, uint32_t depth,
                                    uint4* roots);
__global__ void k_trie_branch(const uint4* levels, uint64_t cap, uint64_t count, uint32_t depth, uint64_t index,
                              uint4* branch);
// branches of k indices (and the root) as of a past deposit count; one branch per wave, kBranchWaves per workgroup
constexpr uint32_t kBranchWaves = 4;
__global__ void k_trie_branches_at(const uint4* levels, uint64_t cap, uint64_t count, uint64_t as_of, uint32_t depth,
                                   const uint64_t* indices, uint64_t k, uint4* branches, uint4* root_at);
// verifyDeposit for a batch: leaf hash of the deposit data, the fold, the compare (root_stride 0: one shared root)
__global__ void k_verify_deposits(const uint8_t* data, const uint64_t* offs, const uint4* branches,
                                  const uint64_t* indices, uint32_t depth, uint32_t tree_depth, const uint4* roots,
                                  uint32_t root_stride, uint64_t n, uint8_t* ok);
template <bool LEAF>
__global__ void k_many_level(const uint8_t* items, const ManyList* lists, const ManyAct* act, uint32_t nact,
                             uint64_t nodes, const uint4* in, uint4* out, uint4* tops);
__global__ void k_many_final(const uint8_t* items, const ManyList* lists, uint32_t nlists, const uint4* tops,
                             uint4* roots);
__global__ void k_synth(uint64_t* dst, uint64_t nwords, uint64_t seed, uint64_t word0);
// device-resident list tree (kernels_tree.hip, list_tree_api.cpp)
struct ListTreeArgs {
    const uint8_t* items;  // level 0: n_new items of item_len bytes
    uint32_t* levels;      // level d >= 1 at node sum_{1<=i<d} ceil(cap_chunks / 2^i)
    const uint64_t* idx;   // k_idx ascending dirty item indices < n_old (device)
    uint64_t k_idx;
    uint64_t n_old, n_new;  // items n_old .. n_new - 1 are appended (dirty)
    uint64_t cap_chunks;
    uint32_t item_len;
    uint32_t per;          // items per chunk
    uint64_t* arrive;      // one zeroed word per work item (k_idx + n_new - n_old)
    uint32_t* root_out;
};
// one lane pair per dirty item; the ancestors of the dirty chunks and the root
__global__ void k_list_tree_update(ListTreeArgs a);
// several resident trees in one launch (tree_many_api.cpp): the descriptors by value, 1.4 KB of kernel arguments
constexpr uint32_t kTreesMax = 16;
struct TreesArgs {
    ListTreeArgs t[kTreesMax];  // tree blockIdx.y; at most one chunk (no levels): root over the raw chunk
    uint32_t coff[kTreesMax];   // byte offset (4-B aligned) of the tree's root in the container, 0xffffffff: none
    uint8_t* container;         // the struct's hash message (4-B aligned), NULL: no container
    uint32_t* counter;          // zeroed; the nparts participating trees arrive here
    uint32_t* container_root;   // K(container[0, container_len)), by the last tree to arrive
    uint32_t container_len;
    uint32_t nparts;
};
// grid (blocks of the largest tree, ntrees): slice y is k_list_tree_update over t[y], then the container
__global__ void k_trees_update(TreesArgs g);
__global__ void k_list_tree_scatter(uint8_t* items, const uint64_t* idx, uint64_t k_idx, uint64_t n_old,
                                    uint64_t n_app, uint32_t item_len, uint32_t unit, const uint8_t* vals);
// device-resident registry tree (struct_tree_api.cpp): the dirty records side by side
__global__ void k_struct_tree_gather(const uint8_t* rec, const uint64_t* idx, uint64_t k_idx, uint64_t n_old,
                                     uint64_t n_app, uint32_t rec_len, uint32_t ext, uint8_t* out);

// device-resident tree of a list of byte strings (bytes_tree_api.cpp): the digests of the dirty
// elements, read in place, into the tree's level 0 (fast32: 32-B elements at a 16-B aligned base)
__global__ void k_bytes_tree_digest(const uint8_t* elems, uint32_t elem_len, uint32_t fast32, const uint64_t* idx,
                                    uint64_t k_idx, uint64_t n_old, uint64_t n_app, uint4* digests);

// stage 0 of several resident trees in one launch (tree_many_api.cpp): the segment descriptors by
// value, 1.8 KB of kernel arguments.  Work item v of a segment is listed index idx[v] (v < k_idx,
// skipped when >= n_old), then appended item n_old + (v - k_idx); its value is vals + v * item_len.
constexpr uint32_t kStage0Digest = 0x100;    // mode: element digests (elem_digest_any)
constexpr uint32_t kStage0Digest32 = 0x101;  // ... of 32-B elements at a 16-B aligned `vals` (elem32_digest)
struct Stage0Seg {
    uint8_t* dst;          // scatter: the item buffer (or level 0, item_len 32); digest: level 0
    const uint8_t* vals;   // the staged values of the k_idx + n_app work items, in work-item order
    const uint64_t* idx;
    uint64_t k_idx, n_old, n_app;
    uint32_t item_len;
    uint32_t mode;         // 8 or 1: scatter in pieces of that many bytes, one per thread; kStage0Digest*
};
constexpr uint32_t kStage0SegsMax = 2 * kTreesMax;
struct Stage0Args {
    Stage0Seg s[kStage0SegsMax];  // segment blockIdx.y
};
// grid (blocks of the largest segment, nseg): slice y is k_list_tree_scatter or k_bytes_tree_digest
// (from the staged values) over s[y]; a block beyond its segment's work returns at once
__global__ void k_trees_stage0(Stage0Args g);

// stable erase of a resident tree (list_tree_api.cpp): destinations [first, first +
// moved) of a list gathered out of place, destination q from source q + j (tree_compact.hpp).  A
// segment is one array that moves that way: the value buffer, and level 0 of a struct / bytes tree.
struct CompactSeg {
    const uint8_t* src;  // the value at position `first` of the source array
    uint8_t* dst;        // where destination `first` goes (no overlap with any segment's source)
    uint32_t item_len;
    uint32_t unit;       // 16, 8, 4 or 1: bytes per thread; divides item_len and both addresses
};
struct CompactArgs {
    CompactSeg s[2];     // segment blockIdx.y
    const uint64_t* rm;  // k_rm strictly ascending removed indices (device); k_rm == 0: a plain copy
    uint64_t k_rm, first, moved;
};
// grid (blocks of the larger segment, nseg), 256 threads; a block beyond its segment's pieces returns at once
__global__ void k_tree_compact(CompactArgs g);

// Merkle proofs of a resident list tree (tree_branch_api.cpp; the arithmetic: list_branch.hpp).
// One record per wave and turn, kBranchWaves waves per workgroup: the item's 256-B window, then sib[1 .. D - 1].
__global__ void k_list_tree_branches(const uint8_t* level0, const uint4* levels, uint64_t n, uint64_t capacity,
                                     uint32_t item_len, const uint64_t* indices, uint64_t k, uint4* out);
// one proof per thread: the window with the caller's value in place, the fold, the mix-in, the container
__global__ void k_verify_list_branches(const uint8_t* values, const uint64_t* indices, uint64_t k, uint64_t n,
                                       uint32_t item_len, const uint8_t* branches, const uint8_t* roots,
                                       uint32_t root_stride, const uint8_t* container, uint32_t container_len,
                                       uint32_t container_off, uint8_t* ok);

// Copy of up to kTreesMax resident trees from the layout of one capacity into that of another, plus one
// optional 32-byte extra (tree_copy_api.cpp; the piece map: tree_copy.hpp).  The descriptors
// by value, 1.6 KB of kernel arguments: nothing is uploaded.
struct CopyTree {
    const uint8_t *src_items, *src_level0, *src_levels, *src_root;  // level0, levels and root 16-B aligned
    uint8_t *dst_items, *dst_level0, *dst_levels, *dst_root;
    uint64_t n, cap_src, cap_dst;
    uint32_t item_len;
    uint32_t level0;  // a struct / bytes tree: 32 n bytes of level 0 travel
};
struct TreesCopyArgs {
    CopyTree t[kTreesMax];
    const uint8_t* extra_src;  // 32 bytes, 16-B aligned; NULL: none
    uint8_t* extra_dst;
    uint32_t ntrees;
};
constexpr uint32_t kCopyThreads = 256;  // a workgroup
constexpr uint32_t kCopyUnroll = 4;     // 16-byte pieces a thread has in flight per turn
// a bounded grid striding over the 16-byte pieces of all the trees; every thread writes only its own pieces
__global__ void k_trees_copy(TreesCopyArgs g);

// Audit of up to kTreesMax resident trees and their container (tree_audit_api.cpp; the work-item
// map: tree_audit.hpp): every stored node of level >= 1, every root and the container checks in one launch.
// The descriptors by value, 0.8 KB of kernel arguments; nothing but the reports is written.
struct AuditTree {
    const uint8_t *level0, *levels, *root;  // level 0: the items of a list tree, else the 32-B roots / digests
    uint64_t n, capacity;
    uint32_t len0;  // bytes of a level-0 entry: 1 .. 128
    uint32_t coff;  // the root's offset in the container message, 0xffffffff: none
};
// a report as the kernels keep it until k_audit_reports(finish) unpacks the key: mk_audit_report's 24 bytes
struct AuditReport {
    uint64_t bad;
    uint64_t key;  // audit_key(level, index) of the first mismatch, kAuditKeyNone: none; then first_index
    uint32_t first_level, pad;
};
struct TreesAuditArgs {
    AuditTree t[kTreesMax];
    const uint8_t* container;       // the hash message, 4-B aligned; NULL: no container
    const uint8_t* container_root;  // 32 bytes
    AuditReport* reports;           // ntrees + 1, the last the container's
    uint32_t container_len;
    uint32_t ntrees;
};
constexpr uint32_t kAuditThreads = 256;
// a bounded grid striding over the work items of all the trees, one Keccak state per lane
__global__ void k_trees_audit(TreesAuditArgs g);
// level 0 of a struct / bytes tree: entries [first, first + m) of the stored level 0 against the m freshly
// hashed ones in `fresh` (the bounded workspace), 32 bytes each; a mismatch goes into *report
__global__ void k_audit_compare(const uint4* fresh, const uint4* stored, uint64_t first, uint64_t m,
                                AuditReport* report);
// count reports: finish == 0 clears them before the checks, finish == 1 unpacks every key into (first_level,
// first_index) after them
__global__ void k_audit_reports(AuditReport* reports, uint32_t count, uint32_t finish);

// Diff of up to kTreesMax pairs of resident trees by Merkle descent (tree_diff_api.cpp; the
// rule: tree_diff.hpp).  The descriptors by value, 1.4 KB of kernel arguments; nothing but the reports and the
// pairs' index buffers is written.
struct DiffTree {
    const uint8_t *a_leaves, *a_levels;  // the leaves: the items of a list tree, else the 32-B roots / digests
    const uint8_t *b_leaves, *b_levels;
    uint64_t n_a, cap_a, n_b, cap_b;
    uint64_t* idx_out;  // max_out slots
    uint64_t max_out;
    uint32_t len0;  // bytes of a leaf: 1 .. 128
    uint32_t pad;
};
// mk_diff_report's 16 bytes
struct DiffReport {
    uint64_t total;        // differing indices, exact
    uint64_t first_index;  // the smallest, ~0: none
};
struct TreesDiffArgs {
    DiffTree t[kTreesMax];
    DiffReport* reports;  // ntrees, cleared before the launch
    uint32_t ntrees;
};
constexpr uint32_t kDiffThreads = 256;
// one work item (a subtree of height h0 of one pair) per workgroup turn, a bounded grid striding over them
__global__ void k_trees_diff(TreesDiffArgs g);
// count reports cleared to (0, ~0)
__global__ void k_diff_reports(DiffReport* reports, uint32_t count);

// Undo journal of up to kTreesMax resident trees and their container (tree_journal_api.cpp; the
// slot map: tree_journal.hpp).  The descriptors by value, 1.5 KB of kernel arguments: nothing is uploaded.
struct JournalSeg {
    uint8_t *items, *level0, *levels, *root;  // the tree; level0 NULL for a list tree
    const uint64_t* idx;                      // journal: the update's k_idx indices (device); restore: unused
    uint8_t* jr;                              // the tree's region of the journal, 16-B aligned
    uint64_t n_old, n_new, capacity, k_idx;
    uint32_t item_len;
    uint32_t unit;  // 16, 8 or 1: bytes per value piece; divides item_len and the value buffer's address
};
struct JournalArgs {
    JournalSeg s[kTreesMax];  // segment blockIdx.y < ntrees; segment ntrees: the container
    uint8_t* container;       // the hash message, 4-B aligned; NULL: no container
    uint8_t* container_root;  // 32 bytes, 4-B aligned
    uint8_t* jr_container;    // up16(container_len) bytes of message, then the 32 bytes of its root
    uint32_t container_len;
    uint32_t ntrees;
};
// grid (blocks of the largest segment, segments), 256 threads, one piece per thread; a block beyond its
// segment's pieces returns at once.  k_trees_journal: tree -> journal; k_trees_restore: journal -> tree
__global__ void k_trees_journal(JournalArgs g);
__global__ void k_trees_restore(JournalArgs g);

// The resident deposit trie rolled back, compared, audited and copied (kernels_trie_admin.hip,
// trie_admin_api.cpp; the rules: trie_admin.hpp).
// one wave: the straddling nodes of a roll back to c <= count stored along the as-of chain, the root to root_out
__global__ void k_trie_truncate(uint4* levels, uint64_t cap, uint64_t count, uint64_t c, uint32_t depth,
                                uint4* root_out);
// one wave: the smallest leaf index below min(count_a, count_b) at which the tries differ, else that minimum
__global__ void k_trie_fork_point(const uint4* a, uint64_t cap_a, uint64_t count_a, const uint4* b, uint64_t cap_b,
                                  uint64_t count_b, uint32_t depth, uint64_t* out);
// a bounded grid of kAuditThreads striding over the live nodes of level 1 .. depth and the root
__global__ void k_trie_audit(const uint4* levels, uint64_t cap, uint64_t count, uint32_t depth, const uint4* root,
                             AuditReport* report);
// a bounded grid of kCopyThreads striding over the 16-byte halves of the live nodes (and the root's, when given)
__global__ void k_trie_copy(const uint4* src, uint64_t cap_src, uint64_t count, uint4* dst, uint64_t cap_dst,
                            uint32_t depth, const uint4* src_root, uint4* dst_root);

// hashutil.RepeatHash in batches (kernels_repeat.hip, repeat_api.cpp; the helpers: repeat_dev.hpp).
enum RepeatMode : int { kRepeatChain = 0, kRepeatOnion = 1, kRepeatVerify = 2 };
struct RepeatArgs {
    const uint8_t* seeds;    // n x 32: the seeds, verify: the reveals
    const uint32_t* layers;  // chain: n trip counts
    uint8_t* out;            // chain: n x 32; onion: n x (max_layers + 1) x 32; verify: n verdict bytes
    uint32_t* status;        // chain: set to 1 when a trip count exceeds max_layers (NULL: the host checked)
    const uint8_t* records;  // verify: n_records records `stride` bytes apart
    const uint64_t* idx;     // verify: n record indices
    uint64_t n, n_records, stride;
    uint32_t commit_off, layers_off;  // verify: the 32-B commitment and the le64 layer count inside a record
    uint32_t max_layers;              // the bound of every chain's trip count; onion: the trip count
    uint32_t io16;   // seeds and (chain, onion) out are 16-B aligned: whole-word accesses, else bytes
    uint32_t rec4;   // verify: records, stride and both offsets are multiples of 4: dword loads, else bytes
};
constexpr uint32_t kRepeatThreads = 256;
constexpr uint32_t kRepeatWaves = kRepeatThreads / 64;  // k_repeat_wave: chains per workgroup
// one chain per GPU lane; a wave runs as long as its longest chain, the shorter ones masked off
template <int MODE>
__global__ void k_repeat_lane(RepeatArgs a);
// one chain per wave (mk::spread), kRepeatWaves chains per workgroup
template <int MODE>
__global__ void k_repeat_wave(RepeatArgs a);

}  // namespace mk
