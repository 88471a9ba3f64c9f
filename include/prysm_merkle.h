/*
 * prysm_merkle.h — C ABI of the MI355X Merkleization engine (libprysm_merkle.so).
 *
 * Drop-in boundary for the Keccak-era Prysm SSZ tree-hash path.  The reference
 * is pure Go with no FFI; these entry points are what a new
 * cgo package `gpu/merkle` binds (INTEGRATION.md shows the binding), called
 * from the unchanged exported Go signatures:
 *
 *   hashutil.Hash(data []byte) [32]byte      shared/hashutil/hash.go:11
 *   ssz.merkleHash(list [][]byte)            shared/ssz/hash.go:194
 *   ssz.TreeHash(val interface{})            shared/ssz/hash.go:23 (via
 *                                            makeSliceHasher hash.go:118-139)
 *   (*trieutil.DepositTrie).UpdateDepositTrie / GenerateMerkleBranch / Root
 *                                            shared/trieutil/deposit_trie.go:29-63
 *   trieutil.VerifyMerkleBranch              shared/trieutil/deposit_trie.go:68-81
 *   hashutil.MerkleRoot                      shared/hashutil/merkleRoot.go:12
 *
 * Conventions
 *   - Every compute entry point takes a per-call context `mk_call*` first
 *     (NULL = defaults).  cgo may run two consecutive C calls of one goroutine
 *     on different OS threads, so the device and the error detail travel with
 *     the call, never with the thread:
 *       call->device  in:  device index; -1 = for dev entry points the device
 *                          of `stream` (the thread's current HIP device when
 *                          stream is NULL), for host-buffer entry points the
 *                          thread's current HIP device (0 unless set).
 *       call->code    out: the status returned.
 *       call->err     out: NUL-terminated detail of a failure ("" on success).
 *     The calling thread's current HIP device is the same after the call as
 *     before it.  mk_last_error() keeps the thread's last detail for C callers.
 *   - Every function returns 0 (MK_OK) or a negative MK_E* code; mk_strerror()
 *     names it.  Nothing panics across the boundary; there is NO CPU
 *     fallback: without a usable gfx950 device every compute entry point
 *     returns MK_ENODEV.
 *   - Host-buffer entry points (no `dev` in the name) borrow caller memory for
 *     the duration of the call only (cgo rule: Go memory is never retained);
 *     `[][]byte` inputs are passed flattened as (data, offs[n+1]).
 *   - `dev` entry points take device pointers (HBM-resident inputs) and a
 *     hipStream_t passed as void* (NULL = the device's default stream); they
 *     enqueue work and return without synchronising.  Their scratch space is
 *     caller-provided (size from the *_workspace_bytes query), so they never
 *     allocate and can be captured into a hipGraph -- except
 *     mk_dev_ssz_merkle_many (host-planned descriptors, uploaded per call)
 *     and mk_dev_ssz_merkle_hash_multi (RCCL, library workspaces), which
 *     refuse / are not meant for capture.
 *   - Thread safety: every entry point may be called concurrently from any OS
 *     thread; host-buffer entry points take a per-device lock, deposit-trie
 *     and list-tree handles a per-handle lock.
 *   - Digests are 32 bytes; node arrays are n x 32 contiguous bytes.
 */
#ifndef PRYSM_MERKLE_H
#define PRYSM_MERKLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_OK 0
#define MK_EINVAL (-22)  /* bad argument (also: reference panics, e.g. len(list[0]) == 0) */
#define MK_ENODEV (-19)  /* no usable gfx950 device / device index out of range */
#define MK_ENOMEM (-12)  /* device or host allocation failed / workspace too small */
#define MK_EHIP (-5)     /* a HIP runtime call failed (see call->err) */
#define MK_ECOMM (-71)   /* RCCL failure in the multi-device path */

#define MK_ERR_LEN 256
typedef struct mk_call {
    int32_t device;         /* in: device index, -1 = default (see Conventions) */
    int32_t code;           /* out: status of the call */
    char err[MK_ERR_LEN];   /* out: detail of a failure, "" on success */
} mk_call;

/* ---- lifecycle --------------------------------------------------------- */
int mk_init(int device);          /* idempotent: creates `device`'s streams; 0 ok */
int mk_device_count(void);        /* number of visible gfx950 devices (0 if none) */
const char* mk_strerror(int code);
const char* mk_last_error(void);  /* the calling thread's last failure detail */
const char* mk_version(void);

/* ---- hashutil.Hash (hash.go:11-25): legacy Keccak-256 ------------------- */
/* Single message.  Provided for completeness; Go keeps single Hash calls on
 * the CPU (launch latency, and Hash cannot return an error). */
int mk_hash(mk_call* call, const uint8_t* data, uint64_t len, uint8_t out[32]);
/* Batched form ("HashBatch"): n messages of msg_len bytes, contiguous -> n*32. */
int mk_hash_batch(mk_call* call, const uint8_t* in, uint64_t n, uint32_t msg_len, uint8_t* out);
/* Variable-length batch: message i = in[offs[i], offs[i+1]) -> n*32. */
int mk_hash_batch_var(mk_call* call, const uint8_t* in, const uint64_t* offs, uint64_t n, uint8_t* out);
int mk_dev_hash_batch(mk_call* call, const void* d_in, uint64_t n, uint32_t msg_len, void* d_out, void* stream);
int mk_dev_hash_batch_var(mk_call* call, const void* d_in, const uint64_t* d_offs, uint64_t n, void* d_out,
                          void* stream);

/* ---- ssz.merkleHash (hash.go:194-239) ---------------------------------- */
/* n items of item_len bytes each, contiguous (the flattened [][]byte; every
 * list TreeHash builds has uniform element length).  out = 32-B result.
 * item_len == 0 with n > 0 is the reference's divide-by-zero panic: MK_EINVAL. */
int mk_ssz_merkle_hash(mk_call* call, const uint8_t* items, uint64_t n, uint32_t item_len, uint8_t out[32]);
/* Workspace of mk_dev_ssz_merkle_hash, exact: one byte less is MK_ENOMEM
 * before anything is launched, whatever the alignment of d_items and d_ws
 * (items that are not 16-B aligned never need more).  A 16-B aligned d_ws lets
 * lists of 17 .. 4096 first-level windows take the latency list tree; any
 * other d_ws takes the planner's passes to the same root.  With at most one
 * chunk nothing is read from the workspace (the query still returns 256). */
uint64_t mk_ssz_merkle_workspace_bytes(uint64_t n, uint32_t item_len);
int mk_dev_ssz_merkle_hash(mk_call* call, const void* d_items, uint64_t n, uint32_t item_len, void* d_out32,
                           void* d_ws, uint64_t ws_bytes, void* stream);

/* Many lists in one call (makeSliceHasher over a list of lists, a struct's
 * list fields, a state's lists): list i = n[i] items of item_len[i] bytes at
 * byte offset offs[i] of d_items (16-B aligned offsets take the streaming
 * path); d_roots[i] (32 B each) = merkleHash(list i).  offs, n and item_len
 * are HOST arrays (the library plans on the host and uploads the per-list
 * descriptors into the workspace).  Lists of up to 2^15 chunks share one leaf
 * launch and one launch per level; longer lists run their own fused passes.
 * Workspace from mk_ssz_merkle_many_workspace_bytes (same n, item_len).
 * The descriptors go through a small pinned host ring on every call, so the
 * call cannot be captured into a hipGraph: on a capturing stream it returns
 * MK_EINVAL. */
uint64_t mk_ssz_merkle_many_workspace_bytes(const uint64_t* n, const uint32_t* item_len, uint32_t nlists);
int mk_dev_ssz_merkle_many(mk_call* call, const void* d_items, const uint64_t* offs, const uint64_t* n,
                           const uint32_t* item_len, uint32_t nlists, void* d_roots, void* d_ws, uint64_t ws_bytes,
                           void* stream);
/* Host-buffer form: list i = items[offs[i], offs[i] + n[i]*item_len[i]). */
int mk_ssz_merkle_many(mk_call* call, const uint8_t* items, const uint64_t* offs, const uint64_t* n,
                       const uint32_t* item_len, uint32_t nlists, uint8_t* roots);

/* ---- ssz.TreeHash of a list of byte strings (hash.go:100-107, 118-139) -- */
/* TreeHash([][N]byte) / TreeHash([][]byte) with n elements of elem_len bytes
 * each, contiguous: makeSliceHasher hashes every element with hashedEncoding
 * (Keccak(le32(elem_len) || element)) and runs merkleHash over those 32-B
 * digests.  One call, no host round trip: with 32-B elements (16-B aligned)
 * the digests are computed inside the tree's leaf pass and never reach HBM.
 * Workspace from mk_ssz_tree_hash_bytes_list_workspace_bytes (for a 16-B
 * aligned d_elems; other alignments take the two-phase form and need that
 * size plus n*32 rounded up to 256, and report MK_ENOMEM below it). */
uint64_t mk_ssz_tree_hash_bytes_list_workspace_bytes(uint64_t n, uint32_t elem_len);
int mk_dev_ssz_tree_hash_bytes_list(mk_call* call, const void* d_elems, uint64_t n, uint32_t elem_len,
                                    void* d_out32, void* d_ws, uint64_t ws_bytes, void* stream);
int mk_ssz_tree_hash_bytes_list(mk_call* call, const uint8_t* elems, uint64_t n, uint32_t elem_len,
                                uint8_t out[32]);

/* ---- device-resident list tree: merkleHash re-hashed from changed items --- */
/* The tree of ssz.merkleHash over n items of item_len bytes (flat,
 * contiguous), every level kept in HBM, so that a changed or appended item
 * costs its chunk's ancestors (O(changed x depth) hashes) instead of the
 * whole list.  Layout: p = 128 / item_len items per chunk (1 when item_len >=
 * 128), nchunks = ceil(n / p), cap_chunks the same of `capacity`.  Level 0 is
 * the caller's item buffer and is never copied.  Level d (1 <= d <= D, D the
 * first level with ceil(cap_chunks / 2^d) == 1) starts at node
 * sum_{1<=i<d} ceil(cap_chunks / 2^i) of the level array and holds
 * ceil(nchunks / 2^d) nodes of 32 B: node j = Keccak(child 2j || child 2j+1),
 * a missing right child being 0^128 (hash.go:229-236).  Every level up to the
 * current top (the first with one node) is stored; nodes beyond those counts
 * and levels above the top are unspecified.  root = Keccak(top || le64(n) ||
 * 0^24); with nchunks <= 1 there are no levels and top is the raw chunk
 * (0^128 when n == 0).  A grown tree gains levels above its old top, which
 * stays node 0 of its level.  item_len is 1 .. 2^30.
 * mk_ssz_list_tree_levels_bytes: bytes of the level array (0 for item_len ==
 * 0 or cap_chunks <= 1); d_levels is 16-B aligned.
 * Replaces: ssz.merkleHash (shared/ssz/hash.go:194-239) for a list whose tree
 * is already built. */
uint64_t mk_ssz_list_tree_levels_bytes(uint64_t capacity, uint32_t item_len);
/* All levels and the root of n <= capacity items. */
uint64_t mk_ssz_list_tree_build_workspace_bytes(uint64_t n, uint32_t item_len);
int mk_dev_ssz_list_tree_build(mk_call* call, const void* d_items, uint64_t n, uint64_t capacity, uint32_t item_len,
                               void* d_levels, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream);
/* Re-hash after a change: d_idx holds k_idx strictly ascending item indices
 * < n_old (device memory) whose items changed; items [n_old, n_new) are
 * appended (n_old <= n_new <= capacity).  d_values != NULL: k_idx new item
 * values, then n_new - n_old appended ones, item_len bytes each, scattered
 * into d_items first by the same call; NULL: the caller has already written
 * the new bytes into d_items on this stream.  Recomputes exactly the
 * ancestors of the changed chunks and writes the root to d_root32 (also when
 * nothing changed).  An index >= n_old is ignored; a list that is not
 * ascending gives an undefined root but no access outside the buffers.
 * Workspace (8-B aligned) from mk_ssz_list_tree_update_workspace_bytes(k),
 * k = k_idx + n_new - n_old (< 2^31): the call zeroes and owns it until it has
 * run, so trees updated concurrently on different streams need a workspace
 * each; too small is MK_ENOMEM.  item_len == 0, n_new < n_old and n_new >
 * capacity are MK_EINVAL. */
uint64_t mk_ssz_list_tree_update_workspace_bytes(uint64_t k);
int mk_dev_ssz_list_tree_update(mk_call* call, void* d_items, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                uint32_t item_len, void* d_levels, const uint64_t* d_idx, uint64_t k_idx,
                                const void* d_values, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream);
/* Shrink on the device, one entry for both forms.
 * Erase: d_rm holds k_rm > 0 strictly ascending item indices < n_old (device
 * memory, 8-B aligned) that leave the list; the survivors close the gaps in
 * order (a stable compaction) and n_new must be n_old - k_rm.  `first` is a
 * host-side lower bound of the removed indices: items below it are not
 * touched (0 is always allowed and only costs time), first <= n_new.
 * Truncate: k_rm == 0 and n_new <= n_old given explicitly, the first n_new
 * items stay (d_rm and first's value are unused, first <= n_new still holds).
 * The items move inside d_items (through the workspace); the tree is climbed
 * from the first moved item, or its levels rebuilt when that is cheaper;
 * nodes to the right of the new end stay unspecified.  The root, with n_new
 * mixed in, goes to d_root32.  Workspace (8-B aligned, 16 B lets 16-B items
 * move in 16-B pieces) from mk_ssz_list_tree_erase_workspace_bytes(moved,
 * item_len), moved = n_new - first for an erase (< 2^31) and 0 for a
 * truncate; 0 for item_len == 0 or moved >= 2^31.  Every argument is checked
 * before a device is looked up: null or misaligned pointers, n_new > n_old,
 * k_rm > n_old, n_new != n_old - k_rm, first > n_new are MK_EINVAL, a short
 * workspace MK_ENOMEM.  A list that is not ascending gives an undefined list
 * and root but no access outside the buffers.  Allocates nothing: capturable
 * into a hipGraph.  mk_dev_ssz_list_tree_update still rejects n_new < n_old. */
uint64_t mk_ssz_list_tree_erase_workspace_bytes(uint64_t moved, uint32_t item_len);
int mk_dev_ssz_list_tree_erase(mk_call* call, void* d_items, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                               uint32_t item_len, void* d_levels, const uint64_t* d_rm, uint64_t k_rm, uint64_t first,
                               void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream);
/* Handle form for host callers: items and levels stay in HBM under a
 * per-handle lock (the validator registry's roots, the balances).  update
 * takes host indices in any order (list[idx[j]] = values[j] in sequence: of a
 * repeated index the last value wins; an index >= count is MK_EINVAL and
 * nothing changes) and uploads only the k indices and values; append past the
 * capacity doubles it and rebuilds; a call that dirties 1/512 of the list or
 * more rebuilds instead of climbing.  The root of a new handle is
 * merkleHash([]). */
typedef struct mk_list_tree mk_list_tree;
int mk_list_tree_new(mk_call* call, uint32_t item_len, uint64_t capacity, mk_list_tree** out);
void mk_list_tree_free(mk_list_tree* t);
uint64_t mk_list_tree_count(const mk_list_tree* t);
/* Replaces the whole list by n items. */
int mk_list_tree_assign(mk_call* call, mk_list_tree* t, const uint8_t* items, uint64_t n);
int mk_list_tree_update(mk_call* call, mk_list_tree* t, const uint64_t* idx, const uint8_t* values, uint64_t k);
int mk_list_tree_append(mk_call* call, mk_list_tree* t, const uint8_t* items, uint64_t k);
/* Shrink without giving the residency up: truncate keeps the first n items
 * (n > count is MK_EINVAL, n == count a no-op); erase removes the items at the
 * k host indices (any order, a repeated index counts once; an index >= count
 * is MK_EINVAL and nothing changes; k == 0 a no-op) and closes the gaps in
 * order.  Only the sorted indices are uploaded; capacity and buffers stay. */
int mk_list_tree_truncate(mk_call* call, mk_list_tree* t, uint64_t n);
int mk_list_tree_erase(mk_call* call, mk_list_tree* t, const uint64_t* idx, uint64_t k);
int mk_list_tree_root(mk_call* call, mk_list_tree* t, uint8_t root[32]);
/* Items [first, first + cnt), cnt x item_len bytes. */
int mk_list_tree_items(mk_call* call, mk_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out);
/* Merkle proofs out of a resident tree and their batched verifier (DESIGN.md
 * §5l).  For n items of s = item_len bytes, 1 <= s <= 128: p = 128 / s items
 * per chunk, cb = p * s, nchunks = ceil(n / p), total = n * s, D the smallest
 * d with ceil(nchunks / 2^d) == 1.  The record of item i < n is
 * 256 + 32 * max(D - 1, 0) bytes (mk_ssz_list_branch_bytes; 0 for item_len 0
 * or above 128): window[256] = the list bytes [2 j cb, min(total, (2 j + 2)
 * cb)) with j = (i / p) / 2 ([0, total) for nchunks <= 1), zeros after them;
 * then sib[d], d = 1 .. D - 1: the stored level-d node (j >> (d - 1)) ^ 1, or
 * 0^32 when that index is >= ceil(nchunks / 2^d).  The level-1 sibling is in
 * the window.  The record of an index >= n is all zeros (device indices are
 * not checked on the host).
 * mk_dev_ssz_list_tree_branches gathers k records (k x stride bytes, 16-B
 * aligned) from d_level0 -- the item buffer of a list tree, or d_roots /
 * d_digests of a struct / bytes tree with item_len = 32 -- and the level array
 * of mk_ssz_list_tree_levels_bytes(capacity, item_len).  No node at or beyond
 * a level's current count and no item byte at or beyond total is read.  One
 * launch: allocates nothing, never synchronises, capturable into a hipGraph.
 * Verify (value, i, n, s, record, root), false for i >= n: the window with
 * the value written over the item's bytes; for nchunks <= 1 top = its first
 * total bytes, else node = K(window[0, wl)) (0^128 appended when 2 j + 1 ==
 * nchunks) folded for d = 1 .. D - 1 with q = j >> (d - 1): K(sib[d] || node)
 * for odd q, K(node || sib[d]) when q + 1 < ceil(nchunks / 2^d), else
 * K(node || 0^128) (the slot is ignored); list_root = K(top || le64(n) ||
 * 0^24).  With d_container (container_len <= MK_CONTAINER_MAX, container_off
 * + 32 <= container_len) the compared value is K(container with list_root at
 * container_off), else list_root; against d_roots[0] (root_stride 0) or
 * d_roots[32 g] (root_stride 32).  d_ok: one byte per proof.
 * Every argument check comes before a device is looked up: null or
 * misaligned pointers, item_len 0 or above 128, n > capacity, k >= 2^31, a
 * root_stride other than 0 or 32 and a bad container_off are MK_EINVAL. */
uint64_t mk_ssz_list_branch_bytes(uint64_t n, uint32_t item_len);
int mk_dev_ssz_list_tree_branches(mk_call* call, const void* d_level0, uint64_t n, uint64_t capacity,
                                  uint32_t item_len, const void* d_levels, const uint64_t* d_idx, uint64_t k,
                                  void* d_branches, void* stream);
int mk_dev_verify_list_branches(mk_call* call, const void* d_values, const uint64_t* d_idx, uint64_t k, uint64_t n,
                                uint32_t item_len, const void* d_branches, const void* d_roots, uint32_t root_stride,
                                const void* d_container, uint32_t container_len, uint32_t container_off, void* d_ok,
                                void* stream);
int mk_verify_list_branches(mk_call* call, const uint8_t* values, const uint64_t* idx, uint64_t k, uint64_t n,
                            uint32_t item_len, const uint8_t* branches, const uint8_t* roots, uint32_t root_stride,
                            const uint8_t* container, uint32_t container_len, uint32_t container_off, uint8_t* ok);
/* Handle form: the proofs of the items at k host indices (any order, repeats
 * allowed; an index >= count is MK_EINVAL and nothing is written; k == 0 a
 * no-op).  values_out gets the k level-0 values (k x item_len bytes; 32-B
 * struct roots / element digests for the other two kinds), branches_out the k
 * records of mk_ssz_list_branch_bytes(count, item_len or 32) bytes.  One upload
 * of the indices, one launch, one read-back.  item_len above 128 is MK_EINVAL. */
int mk_list_tree_branches(mk_call* call, mk_list_tree* t, const uint64_t* idx, uint64_t k, uint8_t* values_out,
                          uint8_t* branches_out);

/* ---- subtree sharding across GPUs ----------------------- */
/* Split a merkleHash of n items over `nshards` devices: every shard is a
 * power-of-two-aligned run of 2^height chunks.  item_begin[nshards+1] gets
 * each shard's item range (empty shards have begin == end); *nonempty the
 * number of non-empty shards.  When the tree is too small to shard
 * (*nonempty == 1) shard 0 holds everything and is hashed with
 * mk_dev_ssz_merkle_hash instead. */
int mk_ssz_merkle_shard_plan(mk_call* call, uint64_t n, uint32_t item_len, uint32_t nshards, uint32_t* height,
                             uint32_t* nonempty, uint64_t* item_begin);
/* Root (32 B, height `height` above the chunks) of one shard.  pad_at_one=1
 * for every shard of a tree with >1 non-empty shard: a ragged last shard keeps
 * applying the reference's odd rule (node || 0^128) up to `height`.
 * Workspace: mk_ssz_merkle_workspace_bytes(shard_n, item_len), the query of a
 * merkleHash over the shard's own items -- its plan bounds the subtree plan at
 * every height, pad_at_one and alignment; less is MK_ENOMEM before any launch.
 * The query is not monotonic in n: a workspace shared by shards of different
 * sizes takes the largest of their queries. */
int mk_dev_ssz_merkle_subtree(mk_call* call, const void* d_shard_items, uint64_t shard_n, uint32_t item_len,
                              uint32_t height, int pad_at_one, void* d_out32, void* d_ws, uint64_t ws_bytes,
                              void* stream);
/* Frontier variant: stop `frontier_log2` levels below the shard root and
 * write the shard's nodes at height (height - frontier_log2) to d_out (32 B
 * each, 2^frontier_log2 of them, fewer for a ragged last shard; *nodes_out
 * gets the count).  The shards' frontiers, concatenated in shard order, are
 * that level of the whole tree, so ranks gather a few KB each and the top
 * levels move to the finisher (mk_dev_ssz_merkle_finish_nodes), which can
 * overlap the ranks' next Merkleization.  0 < frontier_log2 < height; a
 * frontier one level above the chunks (frontier_log2 == height - 1) of a shard
 * of more than 2^17 first-level windows is MK_EINVAL.  d_out holds 32 <<
 * frontier_log2 bytes, of which only the first 32 * *nodes_out are written.
 * Workspace: mk_ssz_merkle_workspace_bytes(shard_n, item_len), as for
 * mk_dev_ssz_merkle_subtree (it bounds every frontier plan too). */
int mk_dev_ssz_merkle_subtree_frontier(mk_call* call, const void* d_shard_items, uint64_t shard_n,
                                       uint32_t item_len, uint32_t height, uint32_t frontier_log2, int pad_at_one,
                                       void* d_out, uint64_t* nodes_out, void* d_ws, uint64_t ws_bytes,
                                       void* stream);
/* The same subtree continued from one of its node levels: `count` 32-B nodes
 * (a shard's level, e.g. the output of the leaf pass) reduced for `height`
 * levels with the reference's odd rule (hash.go:225-235; pad_at_one as
 * above), stopping `frontier_log2` levels below the top (0 = to the top
 * node).  Lets a rank split its shard into the leaf pass and the narrower
 * node passes and run the latter on another stream (prysm_amd/parallel.py
 * ShardedMerklePipeline).  Workspace from
 * mk_ssz_merkle_node_frontier_workspace_bytes. */
uint64_t mk_ssz_merkle_node_frontier_workspace_bytes(uint64_t count, uint32_t height, uint32_t frontier_log2);
int mk_dev_ssz_merkle_node_frontier(mk_call* call, const void* d_nodes, uint64_t count, uint32_t height,
                                    uint32_t frontier_log2, int pad_at_one, void* d_out, uint64_t* nodes_out,
                                    void* d_ws, uint64_t ws_bytes, void* stream);
/* Finisher over `count` nodes forming one complete tree level in order (the
 * gathered frontiers): the reference level loop (odd -> 0^128 pad) and
 * Keccak(root || le64(n_total) || 0^24).  Workspace from
 * mk_ssz_merkle_finish_workspace_bytes(count). */
uint64_t mk_ssz_merkle_finish_workspace_bytes(uint64_t count);
int mk_dev_ssz_merkle_finish_nodes(mk_call* call, const void* d_nodes, uint64_t count, uint64_t n_total,
                                   void* d_out32, void* d_ws, uint64_t ws_bytes, void* stream);
/* The same finisher for one field of a two-field struct whose fields are
 * both lists (hash.go:141-159; the State{registry, balances} of BASELINE
 * config 3): the list root goes to d_pair_block[32 slot, 32 slot + 32), and
 * whichever of the two finishers of one pair (slot 0 and slot 1, the same
 * `epoch`, launched in any order on any streams; neither waits for the other)
 * completes second writes the struct root Keccak(d_pair_block[0, 64)) to
 * d_pair_block[64, 96).  d_pair_block[96, 100) is the arrival word: zero
 * before the block's first use, then owned by the finishers.  Each pair takes
 * the next epoch of a counter over 1 .. 2^30 - 1 (wrapping; "newer" = ahead by
 * less than 2^29), so a pair left half-done by a failed call never completes
 * with the next one, and a finisher whose epoch is already behind the word's
 * when it starts is ignored.  That check is best-effort (it precedes the
 * finisher's slot store): two epochs' finishers of one slot must not run
 * concurrently -- order them on one stream or by events.  The
 * first finisher of an epoch zeroes d_pair_block[64, 96), so a pair that
 * never completes reads back as zeros, not as the previous pair's root.  The
 * block is MK_PAIR_BLOCK_BYTES, 16-B aligned; the caller waits for both
 * finishers before reading the struct root. */
#define MK_PAIR_BLOCK_BYTES 128
int mk_dev_ssz_merkle_finish_nodes_pair(mk_call* call, const void* d_nodes, uint64_t count, uint64_t n_total,
                                        void* d_pair_block, uint32_t slot, uint32_t epoch, void* d_ws,
                                        uint64_t ws_bytes, void* stream);
/* One or two lists' trees above a complete node level, to the roots, in ONE
 * launch (round 6): `count0` 32-B nodes at d_nodes0 (8-B
 * aligned) forming one complete level of a list of `n0` items, reduced with
 * the reference level loop (hash.go:225-236, odd -> 0^128) and mixed in
 * (Keccak(root || le64(n0) || 0^24), :237-238); count1 == 0: d_out gets the
 * 32-B list root.  count1 > 0: a second list (d_nodes1, count1, n1) side by
 * side, and d_out is a pair block laid out as for
 * mk_dev_ssz_merkle_finish_nodes_pair (list 0's root at [0, 32), list 1's at
 * [32, 64), the struct root Keccak(d_out[0, 64)) at [64, 96) written by
 * whichever list finishes second; both finishers are in this launch, so the
 * arrival word at [96, 100) is not used; `epoch` is range-checked, 1 .. 2^30
 * - 1, only for symmetry with the pair finishers and otherwise unused -- the
 * launch synchronises on an arrival counter): the State root of BASELINE config 3 from the two
 * trees' level-1 nodes in one call on one stream.  Each count is 1 .. 2^20; at most
 * 4096 such launches in flight per device (arrival counters).  Workspace from
 * mk_ssz_merkle_top_fused_workspace_bytes(count0, count1), 16-B aligned.
 * Replaces: ssz.merkleHash's level loop (shared/ssz/hash.go:223-239) for a
 * list whose lower levels are already built. */
uint64_t mk_ssz_merkle_top_fused_workspace_bytes(uint64_t count0, uint64_t count1);
int mk_dev_ssz_merkle_top_fused(mk_call* call, const void* d_nodes0, uint64_t count0, uint64_t n0,
                                const void* d_nodes1, uint64_t count1, uint64_t n1, void* d_out, uint32_t epoch,
                                void* d_ws, uint64_t ws_bytes, void* stream);
/* Finisher on one device: the reference level loop over the `nroots`
 * gathered shard roots (odd -> 0^128 pad), then Keccak(root || le64(n) || 0^24). */
int mk_dev_ssz_merkle_finish(mk_call* call, const void* d_roots, uint64_t nroots, uint64_t n_total, void* d_out32,
                             void* stream);
/* Single-process multi-device merkleHash for the cgo caller.  The items are
 * split by mk_ssz_merkle_shard_plan into `nshards` shards; shard s runs on
 * device devs[s] (devs == NULL: device s).  Every device uploads its shards
 * from its own host thread (chunked async copies from the caller's buffer),
 * so the PCIe links copy in parallel and a shard's passes overlap the upload
 * of the device's next shard; every shard is reduced to its frontier level (up to 1024
 * nodes).  When each device holds exactly one shard the frontiers are
 * all-gathered over RCCL (xGMI); otherwise they are copied to devs[0].  The
 * top levels and the length mix-in finish on devs[0]. */
int mk_ssz_merkle_hash_multi(mk_call* call, const uint8_t* items, uint64_t n, uint32_t item_len, int nshards,
                             const int* devs, uint8_t out[32]);
/* Device-resident form on devices 0..ndev-1 (one shard per device, shard d =
 * items [item_begin[d], item_begin[d+1]) of mk_ssz_merkle_shard_plan(n,
 * item_len, ndev), at d_shards[d] on device d).  Each device reduces its
 * shard to its frontier on streams[d] (NULL entries: the library's stream of
 * that device), the frontiers are all-gathered over RCCL and device 0
 * finishes into d_out32 (device 0 memory).  Enqueues only; the library's
 * per-device workspaces are reused by the next call, so successive calls
 * must be on the same streams (or synchronised). */
int mk_dev_ssz_merkle_hash_multi(mk_call* call, const void* const* d_shards, uint64_t n, uint32_t item_len,
                                 int ndev, void* d_out32, void* const* streams);

/* ---- struct hashing (hash.go:141-159) for flat fixed-layout records ------ */
/* The typed-registry path behind ssz.Hashable (hash.go:18-20, 57-58): a Go
 * wrapper flattens []*ValidatorRecord into n records of record_len bytes once
 * and describes the fields in declaration order ("XXX" fields omitted, as
 * structFields does, ssz_utils_cache.go:100).  Field hash = MK_FIELD_BYTES:
 * Keccak(le32(len) || bytes) (offset must be 4-byte aligned, record_len too);
 * MK_FIELD_RAW: raw little-endian scalar of len 1/2/4/8 (not hashed).
 * The struct root is Keccak(concat of field outputs).
 *
 * The rest of makeStructHasher's type grammar (hash.go:141-178) keeps records
 * flat, fixed-length and 4-byte aligned; there is no side heap:
 * MK_FIELD_VARBYTES: a []byte of varying length in a slot of 4 + len bytes at
 * a 4-byte aligned offset: le32(L), then L bytes, 0 <= L <= len (the capacity;
 * the slot's other len - L bytes are ignored).  Field hash = Keccak(record[
 * offset, offset + 4 + L)), which is hashedEncoding of the []byte
 * (hash.go:100-107).  Device entry points cannot report a bad L: they clamp it
 * to len and never read outside the slot.  The host-buffer and handle entry
 * points (mk_ssz_struct_roots, mk_ssz_struct_list_root,
 * mk_struct_list_tree_assign/update/append) check every record they are given
 * and return MK_EINVAL, changing nothing, when some L > len.
 * MK_FIELD_STRUCT: a nested struct, by value or by non-nil pointer
 * (makePtrHasher only dereferences).  len = the number of mk_field entries
 * that follow and belong to it, all its descendants flattened in pre-order
 * (len == 0 is MK_EINVAL); offset must be 0, the children carry absolute
 * record offsets.  Field hash = Keccak(concat of its direct children's
 * outputs).  Nesting depth at most 4, the top-level struct counting as 1;
 * at most 32 entries in all.
 * Layouts with either kind hash in one launch, one record per thread, with
 * each struct's message staged in LDS: the message lengths along any one
 * root-to-leaf nesting path may sum to at most 320 bytes (each rounded up to
 * 4), otherwise the layout is MK_EINVAL; their records must be 4-byte aligned.
 *
 * MK_FIELD_LIST: a slice ([]T) of fixed-size items in a slot at a 4-byte
 * aligned offset: le32(count), then len (the capacity, >= 1) item cells of
 * `stride` bytes each; the cells beyond count are ignored.  The entry {LIST,
 * offset, cap} is followed by exactly one item descriptor whose offset member
 * carries the stride:
 *   {MK_FIELD_RAW, stride, len}    len 1/2/4/8 and stride == len; the element
 *                                  hash is the raw encoding
 *   {MK_FIELD_BYTES, stride, N}    N % 4 == 0, stride % 4 == 0, stride >= N;
 *                                  the element hash is Keccak(le32(N) || bytes)
 *   {MK_FIELD_STRUCT, stride, k}   plus its k flattened descendants (RAW,
 *                                  BYTES, VARBYTES, STRUCT; no LIST) at
 *                                  offsets inside the cell; stride % 4 == 0 and
 *                                  covers every child; the element hash is the
 *                                  struct hash.  The item struct counts as one
 *                                  nesting level.
 * Field hash = merkleHash of the count element hashes (hash.go:194-239):
 * 128 / out_len items per chunk (out_len = len for RAW items, else 32), the
 * last chunk short, no item = one chunk of 128 zero bytes, an odd level of
 * more than one node padded with 128 zero bytes, and Keccak(top ||
 * le64(count) || 0^24).  A list may stand at top level or inside a nested
 * struct, several in one record; a list inside a list item is MK_EINVAL.
 * Limits: at most 256 chunks per list field (cap <= 256 * 128 / out_len); the
 * depth and entry limits above; and per record, along any one nesting path,
 * the messages (each rounded up to 4), a list's 256-byte chunk pair, 32 bytes
 * per level of its node stack (0 for a list of one chunk, else the bit length
 * of ceil(chunks / 2): at most 8) and behind them a struct item's messages may
 * sum to at most 640 bytes -- these layouts run 64 or 128 threads per
 * workgroup.  Device entry points clamp count to cap and never read outside
 * the slot; the host-buffer and handle entry points return MK_EINVAL,
 * changing nothing, for a count above cap (or a stored length above its slot
 * inside one of the first count items).
 *
 * mk_ssz_struct_msg_len: the top-level struct's message length; for a layout
 * with MK_FIELD_STRUCT entries the scratch bytes per record instead, the
 * message lengths of the top-level struct and of every nested struct summed.
 * 0 for a layout that is refused. */
#define MK_FIELD_BYTES 1
#define MK_FIELD_RAW 2
#define MK_FIELD_VARBYTES 3
#define MK_FIELD_STRUCT 4
#define MK_FIELD_LIST 5
typedef struct mk_field {
    uint32_t kind;
    uint32_t offset;
    uint32_t len;
} mk_field;
uint64_t mk_ssz_struct_msg_len(const mk_field* fields, uint32_t nfields);
/* roots of n records -> n x 32 bytes (one struct hash per record). */
int mk_ssz_struct_roots(mk_call* call, const uint8_t* records, uint64_t n, uint32_t record_len,
                        const mk_field* fields, uint32_t nfields, uint8_t* roots);
/* Device-resident struct roots (makeStructHasher per element,
 * hash.go:141-159): n records -> d_roots (n x 32) on `stream`; d_ws of at
 * least n * mk_ssz_struct_msg_len bytes. */
int mk_dev_ssz_struct_roots(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                            const mk_field* fields, uint32_t nfields, void* d_roots, void* d_ws, uint64_t ws_bytes,
                            void* stream);
/* TreeHash of a list of such structs: merkleHash over the n struct roots. */
uint64_t mk_ssz_struct_list_workspace_bytes(uint64_t n, const mk_field* fields, uint32_t nfields);
int mk_dev_ssz_struct_list_root(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                                const mk_field* fields, uint32_t nfields, void* d_out32, void* d_ws,
                                uint64_t ws_bytes, void* stream);
int mk_ssz_struct_list_root(mk_call* call, const uint8_t* records, uint64_t n, uint32_t record_len,
                            const mk_field* fields, uint32_t nfields, uint8_t out[32]);
/* The list root's first tree level in the struct-roots launch: d_roots (n x
 * 32) and the level-1 nodes of merkleHash over them, d_nodes (ceil(n/8) x 32:
 * node j = Keccak of roots 8j..8j+7, the ragged last window as merkleHash
 * hashes it, hash.go:205-228).  Optionally (nvalues > 0) the same launch
 * also writes the level-1 nodes of merkleHash over a second list -- nvalues
 * items of value_len bytes (8, 16, 32, 64 or 128) at a 16-B aligned
 * d_values, more than one chunk: ceil(nvalues * value_len / 256) nodes to
 * d_value_nodes (the State's balances, BASELINE config 3).  Finish each with
 * mk_dev_ssz_merkle_finish_nodes(nodes, count, n) -- the split lets the two
 * trees' latency-bound levels run side by side.
 * mk_ssz_struct_list_level1_ok says whether the records qualify (the
 * ValidatorRecord layout at a 16-B aligned address, n >= 2^18); otherwise
 * mk_dev_ssz_struct_list_level1 returns MK_EINVAL. */
int mk_ssz_struct_list_level1_ok(const void* d_records, uint64_t n, uint32_t record_len, const mk_field* fields,
                                 uint32_t nfields);
int mk_dev_ssz_struct_list_level1(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                                  const mk_field* fields, uint32_t nfields, void* d_roots, void* d_nodes,
                                  const void* d_values, uint64_t nvalues, uint32_t value_len, void* d_value_nodes,
                                  void* stream);
/* A stream of states (the State{registry, balances} of BASELINE config 3,
 * hash.go:118-159, one TreeHash per state) with each state's trees folded
 * into the NEXT state's struct launch: mk_dev_ssz_struct_list_level1 plus,
 * in the same launch, levels 2..10 of the PREVIOUS state's registry tree from
 * its level-1 nodes d_prev_nodes (NULL for the first state) over every
 * complete 512-node subtree, into d_prev_levels, and levels 2..4 of its
 * second list's tree from d_prev_value_nodes over every complete 128-node
 * subtree, into d_prev_value_levels (NULL: none).  Buffer sizes from
 * mk_ssz_struct_pipe_levels_bytes(n, nvalues, value_len, which): which = 0
 * the registry's, 1 the second list's.  Then mk_dev_ssz_struct_pipe_top
 * finishes each of the previous state's trees (the ragged last subtree, the
 * levels above the slots and the length mix-in) as one field of a pair
 * block, on another stream, beside the next launch.  Takes what
 * mk_ssz_struct_pipe_ok accepts on the same stream (as
 * mk_ssz_struct_list_level1_ok, with exactly 4 groups of 1024 records per
 * workgroup: 3 x 2^18 < n <= 2^20 on 256 CUs; a second list of at most 128
 * windows per workgroup, e.g. n 8-B balances); MK_EINVAL otherwise.  The
 * previous state must have the same n and second-list shape. */
int mk_ssz_struct_pipe_ok(const void* d_records, uint64_t n, uint32_t record_len, const mk_field* fields,
                          uint32_t nfields, void* stream);
uint64_t mk_ssz_struct_pipe_levels_bytes(uint64_t n, uint64_t nvalues, uint32_t value_len, uint32_t which);
uint64_t mk_ssz_struct_pipe_top_workspace_bytes(uint64_t n, uint64_t nvalues, uint32_t value_len, uint32_t which);
int mk_dev_ssz_struct_list_level1_pipe(mk_call* call, const void* d_records, uint64_t n, uint32_t record_len,
                                       const mk_field* fields, uint32_t nfields, void* d_roots, void* d_nodes,
                                       const void* d_values, uint64_t nvalues, uint32_t value_len,
                                       void* d_value_nodes, const void* d_prev_nodes, void* d_prev_levels,
                                       const void* d_prev_value_nodes, void* d_prev_value_levels, void* stream);
/* One tree's root of a state whose slot levels a later pipelined launch
 * built (d_nodes: its level-1 nodes, d_levels: those levels; which = 0 the
 * registry of n records, 1 the second list of nvalues items of value_len
 * bytes), as one field of a pair block (mk_dev_ssz_merkle_finish_nodes_pair
 * semantics: slot, epoch, the second finisher hashes the struct root). */
int mk_dev_ssz_struct_pipe_top(mk_call* call, const void* d_nodes, uint64_t n, uint64_t nvalues,
                               uint32_t value_len, uint32_t which, void* d_levels, void* d_pair_block, uint32_t slot,
                               uint32_t epoch, void* d_ws, uint64_t ws_bytes, void* stream);

/* ---- device-resident registry tree: a struct list re-hashed from changed records --- */
/* TreeHash of a list of n flat records (mk_field layouts, see the struct
 * hashing section above) with the records, their 32-B struct roots and every
 * level of merkleHash over those roots kept in HBM: a changed or appended
 * record costs its own struct hash and its ancestors instead of the whole
 * registry, and one call owns records and roots, so they cannot drift apart.
 * d_roots holds capacity x 32 B (16-B aligned) and is level 0 of a list tree
 * of 32-B items: d_levels has exactly the layout and size of
 * mk_ssz_list_tree_levels_bytes(capacity, 32) above (4 roots per chunk, a
 * level-1 node covers 8 records); there is no second layout.  d_records is
 * 4-byte aligned, capacity x record_len bytes.
 * Every layout mk_dev_ssz_struct_roots accepts is taken.  An update gathers
 * the dirty records, hashes them with the struct-roots kernels, scatters the
 * roots into d_roots and climbs with the list tree's update kernel.
 * Replaces: ssz.TreeHash of a []struct (makeSliceHasher, makeStructHasher and
 * merkleHash, shared/ssz/hash.go:118-159, 194-239) for a list whose tree is
 * already built. */
uint64_t mk_ssz_struct_list_tree_build_workspace_bytes(uint64_t n, const mk_field* fields, uint32_t nfields);
/* Every struct root (into d_roots), every level and the root of n <= capacity
 * records.  A bad field spec is MK_EINVAL as in mk_dev_ssz_struct_roots. */
int mk_dev_ssz_struct_list_tree_build(mk_call* call, const void* d_records, uint64_t n, uint64_t capacity,
                                      uint32_t record_len, const mk_field* fields, uint32_t nfields, void* d_roots,
                                      void* d_levels, void* d_root32, void* d_ws, uint64_t ws_bytes, void* stream);
/* Re-hash after a change, with the argument rules of
 * mk_dev_ssz_list_tree_update: d_idx holds k_idx strictly ascending record
 * indices < n_old (device memory), records [n_old, n_new) are appended.
 * d_values != NULL (4-byte aligned): k_idx new records, then the appended
 * ones, record_len bytes each, scattered into d_records first by the same
 * call; NULL: the caller has already written them into d_records on this
 * stream.  Recomputes the struct roots of exactly those records and their
 * ancestors and writes the root to d_root32 (also when nothing changed; with
 * n_new <= 4 the root is the mix-in over the raw chunk of roots).  An index >=
 * n_old is ignored.  Workspace (8-B aligned) from
 * mk_ssz_struct_list_tree_update_workspace_bytes(k, ..), k = k_idx + n_new -
 * n_old (< 2^31): the call zeroes and owns it until it has run, so trees
 * updated concurrently on different streams need a workspace each; too small
 * is MK_ENOMEM.  n_new < n_old and n_new > capacity are MK_EINVAL.  Allocates
 * nothing and can be captured into a hipGraph. */
uint64_t mk_ssz_struct_list_tree_update_workspace_bytes(uint64_t k, const mk_field* fields, uint32_t nfields);
int mk_dev_ssz_struct_list_tree_update(mk_call* call, void* d_records, uint64_t n_old, uint64_t n_new,
                                       uint64_t capacity, uint32_t record_len, const mk_field* fields,
                                       uint32_t nfields, void* d_roots, void* d_levels, const uint64_t* d_idx,
                                       uint64_t k_idx, const void* d_values, void* d_root32, void* d_ws,
                                       uint64_t ws_bytes, void* stream);
/* Shrink on the device, mk_dev_ssz_list_tree_erase's contract
 * with records for items: the records AND their 32-B struct roots in d_roots
 * move, no record is hashed again; k_rm == 0 with n_new <= n_old is the
 * truncate.  Workspace from mk_ssz_struct_list_tree_erase_workspace_bytes(
 * moved, record_len), moved = n_new - first (0 for a truncate).  Besides the
 * list tree's checks a bad field layout is MK_EINVAL; all of them come before
 * any device lookup.  Allocates nothing and can be captured into a hipGraph. */
uint64_t mk_ssz_struct_list_tree_erase_workspace_bytes(uint64_t moved, uint32_t record_len);
int mk_dev_ssz_struct_list_tree_erase(mk_call* call, void* d_records, uint64_t n_old, uint64_t n_new,
                                      uint64_t capacity, uint32_t record_len, const mk_field* fields,
                                      uint32_t nfields, void* d_roots, void* d_levels, const uint64_t* d_rm,
                                      uint64_t k_rm, uint64_t first, void* d_root32, void* d_ws, uint64_t ws_bytes,
                                      void* stream);
/* Handle form for host callers (the validator registry): records, roots and
 * levels stay in HBM under a per-handle lock, with mk_list_tree's semantics.
 * update takes host indices in any order (list[idx[j]] = records[j] in
 * sequence: of a repeated index the last value wins; an index >= count is
 * MK_EINVAL and nothing changes) and uploads only the k indices and records;
 * append past the capacity doubles it and rebuilds; a call that dirties a
 * 1/32 of the list or more rebuilds instead of climbing.  The
 * root of a new handle is merkleHash([]). */
typedef struct mk_struct_list_tree mk_struct_list_tree;
int mk_struct_list_tree_new(mk_call* call, uint32_t record_len, const mk_field* fields, uint32_t nfields,
                            uint64_t capacity, mk_struct_list_tree** out);
void mk_struct_list_tree_free(mk_struct_list_tree* t);
uint64_t mk_struct_list_tree_count(const mk_struct_list_tree* t);
/* Replaces the whole list by n records. */
int mk_struct_list_tree_assign(mk_call* call, mk_struct_list_tree* t, const uint8_t* records, uint64_t n);
int mk_struct_list_tree_update(mk_call* call, mk_struct_list_tree* t, const uint64_t* idx, const uint8_t* records,
                               uint64_t k);
int mk_struct_list_tree_append(mk_call* call, mk_struct_list_tree* t, const uint8_t* records, uint64_t k);
/* mk_list_tree_truncate / _erase for records (CleanupAttestations' stable filter). */
int mk_struct_list_tree_truncate(mk_call* call, mk_struct_list_tree* t, uint64_t n);
int mk_struct_list_tree_erase(mk_call* call, mk_struct_list_tree* t, const uint64_t* idx, uint64_t k);
int mk_struct_list_tree_root(mk_call* call, mk_struct_list_tree* t, uint8_t root[32]);
/* Records [first, first + cnt), cnt x record_len bytes. */
int mk_struct_list_tree_records(mk_call* call, mk_struct_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out);
/* mk_list_tree_branches over the 32-B struct roots: values_out gets k x 32 bytes (the proven leaves). */
int mk_struct_list_tree_branches(mk_call* call, mk_struct_list_tree* t, const uint64_t* idx, uint64_t k,
                                 uint8_t* values_out, uint8_t* branches_out);

/* ---- device-resident bytes tree: a [][N]byte list re-hashed from changed elements --- */
/* TreeHash of a list of n byte strings of elem_len bytes each (1 .. 2^30; the
 * list mk_dev_ssz_tree_hash_bytes_list hashes in one shot) with the elements,
 * their 32-B digests K(le32(elem_len) || e_i) and every level of merkleHash
 * over those digests kept in HBM: a changed or appended element costs its own
 * digest and the ancestors of its chunk instead of the whole list, and one
 * call owns elements and digests, so they cannot drift apart.
 * d_digests holds capacity x 32 B (16-B aligned) and is level 0 of a list tree
 * of 32-B items: d_levels has exactly the layout and size of
 * mk_ssz_list_tree_levels_bytes(capacity, 32) above (4 digests per chunk, a
 * level-1 node covers 8 elements); there is no second layout.  d_elems is
 * capacity x elem_len bytes, flat, at any byte alignment (32-B elements at a
 * 16-B aligned base take the one-permutation digest).  elem_len == 0 is
 * MK_EINVAL here (the one-shot entry keeps accepting it); a list whose
 * elements differ in length is not covered.
 * Replaces: ssz.TreeHash of a [][N]byte (makeSliceHasher, hashedEncoding and
 * merkleHash, shared/ssz/hash.go:100-107, 118-139, 194-239) for a list whose
 * tree is already built. */
uint64_t mk_ssz_bytes_list_tree_build_workspace_bytes(uint64_t n, uint32_t elem_len);
/* Every element digest (into d_digests), every level and the root of
 * n <= capacity elements. */
int mk_dev_ssz_bytes_list_tree_build(mk_call* call, const void* d_elems, uint64_t n, uint64_t capacity,
                                     uint32_t elem_len, void* d_digests, void* d_levels, void* d_root32, void* d_ws,
                                     uint64_t ws_bytes, void* stream);
/* Re-hash after a change, with the argument rules of
 * mk_dev_ssz_struct_list_tree_update: d_idx holds k_idx strictly ascending
 * element indices < n_old (device memory), elements [n_old, n_new) are
 * appended.  d_values != NULL: k_idx new elements, then the appended ones,
 * elem_len bytes each, scattered into d_elems first by the same call; NULL:
 * the caller has already written them into d_elems on this stream.
 * Recomputes the digests of exactly those elements (read in place, no
 * gathered copy) and their ancestors and writes the root to d_root32 (also
 * when nothing changed; with n_new <= 4 the root is the mix-in over the raw
 * chunk of digests).  An index >= n_old is ignored.  Workspace (8-B aligned)
 * from mk_ssz_bytes_list_tree_update_workspace_bytes(k, elem_len), k = k_idx +
 * n_new - n_old (< 2^31): the call zeroes and owns it until it has run, so
 * trees updated concurrently on different streams need a workspace each; too
 * small is MK_ENOMEM.  n_new < n_old, n_new > capacity and elem_len == 0 are
 * MK_EINVAL; these checks come before any device lookup.  Allocates nothing
 * and can be captured into a hipGraph. */
uint64_t mk_ssz_bytes_list_tree_update_workspace_bytes(uint64_t k, uint32_t elem_len);
int mk_dev_ssz_bytes_list_tree_update(mk_call* call, void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                      uint32_t elem_len, void* d_digests, void* d_levels, const uint64_t* d_idx,
                                      uint64_t k_idx, const void* d_values, void* d_root32, void* d_ws,
                                      uint64_t ws_bytes, void* stream);
/* Shrink on the device, mk_dev_ssz_list_tree_erase's contract
 * with elements for items: the elements AND their digests in d_digests move,
 * no element is digested again; k_rm == 0 with n_new <= n_old is the truncate.
 * Workspace from mk_ssz_bytes_list_tree_erase_workspace_bytes(moved, elem_len),
 * moved = n_new - first (0 for a truncate).  Every check comes before any
 * device lookup.  Allocates nothing and can be captured into a hipGraph. */
uint64_t mk_ssz_bytes_list_tree_erase_workspace_bytes(uint64_t moved, uint32_t elem_len);
int mk_dev_ssz_bytes_list_tree_erase(mk_call* call, void* d_elems, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                                     uint32_t elem_len, void* d_digests, void* d_levels, const uint64_t* d_rm,
                                     uint64_t k_rm, uint64_t first, void* d_root32, void* d_ws, uint64_t ws_bytes,
                                     void* stream);
/* Handle form for host callers (the state's root arrays): elements, digests
 * and levels stay in HBM under a per-handle lock, with mk_struct_list_tree's
 * semantics.  update takes host indices in any order (list[idx[j]] = elems[j]
 * in sequence: of a repeated index the last value wins; an index >= count is
 * MK_EINVAL and nothing changes) and uploads only the k indices and elements;
 * append past the capacity doubles it and rebuilds; a call that dirties a
 * 1/256 of the list or more rebuilds instead of climbing.  The
 * root of a new handle is merkleHash([]). */
typedef struct mk_bytes_list_tree mk_bytes_list_tree;
int mk_bytes_list_tree_new(mk_call* call, uint32_t elem_len, uint64_t capacity, mk_bytes_list_tree** out);
void mk_bytes_list_tree_free(mk_bytes_list_tree* t);
uint64_t mk_bytes_list_tree_count(const mk_bytes_list_tree* t);
/* Replaces the whole list by n elements. */
int mk_bytes_list_tree_assign(mk_call* call, mk_bytes_list_tree* t, const uint8_t* elems, uint64_t n);
int mk_bytes_list_tree_update(mk_call* call, mk_bytes_list_tree* t, const uint64_t* idx, const uint8_t* elems,
                              uint64_t k);
int mk_bytes_list_tree_append(mk_call* call, mk_bytes_list_tree* t, const uint8_t* elems, uint64_t k);
/* mk_list_tree_truncate / _erase for elements. */
int mk_bytes_list_tree_truncate(mk_call* call, mk_bytes_list_tree* t, uint64_t n);
int mk_bytes_list_tree_erase(mk_call* call, mk_bytes_list_tree* t, const uint64_t* idx, uint64_t k);
int mk_bytes_list_tree_root(mk_call* call, mk_bytes_list_tree* t, uint8_t root[32]);
/* Elements [first, first + cnt), cnt x elem_len bytes. */
int mk_bytes_list_tree_elems(mk_call* call, mk_bytes_list_tree* t, uint64_t first, uint64_t cnt, uint8_t* out);
/* mk_list_tree_branches over the 32-B element digests K(le32(N) || e_i): values_out gets k x 32 bytes. */
int mk_bytes_list_tree_branches(mk_call* call, mk_bytes_list_tree* t, const uint64_t* idx, uint64_t k,
                                uint8_t* values_out, uint8_t* branches_out);

/* ---- several device-resident trees, and the struct that holds them, in one call --- */
/* mk_dev_ssz_trees_update runs the update of up to MK_TREES_MAX resident trees
 * of any of the three kinds above in one call: every tree's stage 0 (its
 * values scattered in, its struct roots or element digests), then ONE launch
 * in which all the trees climb side by side, about as long as the deepest of
 * them.  For every tree the result in d_items, d_level0, d_levels and d_root32
 * is byte for byte what that kind's own mk_dev_ssz_*_tree_update leaves with
 * the same arguments (an index >= n_old ignored, appends, nothing changed,
 * lists of at most one chunk), and each kind's own argument rules hold.
 * `trees` is host memory, read only during the call.
 * Container: a struct whose list fields are these trees (makeStructHasher,
 * hash.go:141-159).  d_container (4-B aligned, container_len = 1 ..
 * MK_CONTAINER_MAX bytes) is the struct's hash message with every other
 * field's output already written by the caller on this stream; tree i's root
 * is also stored at container_off[i] (4-B aligned, the 32-B ranges disjoint
 * and inside the message; MK_NO_CONTAINER: the tree is no field of it), and
 * the last tree to finish hashes the message into d_container_root32 (4-B
 * aligned) in the same launch.  container_len == 0: no container, d_container
 * and d_container_root32 may be NULL and are not touched.
 * Workspace (16-B aligned) from mk_ssz_trees_update_workspace_bytes (the sum of
 * the per-kind update workspaces plus the container's counter; 0 for a tree
 * list the call would refuse): the call zeroes its arrival words and owns it
 * until it has run, so calls on different streams need a workspace each.
 * MK_EINVAL: ntrees 0 or > MK_TREES_MAX, an unknown kind, a d_level0 that does
 * not match the kind, container_len > MK_CONTAINER_MAX, a misaligned,
 * overflowing or overlapping container_off, a container no tree takes part in,
 * and each kind's own (item_len == 0, n_new < n_old, n_new > capacity, a bad
 * field layout, 2^31 work items); MK_ENOMEM: a short workspace.  Every check
 * comes before any device lookup, and on an error nothing is launched.
 * Uploads nothing, allocates nothing, never synchronises, and can be captured
 * into a hipGraph (a linear chain of nodes).
 * Replaces: ssz.TreeHash (shared/ssz/hash.go:23-239) of a struct whose slice
 * fields are lists with built trees -- a pb.BeaconState -- after some of their
 * elements changed. */
#define MK_TREE_LIST   1   /* mk_dev_ssz_list_tree_update's tree        */
#define MK_TREE_STRUCT 2   /* mk_dev_ssz_struct_list_tree_update's tree */
#define MK_TREE_BYTES  3   /* mk_dev_ssz_bytes_list_tree_update's tree  */
#define MK_TREES_MAX   16
#define MK_NO_CONTAINER 0xffffffffu
#define MK_CONTAINER_MAX 4096

typedef struct mk_tree_update {
    uint32_t kind;
    uint32_t item_len;        /* item_len / record_len / elem_len */
    void* d_items;            /* items / records / elements */
    void* d_level0;           /* STRUCT: d_roots, BYTES: d_digests, LIST: NULL */
    void* d_levels;
    uint64_t n_old, n_new, capacity;
    const uint64_t* d_idx;    /* k_idx strictly ascending indices < n_old, device */
    uint64_t k_idx;
    const void* d_values;     /* NULL: already written into d_items on this stream */
    const mk_field* fields;   /* STRUCT only (host) */
    uint32_t nfields;
    uint32_t container_off;   /* byte offset of this tree's root in d_container, or MK_NO_CONTAINER */
    void* d_root32;           /* this tree's root, always written */
} mk_tree_update;

uint64_t mk_ssz_trees_update_workspace_bytes(const mk_tree_update* trees, uint32_t ntrees);
int mk_dev_ssz_trees_update(mk_call* call, const mk_tree_update* trees, uint32_t ntrees, void* d_container,
                            uint32_t container_len, void* d_container_root32, void* d_ws, uint64_t ws_bytes,
                            void* stream);

/* ---- a set of device-resident trees behind one host handle ---------------- */
/* mk_tree_set is the handle form of mk_dev_ssz_trees_update for host callers
 * (cgo has no device pointers): it owns up to MK_TREES_MAX resident trees of
 * the three kinds and, in HBM, the hash message (container_len = 0 ..
 * MK_CONTAINER_MAX bytes; 0: no container) of the struct whose list fields
 * they are.  Changes are collected on the host; a root is ONE upload of every
 * tree's changes and the message, mk_dev_ssz_trees_update over all the trees,
 * one 32-B read-back and one synchronise.  Every rule below is what
 * mk_list_tree / mk_struct_list_tree / mk_bytes_list_tree promise of one tree.
 * new: needs no device; the set lives on call->device (-1: the device current
 *   when the first tree is added) and every call runs there and restores the
 *   caller's device, free included.
 * add: at any time.  kind = MK_TREE_LIST / STRUCT / BYTES, item_len = item /
 *   record / element length, fields / nfields the record layout (STRUCT only,
 *   copied), container_off the offset of the tree's root in the message or
 *   MK_NO_CONTAINER.  The new tree is empty, its root merkleHash([]); *tree =
 *   0, 1, ... is its number.  MK_EINVAL, before any device is needed: a 17th
 *   tree, an unknown kind, fields missing (STRUCT) or given (LIST, BYTES), the
 *   kind's own shape errors (item_len == 0, a bad layout, capacity * item_len
 *   overflowing), a container_off that is not 4-B aligned, leaves the message
 *   or overlaps another tree's 32 bytes.
 * put: the other fields' outputs into the message; a range that leaves the
 *   message or touches a tree's 32-B root range is MK_EINVAL and nothing is
 *   written.  No device call.
 * update: list[idx[j]] = values[j] in sequence (any order; of a repeated index
 *   the last value wins); an index >= count (pending appends included) is
 *   MK_EINVAL and nothing changes; an index inside the pending appends changes
 *   that pending value.  append: values behind the list.  A STRUCT tree's
 *   records pass the VARBYTES length check here, not at the flush.  Both only
 *   record the change: no device call, no synchronise; the caller's buffers
 *   are copied and free on return.
 * assign: replaces the list (a shorter one too), drops the tree's pending
 *   changes, and goes through the build entry at once.
 * root / tree_root / items flush first: every tree's ascending, de-duplicated
 *   indices and values, then its appended values, in one pinned staging buffer
 *   (indices at 8-B, values at 16-B boundaries) sent by one copy; a tree that
 *   outgrew its capacity doubles it, moves its items and rebuilds; a tree whose
 *   dirty share reaches its kind's (count / 512, / 32, / 256 <= dirty: DESIGN.md
 *   §5d-§5f) takes the write-through and the build; both enter the update with
 *   nothing dirty, so their roots still reach the message.  With nothing
 *   changed the same root comes back.  A failed flush leaves the pending
 *   changes in place: the next call tries again, or the caller frees the set.
 * root: the hash of the message (K(message), every tree's root at its offset);
 *   MK_EINVAL when container_len == 0 or no tree takes part in the container.
 *   tree_root: one tree's root, always.  items: [first, first + cnt) of one
 *   tree, cnt x item_len bytes.  count: its length, pending appends included.
 * One mutex per set: any thread may call, two sets are independent.
 * Replaces: ssz.TreeHash (shared/ssz/hash.go:23-239) of a long-lived struct of
 * lists -- a pb.BeaconState -- between two slots. */
typedef struct mk_tree_set mk_tree_set;
int mk_tree_set_new(mk_call* call, uint32_t container_len, mk_tree_set** out);
void mk_tree_set_free(mk_tree_set* s);
int mk_tree_set_add(mk_call* call, mk_tree_set* s, uint32_t kind, uint32_t item_len, const mk_field* fields,
                    uint32_t nfields, uint64_t capacity, uint32_t container_off, uint32_t* tree);
int mk_tree_set_put(mk_call* call, mk_tree_set* s, uint32_t off, const uint8_t* bytes, uint32_t len);
int mk_tree_set_assign(mk_call* call, mk_tree_set* s, uint32_t tree, const uint8_t* values, uint64_t n);
int mk_tree_set_update(mk_call* call, mk_tree_set* s, uint32_t tree, const uint64_t* idx, const uint8_t* values,
                       uint64_t k);
int mk_tree_set_append(mk_call* call, mk_tree_set* s, uint32_t tree, const uint8_t* values, uint64_t k);
/* Shrink one tree of the set, mk_list_tree_truncate / _erase
 * against count(tree), pending appends included.  A shrink is not recorded:
 * it first flushes whatever the set has pending, then shrinks that tree on
 * the device at once; the next root carries its new root.  A failed shrink
 * leaves the set as the flush left it; a bad argument changes nothing. */
int mk_tree_set_truncate(mk_call* call, mk_tree_set* s, uint32_t tree, uint64_t n);
int mk_tree_set_erase(mk_call* call, mk_tree_set* s, uint32_t tree, const uint64_t* idx, uint64_t k);
uint64_t mk_tree_set_count(const mk_tree_set* s, uint32_t tree);
int mk_tree_set_root(mk_call* call, mk_tree_set* s, uint8_t root[32]);
int mk_tree_set_tree_root(mk_call* call, mk_tree_set* s, uint32_t tree, uint8_t root[32]);
int mk_tree_set_items(mk_call* call, mk_tree_set* s, uint32_t tree, uint64_t first, uint64_t cnt, uint8_t* out);
/* Proofs out of one tree of the set (mk_list_tree_branches against
 * count(tree), pending appends included): flushes whatever is pending, as a
 * root does, then runs the tree's launch.  container_out (may be NULL;
 * container_len bytes, nothing for a set without a container) gets the hash
 * message with every tree's root in place: mk_verify_list_branches takes it
 * with the tree's container offset and compares with mk_tree_set_root. */
int mk_tree_set_branches(mk_call* call, mk_tree_set* s, uint32_t tree, const uint64_t* idx, uint64_t k,
                         uint8_t* values_out, uint8_t* branches_out, uint8_t* container_out);

/* ---- resident trees copied on the device: clone, copy, reserve --- */
/* A second resident state (the candidate post-state of a block, the other side
 * of a fork) and a tree moved to a larger capacity are one operation: the live
 * part of a tree moves from the layout of one capacity into the layout of
 * another and nothing is hashed.  The live part is the n values (n x item_len
 * bytes), level 0 of a STRUCT / BYTES tree (32 n bytes), the ceil(nchunks /
 * 2^d) nodes of every stored level d = 1 .. D -- from node sum_{1<=i<d}
 * ceil(cap_chunks / 2^i) of the source's level array to the same sum for the
 * destination's capacity -- and the 32-byte root.  Levels above D and nodes
 * beyond a level's count are unspecified in both layouts: they are not read
 * and not written, so the destination is a valid tree of n values of capacity
 * dst_capacity whatever its buffers held before, and what a shrink left to the
 * right of the source's end does not travel.
 * mk_dev_ssz_trees_copy copies up to MK_TREES_MAX trees and one optional 32-byte
 * extra (a set's container root; both pointers NULL: none) in ONE launch.
 * `trees` is host memory, read only during the call: the descriptors travel as
 * kernel arguments.  Uploads nothing, allocates nothing, needs no workspace,
 * never synchronises and can be captured into a hipGraph.  d_*_items at any
 * byte alignment (a 16-B aligned pair moves in 16-B pieces); d_*_level0 (NULL
 * for MK_TREE_LIST), d_*_levels, d_*_root32 and the extra 16-B aligned.
 * MK_EINVAL, every check before a device is looked up and nothing launched:
 * ntrees > MK_TREES_MAX, an unknown kind, item_len == 0 or above 2^30, n above
 * either capacity, capacity * item_len overflowing, a null pointer where the
 * shape needs one (values and level 0 for n > 0, levels for D >= 1, the roots
 * always), a level 0 given for a list tree, a misaligned level 0, level array,
 * root or extra, an extra with one side NULL, and a source range that overlaps
 * a destination range of the same call (a tree's levels count from the first
 * stored node to the top).  ntrees == 0 without an extra is MK_OK and launches
 * nothing.  Source and destination lie on the stream's device. */
typedef struct mk_tree_copy {
    uint32_t kind, item_len;          /* MK_TREE_LIST / _STRUCT / _BYTES; item / record / element length */
    uint64_t n, src_capacity, dst_capacity;
    const void *d_src_items, *d_src_level0, *d_src_levels, *d_src_root32;
    void *d_dst_items, *d_dst_level0, *d_dst_levels, *d_dst_root32;
} mk_tree_copy;
int mk_dev_ssz_trees_copy(mk_call* call, const mk_tree_copy* trees, uint32_t ntrees, const void* d_src_extra32,
                          void* d_dst_extra32, void* stream);
/* Handle forms, the same for the three kinds.
 * clone: a new handle of the source's kind, item length, record layout, device
 *   and capacity holding the source's list: one copy launch, nothing uploaded,
 *   nothing hashed.  The two handles share nothing afterwards.
 * copy: dst becomes a copy of src.  dst must be of the same kind, item length
 *   and record layout and on the same device, else MK_EINVAL and nothing
 *   changes.  dst keeps its capacity when src's count fits; otherwise it gets
 *   buffers of src's capacity, allocated before anything is enqueued, so a
 *   failed allocation leaves dst as it was.  dst == src is MK_OK and does nothing.
 * reserve: room for `capacity` values; capacity <= the current one is a no-op.
 *   Allocates the new buffers, moves the tree into the new layout by one copy
 *   launch and frees the old ones: root, count and values are unchanged and
 *   nothing is hashed (an append past the capacity still doubles and rebuilds).
 * capacity: the values the handle has room for (0 for NULL). */
int mk_list_tree_clone(mk_call* call, mk_list_tree* src, mk_list_tree** out);
int mk_list_tree_copy(mk_call* call, mk_list_tree* dst, mk_list_tree* src);
int mk_list_tree_reserve(mk_call* call, mk_list_tree* t, uint64_t capacity);
uint64_t mk_list_tree_capacity(const mk_list_tree* t);
int mk_struct_list_tree_clone(mk_call* call, mk_struct_list_tree* src, mk_struct_list_tree** out);
int mk_struct_list_tree_copy(mk_call* call, mk_struct_list_tree* dst, mk_struct_list_tree* src);
int mk_struct_list_tree_reserve(mk_call* call, mk_struct_list_tree* t, uint64_t capacity);
uint64_t mk_struct_list_tree_capacity(const mk_struct_list_tree* t);
int mk_bytes_list_tree_clone(mk_call* call, mk_bytes_list_tree* src, mk_bytes_list_tree** out);
int mk_bytes_list_tree_copy(mk_call* call, mk_bytes_list_tree* dst, mk_bytes_list_tree* src);
int mk_bytes_list_tree_reserve(mk_call* call, mk_bytes_list_tree* t, uint64_t capacity);
uint64_t mk_bytes_list_tree_capacity(const mk_bytes_list_tree* t);
/* The same for a set.  clone / copy flush the source first, as root does, so
 * the copy holds what root() would describe; then ONE copy launch moves every
 * tree and the container root, and the hash message is copied on the host.
 * The destination's pending changes are dropped and it is not dirty afterwards.
 * copy: the sets must agree in container length, device and, tree by tree, in
 * kind, item length, record layout and container offset, else MK_EINVAL and
 * nothing changes; every destination tree that is too small gets its new
 * buffers before anything is enqueued; dst == src is MK_OK and does nothing.
 * reserve / capacity: mk_*_tree_reserve / _capacity of one tree of the set
 * (pending changes stay pending; capacity is 0 for a tree the set has not). */
int mk_tree_set_clone(mk_call* call, mk_tree_set* src, mk_tree_set** out);
int mk_tree_set_copy(mk_call* call, mk_tree_set* dst, mk_tree_set* src);
int mk_tree_set_reserve(mk_call* call, mk_tree_set* s, uint32_t tree, uint64_t capacity);
uint64_t mk_tree_set_capacity(const mk_tree_set* s, uint32_t tree);

/* ---- resident trees: an update taken back through an undo journal --- */
/* An update overwrites the changed values, their level-0 entries and their
 * ancestors: about changed x depth nodes.  mk_dev_ssz_trees_journal saves
 * exactly those before the update runs, mk_dev_ssz_trees_restore writes them
 * back: an update is undone without a hash and without a second copy of the
 * state.
 * journal takes the very array mk_dev_ssz_trees_update is about to get (the
 * same kinds, d_idx / k_idx, n_old / n_new) and is enqueued BEFORE that update
 * on the same stream -- and, for a tree with d_values == NULL, before the
 * caller writes the new bytes.  ONE launch (k_trees_journal) saves into
 * d_journal, per tree: the work items -- the k_idx listed indices and, when
 * n_new > n_old > 0, one more for the last old value, on whose ancestors every
 * stored ancestor of an appended chunk lies -- each as 8 bytes of index, the
 * old value, its 32-B level-0 entry (STRUCT / BYTES) and node (chunk >> d) of
 * every level d = 1 .. D of the old tree (the layout rule: the resident list
 * tree above); then the tree's 32-B root.  Per call: the container message and
 * the container root.  A slot per (work item, level) at a fixed position: two
 * work items under one node both save it, nothing is compacted, the launch has
 * no atomics and waits for nothing.  A listed index >= n_old stands for the
 * last old value (the update ignores it; either way the journal is right); a
 * tree with n_old == 0 saves its root only.  No byte of a value buffer or a
 * level 0 at or beyond n_old values is part of the old state -- the three
 * kinds' kernels read a level-1 window, a raw chunk and every record or
 * element only below the count they are given -- so none is saved, and what an
 * update appended stays behind the restored end, unspecified as after a shrink.
 * restore takes the same array; the index LISTS (d_idx) and d_values are not
 * read -- they may be NULL or reused -- because the indices come from the
 * journal; kind, item_len, the buffers, capacity, k_idx, n_old and n_new must
 * be what journal got, and n_old is the count to return to.  ONE launch
 * (k_trees_restore) scatters every saved piece back; duplicates carry equal
 * bytes.  Afterwards every byte the layout contract specifies for n_old values
 * is what it was when journal ran: values [0, n_old), level 0, the nodes
 * within the old counts on levels up to the old top, the root, the message and
 * the container root.  Nodes and levels beyond that stay unspecified.  Several
 * records are undone newest first, in stream order.
 * d_journal is 16-B aligned, mk_ssz_trees_journal_bytes long (0 for an array
 * the calls would refuse) and nothing beyond that is written; it depends on
 * the counts, k_idx, item_len and container_len only.  Every argument is
 * checked before a device is looked up, by the rules of
 * mk_dev_ssz_trees_update; a null or misaligned journal is MK_EINVAL, a short
 * one MK_ENOMEM.  Both upload nothing, allocate nothing, never synchronise and
 * can be captured into a hipGraph. */
uint64_t mk_ssz_trees_journal_bytes(const mk_tree_update* trees, uint32_t ntrees, uint32_t container_len);
int mk_dev_ssz_trees_journal(mk_call* call, const mk_tree_update* trees, uint32_t ntrees, const void* d_container,
                             uint32_t container_len, const void* d_container_root32, void* d_journal,
                             uint64_t journal_bytes, void* stream);
int mk_dev_ssz_trees_restore(mk_call* call, const mk_tree_update* trees, uint32_t ntrees, void* d_container,
                             uint32_t container_len, void* d_container_root32, const void* d_journal,
                             uint64_t journal_bytes, void* stream);
/* Checkpoints of a set: apply a block, verify the state root,
 * keep it or roll it back; keep the last slots undoable for about their change
 * volume instead of a clone each.
 * checkpoint: flushes what is pending (journaled only if a checkpoint is open
 *   already), opens a checkpoint and returns its id; ids only grow.  With
 *   MK_CHECKPOINTS_MAX open it is MK_EINVAL and nothing changes.
 * While a checkpoint is open every flush is one record: the flush enqueues
 *   mk_dev_ssz_trees_journal between its upload and its update, into a journal
 *   the set owns (it grows by doubling; journal_reserve gives it room ahead of
 *   a slot), and keeps the per-tree n_old, n_new, k_idx and the offset on the
 *   host.  A change that does not climb -- assign, a flush that rebuilds a tree
 *   at its kind's dirty share or grows it past its capacity, truncate, erase --
 *   writes a full record of that tree instead: its live part copied by the copy
 *   launch (mk_dev_ssz_trees_copy) into memory the journal owns, before the
 *   change.  A record counts only after the synchronise the flush already does:
 *   a failed flush can still be tried again.  add is MK_EINVAL while a
 *   checkpoint is open.
 * rollback(id): drops the pending changes, undoes every record made since
 *   checkpoint id newest first (journals restored, full records copied home),
 *   restores the counts and the message, closes id and every later checkpoint,
 *   and ends with one flush with nothing dirty that brings the trees' roots in
 *   the message and the message's root up to date (the journals of a set hold
 *   no container), under the call's synchronise; a full record's copy home
 *   synchronises too.  Capacity is not part of the state: a tree that grew
 *   stays grown.  An unknown or closed id is MK_EINVAL and nothing changes.
 * release(id): forgets checkpoint id and every earlier one and frees the
 *   records written before the first checkpoint that remains; with none
 *   remaining the journal is empty and flushes stop journaling.
 *   A device error (MK_EHIP) in the middle of a roll back leaves some records
 *   undone and the checkpoint open: the set's content is then undefined, and
 *   the caller frees it or assigns every tree.
 * journal_bytes: the bytes of HBM the open checkpoints hold (journals and full
 *   records).  journal_capacity: the bytes allocated for the journals; the
 *   front a release frees is taken back before the buffer is made larger, so
 *   a ring of checkpoints whose oldest is released every slot keeps it at
 *   about twice its live records.  journal_reserve(bytes): room for that many
 *   bytes of live journal.  clone / copy copy the state, not the journal; a copy INTO a set
 *   with open checkpoints is MK_EINVAL.  The calls run under the set's mutex.
 * mk_list_tree and its siblings have no checkpoints: they have no pending log;
 *   a set of one tree covers them. */
#define MK_CHECKPOINTS_MAX 64
int mk_tree_set_checkpoint(mk_call* call, mk_tree_set* s, uint64_t* id);
int mk_tree_set_rollback(mk_call* call, mk_tree_set* s, uint64_t id);
int mk_tree_set_release(mk_call* call, mk_tree_set* s, uint64_t id);
uint64_t mk_tree_set_journal_bytes(const mk_tree_set* s);
uint64_t mk_tree_set_journal_capacity(const mk_tree_set* s);
int mk_tree_set_journal_reserve(mk_call* call, mk_tree_set* s, uint64_t bytes);

/* ---- resident trees audited on the device ------------------------- */
/* Is a resident tree what its values say it is?  Every stored node is checked
 * against what is stored below it, read-only and in HBM.  len0 = item_len for
 * MK_TREE_LIST and 32 for MK_TREE_STRUCT / _BYTES; p, cb, nchunks, total and D
 * as for mk_ssz_list_branch_bytes over len0.  The checks:
 *   level 0 (STRUCT / BYTES), i < n: d_level0[32 i] against the struct hash of
 *     record i / against K(le32(elem_len) || element i);
 *   level 1, j < ceil(nchunks / 2): K(the level-0 bytes [2 j cb, min(total,
 *     (2 j + 2) cb)), then 0^128 when 2 j + 1 == nchunks) against the stored node;
 *   level d = 2 .. D, j < ceil(nchunks / 2^d): K(child 2j || child 2j+1), or
 *     K(child 2j || 0^128) when 2j+1 is at or beyond level d - 1's count;
 *   the root: K(top || le64(n) || 0^24) against d_root32, top node 0 of level D
 *     or, for nchunks <= 1, the raw chunk (0^128 for n == 0);
 *   the container (container_len > 0): K(message) against d_container_root32
 *     (index 0) and, for each tree i with a container_off, the message's 32
 *     bytes there against the tree's d_root32 (index 1 + i).
 * Every count comes from n; the capacity only places the levels.  No node at or
 * beyond a level's count and no level-0 byte at or beyond total is read.
 * A mismatch has the key (level, index): level 0, 1 .. D, MK_AUDIT_ROOT for the
 * root, MK_AUDIT_CONTAINER for the container checks.  A report holds the number
 * of mismatches and the smallest key in (level, index) order; with none,
 * first_level is MK_AUDIT_NONE and first_index is 2^64 - 1.  A wrong node is
 * reported where it is stored and again one level up, where it is a child.
 * mk_dev_ssz_trees_audit audits up to MK_TREES_MAX trees and the message: the
 * reports are cleared on the stream, level 0 of the STRUCT / BYTES trees goes
 * through the struct-roots / digest launches in pieces of at most 2^18 values
 * into the workspace with a compare launch behind each, ONE launch checks every
 * node of level >= 1, every root and the container, and a last one unpacks the
 * keys.  d_reports: ntrees + 1 reports (8-B aligned), tree i's at i, the
 * container's last (bad == 0 without a container).  Workspace (16-B aligned)
 * from mk_ssz_trees_audit_workspace_bytes: it does not grow with n beyond the
 * piece; 0 for list trees only (d_ws may then be NULL) and for a tree list the
 * call would refuse.  d_level0 (NULL for MK_TREE_LIST), d_levels and d_root32
 * 16-B aligned, records 4-B aligned, d_container and d_container_root32 4-B.
 * MK_EINVAL, every check before a device is looked up and nothing launched:
 * null or misaligned pointers where the shape needs them, an unknown kind,
 * item_len == 0, a LIST item_len above 128, n > capacity, capacity * item_len
 * overflowing, ntrees 0 or > MK_TREES_MAX, a level 0 or fields that do not match
 * the kind, a bad field layout, container_len > MK_CONTAINER_MAX, a
 * container_off that is misaligned, leaves the message, overlaps another or
 * comes without a message, 2^31 or more work items; MK_ENOMEM: a short
 * workspace.  Allocates nothing, uploads nothing, never synchronises, writes
 * nothing but d_reports and d_ws, and can be captured into a hipGraph (a linear
 * chain of nodes). */
#define MK_AUDIT_ROOT 64u
#define MK_AUDIT_CONTAINER 65u
#define MK_AUDIT_NONE 0xffffffffu
typedef struct mk_tree_audit {
    uint32_t kind, item_len;       /* MK_TREE_LIST / _STRUCT / _BYTES; item / record / element length */
    const void *d_items, *d_level0, *d_levels, *d_root32;
    uint64_t n, capacity;
    const mk_field* fields;        /* STRUCT only (host) */
    uint32_t nfields;
    uint32_t container_off;        /* byte offset of this tree's root in d_container, or MK_NO_CONTAINER */
} mk_tree_audit;
typedef struct mk_audit_report {
    uint64_t bad;                  /* mismatches */
    uint64_t first_index;          /* of the smallest key */
    uint32_t first_level;          /* MK_AUDIT_NONE: no mismatch */
    uint32_t pad;
} mk_audit_report;
uint64_t mk_ssz_trees_audit_workspace_bytes(const mk_tree_audit* trees, uint32_t ntrees);
int mk_dev_ssz_trees_audit(mk_call* call, const mk_tree_audit* trees, uint32_t ntrees, const void* d_container,
                           uint32_t container_len, const void* d_container_root32, void* d_reports, void* d_ws,
                           uint64_t ws_bytes, void* stream);
/* Handle forms: the audit of the handle's tree, one read-back of its report
 * (*out).  mk_tree_set_audit flushes what is pending, as root does, then audits
 * all the trees and the message in the same launch: out gets count + 1 reports,
 * the container's last; a set without trees is MK_EINVAL.  The deposit trie's
 * audit is mk_deposit_trie_audit, with the same report. */
int mk_list_tree_audit(mk_call* call, mk_list_tree* t, mk_audit_report* out);
int mk_struct_list_tree_audit(mk_call* call, mk_struct_list_tree* t, mk_audit_report* out);
int mk_bytes_list_tree_audit(mk_call* call, mk_bytes_list_tree* t, mk_audit_report* out);
int mk_tree_set_audit(mk_call* call, mk_tree_set* s, mk_audit_report* out);

/* ---- two resident trees diffed on the device ---------------------- */
/* Which values of two resident trees differ?  Two stored trees that agree at a
 * node agree on everything under it, so the differing values are found by
 * walking down only through nodes that differ: about (differences) x (depth)
 * node reads whatever n is.  len0 = item_len for MK_TREE_LIST and 32 for
 * MK_TREE_STRUCT / _BYTES, p = 128 / len0 leaves per chunk, nchunks_X =
 * ceil(n_X / p), D_X the smallest d with ceil(nchunks_X / 2^d) == 1; level d of
 * tree X starts at node sum_{1<=i<d} ceil(cap_chunks_X / 2^i) of its level
 * array, so every offset is taken per side.  With m = min(n_a, n_b):
 *   the result is the set of indices i < m whose leaf differs -- the item_len
 *     bytes of item i of a LIST tree, the 32-byte level-0 entry (struct root /
 *     element digest) of a STRUCT / BYTES tree, so record bytes outside the
 *     fields and the slack of a VARBYTES slot are no difference.  Indices at or
 *     above m are never listed: the caller has n_a and n_b;
 *   node (d, j) covers values [j 2^d p, (j + 1) 2^d p).  It is visited only when
 *     j 2^d p < m and is comparable when n_a == n_b or (j + 1) 2^d p <= m.  A
 *     comparable node whose 32 bytes are equal ends the descent; one that is
 *     not comparable (the straddler of its level when the counts differ) is
 *     never read and always descended -- with the 0^128 pad of an odd level,
 *     K(c || 0^128) is both "c was the last chunk" and "an all-zero chunk
 *     follows c", so a straddler may be equal in two trees of different length;
 *   no node at or beyond a level's count of its tree, no level above
 *     min(D_a, D_b) and no leaf byte at or beyond m len0 is read.
 * mk_dev_ssz_trees_diff diffs up to MK_TREES_MAX pairs: the reports are cleared
 * on the stream and ONE launch follows (none when no pair has a value below its
 * m).  Pair i's differing indices go to its d_idx_out in no particular order,
 * an index only into a slot below max_out; report i holds the exact number of
 * differing indices, also above max_out, and the smallest one (2^64 - 1: none).
 * `trees` is host memory, read only during the call: the descriptors travel as
 * kernel arguments.  Allocates nothing, uploads nothing, needs no workspace,
 * never synchronises, writes nothing but d_reports and the d_idx_out, and can be
 * captured into a hipGraph.  The leaves of a LIST tree at any byte alignment;
 * d_*_level0 (NULL for MK_TREE_LIST) and d_*_levels 16-B aligned, d_idx_out and
 * d_reports (ntrees reports) 8-B aligned.  d_*_items of a STRUCT / BYTES tree
 * are not read.  The same buffers on both sides are allowed: the result is empty.
 * MK_EINVAL, every check before a device is looked up and nothing launched:
 * ntrees 0 or > MK_TREES_MAX, an unknown kind, item_len == 0, a LIST item_len
 * above 128, n above its capacity, capacity * item_len overflowing, a level 0
 * given for a list tree, null or misaligned pointers where the shape needs them
 * (the leaves for m > 0, the levels for min(D_a, D_b) >= 1), d_idx_out NULL with
 * max_out > 0, an output range that overlaps an input range of the call (a
 * tree's levels count from the first stored node to its top) or another output
 * range, 2^31 or more work items (a work item is a subtree of 2^10 chunks). */
typedef struct mk_tree_diff {
    uint32_t kind, item_len;            /* MK_TREE_LIST / _STRUCT / _BYTES; item / record / element length */
    const void *d_a_items, *d_a_level0, *d_a_levels;
    const void *d_b_items, *d_b_level0, *d_b_levels;
    uint64_t n_a, capacity_a, n_b, capacity_b;
    uint64_t* d_idx_out;                /* max_out slots, 8-B aligned; NULL with max_out == 0 */
    uint64_t max_out;
} mk_tree_diff;
typedef struct mk_diff_report {
    uint64_t total;                     /* differing indices below min(n_a, n_b) */
    uint64_t first_index;               /* the smallest; 2^64 - 1: none */
} mk_diff_report;
int mk_dev_ssz_trees_diff(mk_call* call, const mk_tree_diff* trees, uint32_t ntrees, void* d_reports, void* stream);
/* Handle forms, the same for the three kinds: the diff of a's tree against b's,
 * one launch and one read-back.  Both handles must agree in kind, item length,
 * record layout and device, else MK_EINVAL; both mutexes are taken in address
 * order.  idx_out (max_out slots, NULL with max_out == 0) gets the differing
 * indices ascending; *total their exact number, *n_a and *n_b the two counts.
 * With *total > max_out the first max_out slots hold some max_out of the
 * differing indices, still ascending: call again with a larger buffer.  a == b
 * is MK_OK with *total == 0. */
int mk_list_tree_diff(mk_call* call, mk_list_tree* a, mk_list_tree* b, uint64_t* idx_out, uint64_t max_out,
                      uint64_t* total, uint64_t* n_a, uint64_t* n_b);
int mk_struct_list_tree_diff(mk_call* call, mk_struct_list_tree* a, mk_struct_list_tree* b, uint64_t* idx_out,
                             uint64_t max_out, uint64_t* total, uint64_t* n_a, uint64_t* n_b);
int mk_bytes_list_tree_diff(mk_call* call, mk_bytes_list_tree* a, mk_bytes_list_tree* b, uint64_t* idx_out,
                            uint64_t max_out, uint64_t* total, uint64_t* n_a, uint64_t* n_b);
/* The same for two sets, which must agree as mk_tree_set_copy requires (else
 * MK_EINVAL and nothing changes).  Both are flushed first, as root does; ONE
 * launch covers all the trees and one read-back follows.  reports: count + 1.
 * Tree i's indices go to idx_out + i * max_out_per_tree, ascending, its report
 * to reports[i]; the last report describes the container: `total` is the number
 * of message bytes outside every tree's 32-byte root range that differ,
 * compared on the host from the sets' own copies, `first_index` the first such
 * offset.  idx_out may be NULL with max_out_per_tree == 0.  a == b is MK_OK with
 * every total 0.  The counts are mk_tree_set_count's.  The deposit trie has no
 * diff. */
int mk_tree_set_diff(mk_call* call, mk_tree_set* a, mk_tree_set* b, mk_diff_report* reports, uint64_t* idx_out,
                     uint64_t max_out_per_tree);

/* ---- hashutil.MerkleRoot (merkleRoot.go:12-30) -------------------------- */
/* Root of the heap o[i] = Hash(o[2i] || o[2i+1]) over leaves
 * o[n+i] = Hash(values[i]); values i = data[offs[i], offs[i+1]).  leaves_out
 * (optional, n x 32) receives Hash(values[i]): the reference overwrites its
 * input slice with them (merkleRoot.go:16-19) and a drop-in keeps that side
 * effect.  n == 0 is MK_EINVAL (the reference panics: index out of range). */
int mk_merkle_root(mk_call* call, const uint8_t* data, const uint64_t* offs, uint64_t n, uint8_t* leaves_out,
                   uint8_t out[32]);
uint64_t mk_merkle_root_workspace_bytes(uint64_t n);
/* Device-resident: d_offs (n+1, device) or fixed_len; d_heap of
 * mk_merkle_root_workspace_bytes(n); d_leaves32 optional (n x 32). */
int mk_dev_merkle_root(mk_call* call, const void* d_data, const uint64_t* d_offs, uint64_t n, uint32_t fixed_len,
                       void* d_heap, uint64_t heap_bytes, void* d_leaves32, void* d_out32, void* stream);

/* ---- hashutil.RepeatHash (hash.go:29-34): chains, hash onions, the RANDAO check ---- */
/* RepeatHash(x, k) is Keccak-256 applied k times to a 32-byte value; k == 0 returns x.  One chain is serial; its
 * callers are not: verifyBlockRandao (block_operations.go:109-123) runs one chain per block, the hash onions
 * (chaintest/backend/helpers.go:125-135) one per validator with every layer kept.  A chain never leaves the
 * registers of the lane or wave that runs it.
 *
 * Layer counts are data (RandaoLayers comes from a proposer's record), so every entry takes max_layers, the most
 * permutations a chain of this call may run, and MK_EINVAL answers max_layers > MK_REPEAT_MAX_LAYERS.  Nothing a
 * caller passes makes a kernel run more than max_layers permutations per chain.
 *
 * form: MK_REPEAT_LANE runs one chain per GPU lane (a wave runs for as long as its longest chain; shorter ones
 * wait masked off), MK_REPEAT_WAVE one chain per wave (for few chains: 2.8 against 8.7-10 us per layer of a lone chain),
 * MK_REPEAT_AUTO picks by the number of chains.  The results are the same bit for bit; the forced forms exist
 * for tests and timing.  The host entries use MK_REPEAT_AUTO.
 *
 * Device pointers may have any alignment; 16-B aligned seeds and outputs (and, for a verify, records, stride and
 * offsets that are multiples of 4) take whole-word accesses, anything else goes byte by byte.  n == 0 (m == 0) is
 * MK_OK and launches nothing; n, m < 2^31. */
#define MK_REPEAT_MAX_LAYERS (1u << 20)
#define MK_REPEAT_AUTO 0u
#define MK_REPEAT_LANE 1u
#define MK_REPEAT_WAVE 2u
/* the verdict bytes of a verify */
#define MK_REPEAT_BAD 0       /* the chain's end is not the commitment */
#define MK_REPEAT_OK 1        /* RepeatHash(reveal, layers) == commitment */
#define MK_REPEAT_TOO_DEEP 2  /* the record's 64-bit layer count exceeds max_layers: the chain was not run */
#define MK_REPEAT_NO_RECORD 3 /* idx >= n_records (device entry only: the host entries refuse the call) */
/* chain: d_out[i] = RepeatHash(d_seeds[i], d_layers[i]) (n x 32 bytes each, d_layers n x u32).  The host cannot
 * see d_layers: a chain whose count exceeds max_layers gets 32 zero bytes and sets bit 0 of *d_status (one u32
 * of the caller's workspace, 4-B aligned); the other chains are unaffected.  The call only ever sets the word:
 * the caller clears it once and may check it after any number of calls (a clear per call would be a second
 * stream operation beside a launch of a few microseconds). */
int mk_dev_repeat_hash(mk_call* call, const void* d_seeds, const uint32_t* d_layers, uint64_t n, uint32_t max_layers,
                       uint32_t form, void* d_out, uint32_t* d_status, void* stream);
/* onion: d_out[i][t] = RepeatHash(d_seeds[i], t), t = 0 .. layers: n x (layers + 1) x 32 bytes, row 0 the seed,
 * each row stored as its layer completes.  layers <= MK_REPEAT_MAX_LAYERS. */
int mk_dev_hash_onion(mk_call* call, const void* d_seeds, uint64_t n, uint32_t layers, uint32_t form, void* d_out,
                      void* stream);
/* verify: for proposal j, rec = d_records + d_idx[j] * stride, d_ok[j] (one byte) = MK_REPEAT_OK when
 * RepeatHash(d_reveals[j], le64(rec + layers_off)) == rec[commit_off, commit_off + 32), else one of the codes
 * above.  The layer count is compared as 64 bits.  commit_off + 32 and layers_off + 8 <= stride.  Indices may
 * repeat.  For the 160-B ValidatorRecord: stride 160, commit_off 80, layers_off 112. */
int mk_dev_verify_repeat_hash(mk_call* call, const void* d_records, uint64_t n_records, uint64_t stride,
                              uint32_t commit_off, uint32_t layers_off, const uint64_t* d_idx, const void* d_reveals,
                              uint64_t m, uint32_t max_layers, uint32_t form, uint8_t* d_ok, void* stream);
/* The same on host buffers (upload, one launch, read-back).  A layers[i] > max_layers is MK_EINVAL naming the
 * first such i, with nothing launched and `out` untouched; so is an idx[j] >= n_records. */
int mk_repeat_hash_batch(mk_call* call, const uint8_t* seeds, const uint32_t* layers, uint64_t n, uint32_t max_layers,
                         uint8_t* out);
/* RepeatHash itself; num_times > MK_REPEAT_MAX_LAYERS is MK_EINVAL. */
int mk_repeat_hash(mk_call* call, const uint8_t data[32], uint64_t num_times, uint8_t out[32]);
int mk_hash_onion(mk_call* call, const uint8_t* seeds, uint64_t n, uint32_t layers, uint8_t* out);
int mk_verify_repeat_hash(mk_call* call, const uint8_t* records, uint64_t n_records, uint64_t stride,
                          uint32_t commit_off, uint32_t layers_off, const uint64_t* idx, const uint8_t* reveals,
                          uint64_t m, uint32_t max_layers, uint8_t* ok);
/* The verify against the records a resident registry tree owns: only idx and the reveals go up and the m
 * verdicts come back; no record is read back.  Read-only (root, levels and records stay as they are).  idx[j] >=
 * the tree's count, commit_off + 32 or layers_off + 8 > the record length are MK_EINVAL with nothing launched.
 * The set's form takes tree number `tree`, which must be an MK_TREE_STRUCT tree, and flushes pending changes
 * first, as mk_tree_set_branches does: a pending update is seen. */
int mk_struct_list_tree_verify_repeat_hash(mk_call* call, mk_struct_list_tree* t, uint32_t commit_off,
                                           uint32_t layers_off, const uint64_t* idx, const uint8_t* reveals,
                                           uint64_t m, uint32_t max_layers, uint8_t* ok);
int mk_tree_set_verify_repeat_hash(mk_call* call, mk_tree_set* s, uint32_t tree, uint32_t commit_off,
                                   uint32_t layers_off, const uint64_t* idx, const uint8_t* reveals, uint64_t m,
                                   uint32_t max_layers, uint8_t* ok);

/* ---- trieutil deposit trie (deposit_trie.go:29-81) ---------------------- */
/* Level array of a depth-`depth` trie with room for `capacity` leaves: level
 * d (d = 0: leaf hashes Hash(deposit)) starts at node
 * sum_{i<d} ceil(capacity / 2^i) and holds ceil(count / 2^d) nodes.  Empty
 * nodes are 0^32 (Go map miss), root = level `depth` node 0 (0^32 when
 * count == 0). */
uint64_t mk_deposit_trie_levels_bytes(uint64_t capacity, uint32_t depth);
/* Batch build of n deposits (message i = data[offs[i], offs[i+1])) = n calls
 * of UpdateDepositTrie.  levels_out (nullable) receives the level array with
 * capacity n (the data GenerateMerkleBranch reads). */
int mk_deposit_trie_build(mk_call* call, const uint8_t* data, const uint64_t* offs, uint64_t n, uint32_t depth,
                          uint8_t* levels_out, uint8_t root[32]);
/* Device-resident append: the trie in d_levels (capacity `capacity`) holds
 * `count` deposits; deposits count .. count+k-1 are d_data[d_offs[i],
 * d_offs[i+1]) (i < k) or, with d_offs == NULL, fixed_len-byte records (the
 * 280-B deposit-data layout of core/blocks/block.go:103-130).  Hashes the k
 * leaves and recomputes only the right edge of every level above them
 * (<= k/2^d + 2 nodes at level d): UpdateDepositTrie's O(depth) path per
 * deposit (deposit_trie.go:29-40), batched.  count == 0 is the batch build.
 * The new root goes to d_root32.  count + k <= capacity. */
int mk_dev_deposit_trie_append(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, const void* d_data,
                               const uint64_t* d_offs, uint64_t k, uint32_t fixed_len, uint32_t depth,
                               void* d_root32, void* stream);
/* Batch build front: the leaf hashes Hash(deposit) of n deposits into level 0
 * of an empty trie plus levels 1 .. d_to (the root to d_root32 when d_to ==
 * depth; d_root32 may be NULL otherwise).  Deposits as in
 * mk_dev_deposit_trie_append.  With mk_dev_deposit_trie_levels(d_to, depth)
 * this splits one batch build (deposit_trie.go:29-40) across two streams. */
int mk_dev_deposit_trie_build(mk_call* call, void* d_levels, uint64_t capacity, const void* d_data,
                              const uint64_t* d_offs, uint64_t n, uint32_t fixed_len, uint32_t d_to, uint32_t depth,
                              void* d_root32, void* stream);
/* A stream of equal-size tries with each trie's wide top folded into the
 * NEXT trie's front: levels 0..2 of the trie in d_levels (its leaves and the
 * nodes over 2 and 4 of them) and, in the same launch, levels 3..7 of the
 * previous trie in d_prev_levels (NULL for the first trie; the same n and
 * capacity; its levels 0..2 from the previous call).  Then
 * mk_dev_deposit_trie_pipe_top(d_prev_levels, ..) finishes the previous trie
 * (on another stream, beside the next front), and
 * mk_dev_deposit_trie_levels(d_levels, .., 2, depth) the last one.  Takes what
 * mk_deposit_trie_pipe_ok accepts on the same stream (280-B deposits, 16-B
 * aligned, n a multiple of 4096 and at most 4096 x the CUs the stream may
 * use, depth >= 7); MK_EINVAL otherwise.  pipe_ok returns 1 or 0 (0 also
 * when the stream cannot be bound). */
int mk_deposit_trie_pipe_ok(const void* d_data, uint64_t n, uint32_t deposit_len, uint32_t depth, void* stream);
/* Levels 8 .. depth and the root of a trie whose levels 0..7 are complete
 * (a pipelined front's previous trie), in launches of at most one wave per
 * SIMD, which run beside the next pipelined front instead of after it. */
int mk_dev_deposit_trie_pipe_top(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, uint32_t depth,
                                 void* d_root32, void* stream);
int mk_dev_deposit_trie_build_pipe(mk_call* call, void* d_levels, void* d_prev_levels, uint64_t capacity,
                                   const void* d_data, uint64_t n, uint32_t deposit_len, uint32_t depth,
                                   void* stream);
/* Levels d_from+1 .. d_to of the batch build of a `count`-deposit trie whose
 * level d_from is complete (the root to d_root32 when d_to == depth): lets a
 * caller hash the leaves and the wide levels of trie i+1 on one stream while
 * the narrow, latency-bound top of trie i runs on another. */
int mk_dev_deposit_trie_levels(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, uint32_t d_from,
                               uint32_t d_to, uint32_t depth, void* d_root32, void* stream);
/* GenerateMerkleBranch (deposit_trie.go:43-58) from a device level array:
 * d_branch[d] = sibling of `index`'s ancestor at level d (0^32 if absent). */
int mk_dev_deposit_trie_branch(mk_call* call, const void* d_levels, uint64_t capacity, uint64_t count,
                               uint32_t depth, uint64_t index, void* d_branch, void* stream);

/* GenerateMerkleBranch for k indices and Root(), as of a past deposit count:
 * what the reference's trie answered right after its as_of-th
 * UpdateDepositTrie (0 <= as_of <= count), from the level array later appends
 * left behind.  verifyDeposit (core/blocks/block_operations.go:624-641) checks
 * a deposit against state.LatestEth1Data.DepositRootHash32, an earlier state
 * of the trie than the one powchain holds; these are the branches for it.
 * d_indices: k indices on the device, any order, repeats allowed, none read
 * on the host (a sibling that did not exist at as_of, or that no index below
 * 2^depth can have, is 0^32).  d_branches: k x depth x 32 bytes, branch j at
 * 32 * depth * j.  d_root_at (nullable): the 32-B root as of as_of (0^32 for
 * as_of == 0).  One launch; allocates nothing, uploads nothing and never
 * synchronizes, so it can be captured into a hipGraph.  d_levels, d_branches
 * and d_root_at 16-B aligned.  MK_EINVAL (nothing launched): as_of > count,
 * count > capacity, depth outside 1..63.  k == 0 writes only d_root_at. */
int mk_dev_deposit_trie_branches(mk_call* call, const void* d_levels, uint64_t capacity, uint64_t count,
                                 uint32_t depth, uint64_t as_of, const uint64_t* d_indices, uint64_t k,
                                 void* d_branches, void* d_root_at, void* stream);
/* verifyDeposit for a batch of n deposits: ok[i] = fold(Hash(data[offs[i],
 * offs[i+1])), branches[i*depth..], indices[i] + 2^tree_depth) == root, with
 * root = d_roots[0, 32) for every deposit when root_stride == 0 (a block's
 * deposits against the state's deposit root) or d_roots[32 i, 32 i + 32) when
 * root_stride == 32; any other root_stride is MK_EINVAL.  Replaces a
 * mk_dev_hash_batch_var call plus the leaf-hash verifier.  d_offs: n + 1
 * offsets into d_data, device.  d_branches and d_roots 16-B aligned.  One
 * launch; allocates nothing, uploads nothing, never synchronizes. */
int mk_dev_verify_deposits(mk_call* call, const void* d_data, const uint64_t* d_offs, const void* d_branches,
                           const uint64_t* d_indices, uint64_t n, uint32_t depth, uint32_t tree_depth,
                           const void* d_roots, uint32_t root_stride, void* d_ok, void* stream);

/* Device-resident trie handle: the Go DepositTrie (deposit_trie.go:13-16)
 * holds one.  Levels stay in HBM (capacity doubles on demand); appends
 * recompute only the right edge, so powchain's read-Root-then-Update loop
 * (powchain/service.go:379-386) costs O(depth) hashes per deposit. */
typedef struct mk_trie mk_trie;
int mk_deposit_trie_new(mk_call* call, uint32_t depth, uint64_t capacity, mk_trie** out);
void mk_deposit_trie_free(mk_trie* t);
uint64_t mk_deposit_trie_count(const mk_trie* t);
/* Appends k deposits (host data, message i = data[offs[i], offs[i+1])). */
int mk_deposit_trie_append(mk_call* call, mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k);
/* powchain's deposit-log loop in one call (ProcessDepositLog -> saveInTrie,
 * powchain/service.go:248-258, 379-386): for each of the k logs in order,
 * deposit j (data[offs[j], offs[j+1])) is appended iff the trie's Root()
 * before it equals log_roots[32 j .. 32 j + 32) (the merkle root the log
 * carries); a mismatching log is skipped, as the reference skips a log
 * whose saveInTrie fails, and processing continues with the next log.
 * accepted[j] = 1 if deposit j was appended, else 0.  All roots are
 * computed on the device in parallel (one chain of `depth` permutations
 * per log), so a batch costs about one append. */
int mk_deposit_trie_save_logs(mk_call* call, mk_trie* t, const uint8_t* data, const uint64_t* offs, uint64_t k,
                              const uint8_t* log_roots, uint8_t* accepted);
int mk_deposit_trie_root(mk_call* call, mk_trie* t, uint8_t root[32]);
/* depth x 32 bytes: GenerateMerkleBranch(index). */
int mk_deposit_trie_branch(mk_call* call, mk_trie* t, uint64_t index, uint8_t* branch);
/* k x depth x 32 bytes: GenerateMerkleBranch(indices[j]) as of as_of <=
 * count deposits (mk_dev_deposit_trie_branches over the handle: host indices
 * and output, the root as of as_of to root_at when it is not NULL).
 * as_of > count: MK_EINVAL, nothing written.  k == 0 writes only root_at.  A
 * very large k runs in chunks of bounded device scratch. */
int mk_deposit_trie_branches(mk_call* call, mk_trie* t, uint64_t as_of, const uint64_t* indices, uint64_t k,
                             uint8_t* branches, uint8_t* root_at);
/* Root() as of as_of <= count deposits (0^32 for as_of == 0). */
int mk_deposit_trie_root_at(mk_call* call, mk_trie* t, uint64_t as_of, uint8_t root[32]);
/* Leaf hashes [first, first + cnt) (Hash(deposit)), cnt x 32 bytes. */
int mk_deposit_trie_leaves(mk_call* call, mk_trie* t, uint64_t first, uint64_t cnt, uint8_t* out);

/* ---- the resident deposit trie rolled back, compared, audited, copied ---- */
/* cnt(c, d) = ceil(c / 2^d) nodes of level d are LIVE in a trie of c deposits;
 * a node at or beyond that is dead: no entry point of this library reads one.
 * truncate: the trie of the first new_count <= count deposits, without the
 *   deposit data: per level d = 1 .. depth at most one node, (new_count - 1) >>
 *   d, covers deposits on both sides of new_count; it gets the value it had
 *   after the new_count-th append, one chain of at most `depth` hashes from the
 *   stored nodes (the as-of rule of mk_dev_deposit_trie_branches).  Nothing else
 *   of the level array is written, dead nodes keep their bytes; the root goes
 *   to d_root32 (0^32 for new_count == 0, when level `depth` node 0 is zeroed
 *   too).  new_count == count writes only the root.  One single-wave launch.
 *   ETH1 reorganisations (types.Log.Removed): roll back to the removed log's
 *   deposit index, then append again.
 * fork_point: the smallest leaf index i < m = min(count_a, count_b) at which
 *   the two tries' level-0 nodes differ, m when none does, as one uint64 to
 *   d_out8.  Both tries have depth `depth`; counts and capacities may differ.
 *   Only nodes whose leaves all lie below m are compared; nothing is hashed.
 *   One single-wave launch.
 * audit: for d = 1 .. depth and j < cnt(count, d), stored node (d, j) against
 *   K(level_{d-1}[2j] || R), R = level_{d-1}[2j+1] when 2j+1 < cnt(count, d-1),
 *   else 0^32; d_root32 against level `depth` node 0 (0^32 for count == 0).
 *   The report is mk_audit_report: keys (level, index), levels 1 .. depth and
 *   MK_AUDIT_ROOT; level 0 is never reported (no deposit data is kept).  A wrong
 *   interior node is reported where it is stored and one level up.  More than
 *   2^31 work items is MK_EINVAL.  Three launches in a chain: the report
 *   cleared, every node in one launch, the key unpacked.
 * copy: the live nodes of level 0 .. depth from the layout of src_capacity to
 *   that of dst_capacity >= count, and the root (both root pointers NULL: no
 *   root travels).  The buffers must not overlap.  One launch.
 * All four: d_levels and roots 16-B aligned, d_report and d_out8 8-B aligned.
 * MK_EINVAL, every check before a device is looked up and nothing launched:
 * new_count > count, count > capacity, a count above 2^depth, depth outside
 * 1..63, a null or misaligned pointer, overlapping copy buffers.  They allocate
 * nothing, upload nothing, never synchronise and can be captured into a
 * hipGraph (a linear chain of nodes). */
int mk_dev_deposit_trie_truncate(mk_call* call, void* d_levels, uint64_t capacity, uint64_t count, uint64_t new_count,
                                 uint32_t depth, void* d_root32, void* stream);
int mk_dev_deposit_trie_fork_point(mk_call* call, const void* d_levels_a, uint64_t capacity_a, uint64_t count_a,
                                   const void* d_levels_b, uint64_t capacity_b, uint64_t count_b, uint32_t depth,
                                   void* d_out8, void* stream);
int mk_dev_deposit_trie_audit(mk_call* call, const void* d_levels, uint64_t capacity, uint64_t count, uint32_t depth,
                              const void* d_root32, void* d_report, void* stream);
int mk_dev_deposit_trie_copy(mk_call* call, const void* d_src_levels, uint64_t src_capacity, uint64_t count,
                             void* d_dst_levels, uint64_t dst_capacity, uint32_t depth, const void* d_src_root32,
                             void* d_dst_root32, void* stream);
/* Handle forms, one synchronise each.  truncate: the first n deposits stay
 * (n > count: MK_EINVAL, nothing changes).  fork_point(a, a) is the count.
 * clone: a new handle of src's depth and capacity on its device, no hashing.
 * copy: dst becomes src; dst grows to src's capacity only if src's count
 * does not fit.  reserve: room for `capacity` deposits (never shrinks).  Tries
 * of different depth or on different devices are MK_EINVAL; two handles are
 * locked in address order. */
int mk_deposit_trie_truncate(mk_call* call, mk_trie* t, uint64_t n);
int mk_deposit_trie_fork_point(mk_call* call, mk_trie* a, mk_trie* b, uint64_t* out);
int mk_deposit_trie_audit(mk_call* call, mk_trie* t, mk_audit_report* out);
int mk_deposit_trie_clone(mk_call* call, mk_trie* src, mk_trie** out);
int mk_deposit_trie_copy(mk_call* call, mk_trie* dst, mk_trie* src);
int mk_deposit_trie_reserve(mk_call* call, mk_trie* t, uint64_t capacity);
uint64_t mk_deposit_trie_capacity(const mk_trie* t);

/* Batched VerifyMerkleBranch: ok[i] = fold(leaves[i], branches[i*depth..],
 * indices[i] + 2^tree_depth) == roots[i]. */
int mk_verify_merkle_branches(mk_call* call, const uint8_t* leaves, const uint8_t* branches,
                              const uint64_t* indices, uint64_t n, uint32_t depth, uint32_t tree_depth,
                              const uint8_t* roots, uint8_t* ok);
/* mk_dev_verify_deposits over host buffers (deposit i = data[offs[i],
 * offs[i+1]); roots: 32 bytes for root_stride == 0, n x 32 for 32). */
int mk_verify_deposits(mk_call* call, const uint8_t* data, const uint64_t* offs, const uint8_t* branches,
                       const uint64_t* indices, uint64_t n, uint32_t depth, uint32_t tree_depth,
                       const uint8_t* roots, uint32_t root_stride, uint8_t* ok);

/* ---- synthetic inputs (bench / tests) ----------------------------------- */
/* Bytes [8*word0, 8*word0 + nbytes) of the SplitMix64 stream;
 * nbytes must be a multiple of 8. */
int mk_dev_synth_fill(mk_call* call, void* d_dst, uint64_t nbytes, uint64_t seed, uint64_t word0, void* stream);

/* ---- measurement -------------------------------------------------------- */
/* When enabled, every dev merkle call records hipEvents around its dominant
 * (leaf) kernel launches on the call's stream; mk_prof_read synchronises those
 * events and returns the summed milliseconds, launch count, algorithmic
 * Keccak-f permutations and digests (hashes) of those launches, then resets.
 * Any out-pointer may be NULL. */
int mk_prof_enable(int on);
int mk_prof_read(mk_call* call, double* leaf_ms, uint64_t* leaf_launches, double* leaf_perms, double* leaf_hashes);

#ifdef __cplusplus
}
#endif
#endif /* PRYSM_MERKLE_H */
