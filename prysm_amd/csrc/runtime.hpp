// Internal header of libprysm_merkle.so's host side: the device context and
// call scope (runtime.cpp) and every function that crosses translation units
// (hash_api, merkle_api, struct_api, trie_api, multi_api, capi).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "merkle_kernels.hpp"
#include "planner.hpp"
#include "prysm_merkle.h"

#define HIPCHK(x)                                                                            \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) return mk::fail(MK_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

#define TRY(x)                        \
    do {                              \
        int rc_ = (x);                \
        if (rc_ != MK_OK) return rc_; \
    } while (0)

namespace mk::rt {

// ---- devices (runtime.cpp) -------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
int grow(DevBuf& b, size_t bytes);

// small pinned upload ring: descriptor tables for dev entry points (the
// source must outlive the async copy; a slot is reused after its event)
struct SmallStage {
    std::mutex mu;
    static constexpr int kSlots = 4;
    void* host[kSlots] = {};
    size_t cap[kSlots] = {};
    hipEvent_t ev[kSlots] = {};
    bool used[kSlots] = {};
    int next = 0;
};

struct DevCtx {
    std::mutex mu;  // host-buffer entry points: in/out/ws/aux and the big staging
    hipStream_t stream = nullptr;
    DevBuf in, out, ws, aux, dig;  // dig: element digests of the multi-shard TreeHash path
    // side stream + events: the ragged last workgroup of a pass runs
    // concurrently with the pass's full workgroups (fork/join on events)
    std::mutex side_mu;
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;

    // host-buffer uploads on `copy` overlapping compute on `stream`
    hipStream_t copy = nullptr;
    hipEvent_t h2d = nullptr;
    hipEvent_t region_ev[2] = {nullptr, nullptr};  // multi: compute of a shard region done
    bool region_used[2] = {false, false};
    SmallStage small;
    // mk_dev_ssz_merkle_hash_multi's own frontier blocks / workspaces: that
    // path enqueues on the caller's streams without this device's `mu`, so it
    // must never share in/out/ws/aux with the host-buffer entry points
    DevBuf mout, mws, maux;
};

extern std::vector<DevCtx*> g_ctx;  // one per visible device, created by bind_dev
extern thread_local int t_bound;    // device bound by the current call
inline DevCtx* ctx() { return g_ctx[t_bound]; }

int probe_devices();  // visible gfx950 devices
int bind_dev(int dev);
int bind_call();
int bind_stream(hipStream_t st);
int upload_small(DevCtx* c, void* d_dst, const void* src, size_t bytes, hipStream_t st);
bool inject_ehip();
uint64_t lock_grid_cap(hipStream_t st);
inline int launched() {  // after a kernel launch: MK_OK, or MK_EHIP with the launch's error
    HIPCHK(hipGetLastError());
    return MK_OK;
}

// Per-call scope of an extern "C" entry point: installs the call context,
// restores the thread's current device on exit.
struct Scope {
    mk_call* prev;
    int saved = -1;
    bool restore = false;
    explicit Scope(mk_call* c, bool gpu = true) {
        prev = mk::swap_call(c);
        if (c) {
            c->code = MK_OK;
            c->err[0] = 0;
        }
        if (gpu && probe_devices() > 0) restore = hipGetDevice(&saved) == hipSuccess;
    }
    int done(int rc) {
        if (mk::current_call()) mk::current_call()->code = rc;
        return rc;
    }
    ~Scope() {
        int cur = -1;
        if (restore && hipGetDevice(&cur) == hipSuccess && cur != saved) (void)hipSetDevice(saved);
        t_bound = -1;
        mk::swap_call(prev);
    }
};

// Prologue of a device entry point: the call scope, the stream's device, then
// `body` (its argument checks and launches, in that order).
template <class F>
inline int dev_entry(mk_call* call, void* stream, const F& body) {
    Scope S(call);
    const int rc = bind_stream((hipStream_t)stream);
    return S.done(rc ? rc : body());
}

// ---- measurement (runtime.cpp) -----------------------------------------------
// One timed launch (or group of launches) of a leaf pass, mk_prof_read's input.
struct ProfRec {
    hipEvent_t a, b;
    double perms, hashes;
};
bool prof_on();
void prof_enable(bool on);
int prof_begin(ProfRec& r, hipStream_t st);                               // creates the events, records r.a
int prof_end(ProfRec& r, double perms, double hashes, hipStream_t st);  // records r.b and files the record
int prof_read(double* leaf_ms, uint64_t* leaf_launches, double* leaf_perms, double* leaf_hashes);

// ---- hashing (hash_api.cpp) ----------------------------------------------------
int dev_hash_batch(const void* d_in, uint64_t n, uint32_t msg_len, void* d_out, hipStream_t st);
int dev_hash_var(const void* d_in, const uint64_t* d_offs, uint64_t n, void* d_out, hipStream_t st);
int64_t uniform_len(const uint64_t* offs, uint64_t n);  // uniform message length of offs[0..n] (relative), or -1

// ---- RepeatHash in batches (repeat_api.cpp) ------------------------------
// the argument rules every entry shares (no device needed): the cap, the form and the size of one launch; the two
// fields inside `stride` bytes (`what` names it in the message); every index below `count`
int repeat_check_call(uint64_t n, uint32_t max_layers, uint32_t form);
int repeat_check_offsets(uint64_t stride, uint32_t commit_off, uint32_t layers_off, const char* what);
int repeat_check_indices(const uint64_t* idx, uint64_t m, uint64_t count, const char* noun);
// the verify against the records a registry tree's handle owns (MK_TREE_STRUCT only): idx and the reveals up,
// one launch, the m verdicts back.  Takes t's lock; read-only.
struct TreeHandle;
int tree_verify_repeat_hash(TreeHandle* t, uint32_t commit_off, uint32_t layers_off, const uint64_t* idx,
                            const uint8_t* reveals, uint64_t m, uint32_t max_layers, uint8_t* ok);

// ---- merkleHash (merkle_api.cpp) -------------------------------------------------
inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
int launch_plan(const Plan& p, const uint8_t* d_items, uint8_t* d_out32, uint8_t* d_ws, uint64_t ws_bytes,
                hipStream_t st, uint8_t* pair_block = nullptr, uint32_t pair_slot = 0, uint32_t pair_epoch = 0);
bool list_tree_ok(uint64_t n, uint32_t item_len);      // the latency form of a small list's tree applies
uint64_t list_tree_ws(uint64_t n, uint32_t item_len);  // its workspace (0: not that form)
int dev_merkle_hash(const void* d_items, uint64_t n, uint32_t item_len, void* d_out32, void* d_ws, uint64_t ws_bytes,
                    hipStream_t st);
int dev_finish(const void* d_roots, uint64_t nroots, uint64_t n_total, void* d_out32, hipStream_t st,
               void* d_pair_block = nullptr, uint32_t pair_slot = 0, uint32_t pair_epoch = 0);
uint64_t finish_ws_bytes(uint64_t count);
int dev_finish_nodes(const void* d_nodes, uint64_t count, uint64_t n_total, void* d_out32, void* d_ws,
                     uint64_t ws_bytes, hipStream_t st, void* d_pair_block = nullptr, uint32_t pair_slot = 0,
                     uint32_t pair_epoch = 0);
int launch_elem_digests(const void* d_elems, uint64_t n, uint32_t elem_len, void* d_dig, hipStream_t st);
int host_tree_hash_elems_plain(const uint8_t* elems, uint64_t n, uint32_t elem_len, uint8_t* out);
int host_merkle_hash_plain(const uint8_t* items, uint64_t n, uint32_t item_len, uint8_t* out);
// arrival-counter slots of the fused tops (mk::g_arrive): also the trie's and the struct list's
uint32_t next_arrive_slots(uint32_t k);
uint32_t top_arrive_slots(uint64_t parts);

// ---- flat records (struct_api.cpp) ------------------------------------------------
int struct_make_spec(const mk_field* fields, uint32_t nfields, uint32_t record_len, mk::HostSpec& sp);
// a layout whose roots launch needs no message buffer: what k_struct_fused or k_struct_nested takes (4-B aligned records)
bool struct_fused_layout(const mk::HostSpec& sp);
// roots of n records into d_roots (n x 32); d_msg: n x msg_len bytes (unused for a fused layout)
int struct_launch_roots(const void* d_rec, uint64_t n, const mk::HostSpec& sp, void* d_msg, void* d_roots,
                        hipStream_t st);

// ---- list tree over 32-B items (list_tree_api.cpp) -----------------------------------
constexpr uint64_t kMaxWork = 1ull << 31;  // work items of one tree update launch
int list_tree_build32(const void* d_roots, uint64_t n, uint64_t capacity, void* d_levels, void* d_root32, void* d_ws,
                      hipStream_t st);  // d_ws: 256 B
int list_tree_update32(const void* d_roots, void* d_levels, const uint64_t* d_idx, uint64_t k_idx, uint64_t n_old,
                       uint64_t n_new, uint64_t capacity, void* d_root32, void* d_ws, hipStream_t st);  // > 4 items
int list_tree_scatter(void* d_items, const uint64_t* d_idx, uint64_t k_idx, uint64_t n_old, uint64_t n_app,
                      uint32_t item_len, const void* d_values, hipStream_t st);

// ---- one tree of mk_dev_ssz_trees_update (tree_many_api.cpp) ----------------------------
// What each kind's own update entry point runs, shared with the call over
// several trees: its host-checkable arguments, its pointer checks, its stage 0
// (every launch before the climb: the values scattered in, level 0 brought up
// to date) and the climb's descriptor.
int list_tree_check_update(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len, uint64_t k_idx,
                           uint64_t ws_bytes);
int list_tree_check_ptrs(const void* d_items, uint64_t n, uint64_t capacity, uint32_t item_len, const void* d_levels,
                         const void* d_root32, const void* d_ws);
mk::ListTreeArgs list_tree_args(const void* d_items, void* d_levels, const uint64_t* d_idx, uint64_t k_idx,
                                uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len, void* d_root32,
                                void* d_arrive);
struct StructTreeLayout {
    mk::HostSpec sp;
    bool fused;    // the struct-roots launch needs no message buffer (k_struct_fused, k_struct_nested)
    uint32_t ext;  // bytes of a record the fields reach, rounded up to 4 (<= rec_len)
};
int struct_tree_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, StructTreeLayout& L);
// the update workspace for k work items; *arrive_bytes: its leading part, the arrival words (the rest is scratch)
uint64_t struct_tree_update_ws(const StructTreeLayout& L, uint64_t k, uint64_t* arrive_bytes);
int struct_tree_check_update(const StructTreeLayout& L, uint64_t n_old, uint64_t n_new, uint64_t capacity,
                             uint64_t k_idx, uint64_t ws_bytes);
int struct_tree_check_ptrs(const void* d_records, uint64_t n, uint64_t capacity, const void* d_roots,
                           const void* d_levels, const void* d_root32, const void* d_ws);
int struct_tree_stage0(const StructTreeLayout& L, void* d_records, uint64_t n_old, uint64_t n_new, void* d_roots,
                       const uint64_t* d_idx, uint64_t k_idx, const void* d_values, void* d_scratch, hipStream_t st);
int bytes_tree_check_update(uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t elem_len, uint64_t k_idx,
                            uint64_t ws_bytes);
int bytes_tree_check_ptrs(const void* d_elems, uint64_t n, uint64_t capacity, const void* d_digests,
                          const void* d_levels, const void* d_root32, const void* d_ws);
int bytes_tree_stage0(void* d_elems, uint64_t n_old, uint64_t n_new, uint32_t elem_len, void* d_digests,
                      const uint64_t* d_idx, uint64_t k_idx, const void* d_values, hipStream_t st);

// ---- the host handle of a resident tree (tree_handle.cpp) -------------------------------
// One implementation under mk_list_tree, mk_struct_list_tree and
// mk_bytes_list_tree; what differs between the kinds is a TreeKind, defined
// next to the kind's dev_build / dev_update.
struct TreeHandle;
struct TreeKind {
    const char* name;      // "list tree"
    const char* noun;      // "items"
    uint64_t rebuild_div;  // rebuild instead of climbing when count / rebuild_div <= dirty
    bool level0;           // a 32-B entry per item (struct root, element digest) under the levels
    int (*check_shape)(uint64_t n, uint64_t capacity, uint32_t item_len);
    uint64_t (*build_ws)(const TreeHandle& t, uint64_t n);   // workspace of dev_build of n items
    uint64_t (*update_ws)(const TreeHandle& t, uint64_t k);  // ... of dev_update of k work items
    int (*check_values)(const TreeHandle& t, const uint8_t* values, uint64_t n);  // host check; null: none
    // every level and the root of the n items in t.items; the climb from the changed items
    int (*dev_build)(const TreeHandle& t, uint64_t n, hipStream_t st);
    int (*dev_update)(const TreeHandle& t, uint64_t n_old, uint64_t n_new, const uint64_t* d_idx, uint64_t k_idx,
                      const void* d_values, hipStream_t st);
    uint32_t id;                                                  // MK_TREE_LIST / _STRUCT / _BYTES
    TreeHandle* (*make_like)(const TreeHandle& t);                // an empty handle of t's type and layout (null: no memory)
    bool (*same_layout)(const TreeHandle& a, const TreeHandle& b);  // two handles of this kind: the same record layout
};
struct TreeHandle {
    const TreeKind* kind = nullptr;
    std::mutex mu;
    int dev = 0;
    uint32_t item_len = 0;
    uint64_t cap = 0, count = 0;  // items
    DevBuf items, level0, levels, root, idx, vals, ws;
    virtual ~TreeHandle() = default;  // a kind may add state of its own (the struct kind's layout)
};
// mk_*_new after the kind's argument checks and bind_call(): takes t (null: its allocation failed), frees it on failure
int tree_new(TreeHandle* t, const TreeKind& kind, uint32_t item_len, uint64_t capacity);
void tree_free(TreeHandle* t);
int tree_assign(TreeHandle* t, const uint8_t* values, uint64_t n);
int tree_update(TreeHandle* t, const uint64_t* idx, const uint8_t* values, uint64_t k);
int tree_append(TreeHandle* t, const uint8_t* values, uint64_t k);
// shrink: the first n values stay / the values at idx (any order, repeats count once) leave
int tree_truncate(TreeHandle* t, uint64_t n);
int tree_erase(TreeHandle* t, const uint64_t* idx, uint64_t k);
int tree_root(TreeHandle* t, uint8_t* root);
int tree_read(TreeHandle* t, uint64_t first, uint64_t cnt, uint8_t* out);
// Merkle proofs of the k values at idx (any order, repeats allowed): the k level-0 values
// (items, struct roots, element digests) and the k records; one upload, one launch, one read-back
int tree_branches(TreeHandle* t, const uint64_t* idx, uint64_t k, uint8_t* values_out, uint8_t* branches_out);
// Clone, copy and reserve: a tree moved between the layouts of two capacities by the copy
// launch (tree_copy_api.cpp); nothing is hashed.  tree_clone: a new handle like src holding its list;
// tree_copy: dst becomes a copy of src (the same kind, item length, layout and device, else MK_EINVAL);
// tree_reserve: room for `capacity` values.
int tree_clone(TreeHandle* src, TreeHandle** out);
int tree_copy(TreeHandle* dst, TreeHandle* src);
int tree_reserve(TreeHandle* t, uint64_t capacity);
// The pieces of those, for a set that moves all its trees in one launch (tree_set_api.cpp).  The caller
// holds the locks and has the device bound.
struct TreeBufs {  // what of a tree depends on its capacity, and optionally a root
    DevBuf items, level0, levels, root;
};
bool tree_same_shape(const TreeHandle& a, const TreeHandle& b);  // kind, item length, record layout
int tree_bufs_alloc(const TreeHandle& like, uint64_t cap, bool with_root, TreeBufs& b);  // frees what it got on failure
void tree_bufs_free(TreeBufs& b);
void tree_bufs_install(TreeHandle* t, TreeBufs& b, uint64_t cap);  // t's old buffers are freed (after a synchronise)
// a handle like src (buffers of src's capacity and a root, nothing built: the copy writes every live byte), count 0
int tree_new_like(const TreeHandle& src, TreeHandle** out);
// src's live part into dst's buffers, or into nb (of dst_cap values, dst's root where nb has none)
mk_tree_copy tree_copy_desc(const TreeHandle& src, const TreeHandle& dst, const TreeBufs* nb, uint64_t dst_cap);
// each kind's TreeKind and an empty handle of its type for tree_new (null: the allocation failed)
const TreeKind& list_tree_kind();
const TreeKind& struct_tree_kind();
const TreeKind& bytes_tree_kind();
TreeHandle* list_tree_handle();
TreeHandle* struct_tree_handle(const StructTreeLayout& L);
TreeHandle* bytes_tree_handle();
// A tree of a set (tree_set_api.cpp) that does not climb at a flush: room for
// new_cap items (>= t->cap; larger: the items moved), the staged values
// (device: k_idx ascending indices, k_idx + n_new - n_old values) written
// through, then the build of n_new items.  Enqueues on st under the caller's
// lock with the device bound; t->count is the caller's to set.
int tree_write_through_build(TreeHandle* t, uint64_t n_old, uint64_t n_new, uint64_t new_cap, const uint64_t* d_idx,
                             uint64_t k_idx, const void* d_values, hipStream_t st);

// ---- shrinking a resident tree (list_tree_api.cpp) ------------------------------
// What each kind's erase entry point and the handles run.  k_rm strictly
// ascending removed indices (device) leave n_new = n_old - k_rm values, those
// below `first` where they were; k_rm == 0: the first n_new <= n_old values
// stay (a truncate).  moved = n_new - first values (0 for a truncate) and
// their level-0 entries go through the workspace.
uint64_t tree_shrink_ws(const TreeKind& K, uint64_t moved, uint32_t item_len);  // 0: item_len == 0 or moved >= 2^31
int tree_shrink_check(const TreeKind& K, uint64_t n_old, uint64_t n_new, uint64_t capacity, uint32_t item_len,
                      uint64_t k_rm, uint64_t first, uint64_t ws_bytes);  // no device needed
int tree_shrink(const TreeKind& K, void* d_items, uint32_t item_len, void* d_level0, void* d_levels, uint64_t n_old,
                uint64_t n_new, uint64_t capacity, const uint64_t* d_rm, uint64_t k_rm, uint64_t first,
                void* d_root32, void* d_ws, hipStream_t st);

// ---- Merkle proofs of a resident tree (tree_branch_api.cpp) --------------------
// mk_dev_ssz_list_tree_branches: every argument check (no device needed), then the one launch on st
int list_branches_check(const void* d_level0, uint64_t n, uint64_t capacity, uint32_t item_len, const void* d_levels,
                        const uint64_t* d_idx, uint64_t k, const void* d_branches);
int list_branches_launch(const void* d_level0, uint64_t n, uint64_t capacity, uint32_t item_len, const void* d_levels,
                         const uint64_t* d_idx, uint64_t k, void* d_branches, hipStream_t st);

// ---- resident trees copied on the device (tree_copy_api.cpp) ----------------------
// mk_dev_ssz_trees_copy: every argument check (no device needed), then the one launch on st
int trees_copy_check(const mk_tree_copy* trees, uint32_t ntrees, const void* d_src_extra32, const void* d_dst_extra32);
int trees_copy_launch(const mk_tree_copy* trees, uint32_t ntrees, const void* d_src_extra32, void* d_dst_extra32,
                      hipStream_t st);

// ---- the audit of resident trees (tree_audit_api.cpp) ----------------------------
// mk_dev_ssz_trees_audit in three steps, shared with the handles: trees_audit_prepare checks every tree's own
// arguments and parses the record layouts (layouts, when given, holds a parsed layout per tree or null and is
// taken instead of the tree's `fields`), trees_audit_check the rest of the call (no device needed for either),
// trees_audit_launch enqueues the chain on st.
struct AuditCall {
    std::vector<StructTreeLayout> own;           // the layouts parsed here
    const StructTreeLayout* L[MK_TREES_MAX] = {};  // tree i's (STRUCT), else null
    uint64_t ws = 0;                             // workspace bytes
    uint64_t items = 0;                          // work items of the call: nodes, roots, level-0 entries, container
};
int trees_audit_prepare(const mk_tree_audit* trees, uint32_t ntrees, const StructTreeLayout* const* layouts,
                        uint32_t container_len, AuditCall& c);
int trees_audit_check(const mk_tree_audit* trees, uint32_t ntrees, const AuditCall& c, const void* d_container,
                      uint32_t container_len, const void* d_container_root32, const void* d_reports, const void* d_ws,
                      uint64_t ws_bytes);
int trees_audit_launch(const mk_tree_audit* trees, uint32_t ntrees, const AuditCall& c, const void* d_container,
                       uint32_t container_len, const void* d_container_root32, void* d_reports, void* d_ws,
                       hipStream_t st);
// a handle's tree as the audit takes it, and the parsed layout of a registry tree's handle (struct_tree_api.cpp)
mk_tree_audit tree_audit_desc(const TreeHandle& t, uint32_t container_off);
const StructTreeLayout* struct_tree_layout_of(const TreeHandle& t);
// one tree's audit: one chain, one read-back
int tree_audit(TreeHandle* t, mk_audit_report* out);

// ---- the diff of resident trees (tree_diff_api.cpp) ------------------------------
// mk_dev_ssz_trees_diff: every argument check (no device needed), then the reports cleared and the one launch on st
int trees_diff_check(const mk_tree_diff* trees, uint32_t ntrees, const void* d_reports);
int trees_diff_launch(const mk_tree_diff* trees, uint32_t ntrees, void* d_reports, hipStream_t st);
// the pair (a, b) of two handles as the diff takes it (the caller holds both locks)
mk_tree_diff tree_diff_desc(const TreeHandle& a, const TreeHandle& b, uint64_t* d_idx_out, uint64_t max_out);
// the first min(total, max_out) of the max_out slots read back, ascending
void tree_diff_sort(uint64_t* slots, uint64_t total, uint64_t max_out);
// two handles' diff: one launch, one read-back
int tree_diff(TreeHandle* a, TreeHandle* b, uint64_t* idx_out, uint64_t max_out, uint64_t* total, uint64_t* n_a,
              uint64_t* n_b);

// ---- several trees in one call (tree_many_api.cpp) ------------------------------------------
// mk_ssz_trees_update_workspace_bytes with its error, and mk_dev_ssz_trees_update
// after bind_stream(): every check, then the launches on st
int trees_update_workspace(const mk_tree_update* trees, uint32_t ntrees, uint64_t* bytes);
int trees_update(const mk_tree_update* trees, uint32_t ntrees, void* d_container, uint32_t container_len,
                 void* d_container_root32, void* d_ws, uint64_t ws_bytes, hipStream_t st);
// every argument rule of mk_dev_ssz_trees_update but the workspace's size, for the calls that take the same
// array (tree_journal_api.cpp); d_ws16: any 16-B aligned pointer of the caller's; lists == false: the index
// arrays and the staged values are not looked at.  No device needed.
int trees_update_check(const mk_tree_update* trees, uint32_t ntrees, const void* d_container, uint32_t container_len,
                       const void* d_container_root32, const void* d_ws16, bool lists);
// ---- the undo journal of resident trees (tree_journal_api.cpp) ---------------------
// mk_ssz_trees_journal_bytes with its error; mk_dev_ssz_trees_journal / _restore after bind_stream(): every
// check, then the one launch on st
int trees_journal_bytes(const mk_tree_update* trees, uint32_t ntrees, uint32_t container_len, uint64_t* bytes);
int trees_journal(bool restore, const mk_tree_update* trees, uint32_t ntrees, void* d_container, uint32_t container_len,
                  void* d_container_root32, void* d_journal, uint64_t journal_bytes, hipStream_t st);
int struct_tree_stage0_roots(const StructTreeLayout& L, const void* d_records, uint64_t n_new, uint64_t T,
                             const void* d_values, void* d_roots, void* d_scratch, const void** d_new_roots,
                             hipStream_t st);

// ---- multi-device (multi_api.cpp) ------------------------------------------------
int host_merkle_multi(const uint8_t* items, uint64_t n, uint32_t item_len, int nshards, const int* devs_in,
                      uint8_t* out, uint32_t elem_len = 0);

}  // namespace mk::rt
