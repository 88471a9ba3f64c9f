// A set of device-resident trees behind one host handle (mk_tree_set,
// DESIGN.md §5j): up to MK_TREES_MAX trees of the three kinds, each one a
// TreeHandle (tree_handle.cpp), and the hash message of the struct that holds
// them.  Changes are collected on the host (tree_set_plan.cpp); a root is one
// upload, the update over all the trees (tree_many_api.cpp) and one 32-B
// read-back.
#include <functional>

#include "runtime.hpp"
#include "tree_set_plan.hpp"

using namespace mk;
using namespace mk::rt;
namespace sp = mk::setplan;

struct mk_tree_set {
    struct Tree {
        TreeHandle* h = nullptr;
        uint32_t kind = 0, coff = MK_NO_CONTAINER;
        std::vector<mk_field> fields;  // STRUCT
    };
    std::mutex mu;
    int dev = -1;  // the call's device of mk_tree_set_new; -1: the device current when the first tree is added
    uint32_t container_len = 0;
    std::vector<uint8_t> msg;  // the struct's hash message: what put() wrote, zeros elsewhere
    std::vector<Tree> trees;
    std::vector<sp::Pending> pend;  // trees[i]'s
    bool dirty = false;             // something changed since the last flush
    sp::SetPlan plan;               // of the flush in flight
    void* host = nullptr;           // pinned staging: the message, then every tree's indices and values
    size_t host_cap = 0;
    DevBuf stage, ws, croot;  // the staging buffer in HBM (the message at its front), workspace, container root
    // ---- checkpoints ----
    // One record per flush made while a checkpoint is open (and per assign / truncate / erase): the journal of
    // the flush's update (mk_dev_ssz_trees_journal over the flush's own array, no container: a roll back ends
    // with a flush that brings the message and its root up to date), and a full copy of every tree that did
    // not climb -- a handle of its own, taken before the change by the copy launch.
    struct Record {
        bool climbed = false;            // a journal at [off, off + bytes) of `journal`
        uint64_t off = 0, bytes = 0;
        uint32_t nt = 0;
        uint64_t n_old[MK_TREES_MAX] = {}, n_new[MK_TREES_MAX] = {}, k_idx[MK_TREES_MAX] = {};
        std::vector<std::pair<uint32_t, TreeHandle*>> full;  // (tree, what it was)
    };
    struct Checkpoint {
        uint64_t id = 0;
        size_t first_record = 0;       // the records made since
        uint64_t used = 0;             // the journal's fill when it was opened
        std::vector<uint64_t> counts;  // every tree's
        std::vector<uint8_t> msg;      // the host message
    };
    std::vector<Checkpoint> cps;  // the open ones, ids ascending
    std::vector<Record> records;
    Record next;           // of the flush in flight: counts only after its synchronise (flushed)
    uint64_t next_id = 1;
    DevBuf journal;
    uint64_t used = 0, base = 0;  // records live in [base, used)
};

namespace {

uint32_t nparts(const mk_tree_set* s) {
    uint32_t n = 0;
    for (const auto& t : s->trees) n += t.coff != MK_NO_CONTAINER;
    return n;
}

int check_tree(const mk_tree_set* s, uint32_t tree) {
    if (tree >= s->trees.size()) return fail(MK_EINVAL, "tree %u of a set of %zu", tree, s->trees.size());
    return MK_OK;
}

// the set's device bound for this call (decided by the first call that needs one)
int bind_set(mk_tree_set* s) {
    if (s->dev >= 0) return bind_dev(s->dev);
    TRY(bind_call());
    s->dev = t_bound;
    return MK_OK;
}

// the part of a tree's mk_tree_update that is the tree itself
void tree_desc(const mk_tree_set::Tree& t, mk_tree_update& u) {
    u.kind = t.kind;
    u.item_len = t.h->item_len;
    u.d_items = t.h->items.p;
    u.d_level0 = t.h->level0.p;
    u.d_levels = t.h->levels.p;
    u.capacity = t.h->cap;
    u.fields = t.fields.empty() ? nullptr : t.fields.data();
    u.nfields = (uint32_t)t.fields.size();
    u.container_off = t.coff;
    u.d_root32 = t.h->root.p;
}

void drop_record(mk_tree_set::Record& r) {
    for (auto& f : r.full) tree_free(f.second);
    r = mk_tree_set::Record();
}

// tree i as it is now, kept in record r (once: a flush that is tried again keeps the first copy)
int full_record(mk_tree_set* s, uint32_t i, mk_tree_set::Record& r) {
    for (const auto& f : r.full)
        if (f.first == i) return MK_OK;
    TreeHandle* c = nullptr;
    TRY(tree_clone(s->trees[i].h, &c));
    r.full.emplace_back(i, c);
    return MK_OK;
}

// An immediate change of tree i (assign, truncate, erase) under an open
// checkpoint: its full record is a record of its own, filed when the change
// succeeded -- the record of a flush in flight (s->next) is not touched.  A
// flush that failed before may have left the tree half written and kept the
// copy it took first: that copy is what the tree was, so it moves here.
int immediate_begin(mk_tree_set* s, uint32_t i, mk_tree_set::Record& r) {
    if (s->cps.empty()) return MK_OK;
    for (size_t f = 0; f < s->next.full.size(); ++f)
        if (s->next.full[f].first == i) {
            r.full.push_back(s->next.full[f]);
            s->next.full.erase(s->next.full.begin() + f);
            return MK_OK;
        }
    TRY(bind_set(s));
    return full_record(s, i, r);
}
void immediate_end(mk_tree_set* s, mk_tree_set::Record& r, int rc) {
    if (r.full.empty()) return;
    if (rc)
        drop_record(r);
    else
        s->records.push_back(std::move(r));
}

// the record in flight counts
void commit_record(mk_tree_set* s) {
    if (!s->next.climbed && s->next.full.empty()) return;
    if (s->next.climbed) s->used = s->next.off + s->next.bytes;
    s->records.push_back(std::move(s->next));
    s->next = mk_tree_set::Record();
}

// Room for `need` more bytes behind `used`.  The front that release() freed,
// [0, base), is taken back first: the live part [base, used) moves to offset 0
// (through a new buffer, so the two ranges never overlap) and every record's
// offset and every checkpoint's fill move with it.  The buffer is only made
// larger -- by doubling -- when the live part plus `need` does not fit, so a
// ring of checkpoints whose oldest is released every slot holds a journal of
// about twice its live records, however many slots went through it.
int journal_room(mk_tree_set* s, uint64_t need) {
    if (s->journal.cap >= s->used + need) return MK_OK;
    const uint64_t live = s->used - s->base;
    size_t cap = std::max<size_t>(s->journal.cap, (size_t)64 << 10);
    while (cap < live + need) cap *= 2;
    void* p = nullptr;
    if (hipMalloc(&p, cap) != hipSuccess) return fail(MK_ENOMEM, "hipMalloc(%zu) failed", cap);
    hipStream_t st = ctx()->stream;
    if ((live && hipMemcpyAsync(p, (uint8_t*)s->journal.p + s->base, live, hipMemcpyDeviceToDevice, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess) {  // also: nothing enqueued still reads the old buffer
        (void)hipFree(p);
        return fail(MK_EHIP, "moving the journal failed");
    }
    if (s->journal.p) (void)hipFree(s->journal.p);
    s->journal.p = p;
    s->journal.cap = cap;
    for (auto& r : s->records)
        if (r.climbed) r.off -= s->base;
    for (auto& c : s->cps) c.used -= s->base;
    s->used = live;
    s->base = 0;
    return MK_OK;
}

// Everything pending onto the device and every root brought up to date,
// enqueued on the context's stream; the caller adds its read-back,
// synchronises and calls flushed().  Nothing to do when nothing changed.
// While a checkpoint is open (and journaling is not switched off: the flush
// that ends a roll back) the flush writes a record: a full copy of every tree
// that does not climb before it is built, and the journal launch between the
// upload and the update.
int flush(mk_tree_set* s, bool journaling = true) {
    if (!s->dirty || s->trees.empty()) return MK_OK;
    const bool jr = journaling && !s->cps.empty();
    const uint32_t nt = (uint32_t)s->trees.size();
    hipStream_t st = ctx()->stream;
    for (uint32_t i = 0; i < nt; ++i) s->pend[i].cap = s->trees[i].h->cap;
    sp::make_plan(s->pend.data(), nt, (s->container_len + 15) & ~15u, s->plan);
    const sp::SetPlan& P = s->plan;
    if (s->host_cap < P.bytes) {
        if (s->host) (void)hipHostFree(s->host);
        s->host = nullptr;
        s->host_cap = 0;
        const size_t cap = std::max<size_t>(2 * P.bytes, 64 << 10);
        if (hipHostMalloc(&s->host, cap, hipHostMallocDefault) != hipSuccess)
            return fail(MK_ENOMEM, "hipHostMalloc(%zu) failed", cap);
        s->host_cap = cap;
    }
    TRY(grow(s->stage, std::max<size_t>(s->host_cap, 16)));
    TRY(grow(s->croot, 32));
    uint8_t* host = (uint8_t*)s->host;
    uint8_t* stage = (uint8_t*)s->stage.p;
    if (s->container_len) std::memcpy(host, s->msg.data(), s->container_len);
    sp::pack(s->pend.data(), nt, P, host);
    if (P.bytes) HIPCHK(hipMemcpyAsync(stage, host, P.bytes, hipMemcpyHostToDevice, st));
    mk_tree_update table[MK_TREES_MAX] = {};
    for (uint32_t i = 0; i < nt; ++i) {
        const mk_tree_set::Tree& t = s->trees[i];
        const sp::TreePlan& p = P.tree[i];
        const uint64_t* d_idx = (const uint64_t*)(stage + p.idx_off);
        const uint8_t* d_vals = stage + p.val_off;
        const uint64_t T = p.k_idx + (p.n_new - p.n_old);
        mk_tree_update& u = table[i];
        u.n_old = p.n_old;
        u.n_new = p.n_new;
        if (p.action != sp::kClimb) {  // built here: enters the update with nothing dirty
            if (jr) TRY(full_record(s, i, s->next));
            TRY(tree_write_through_build(t.h, p.n_old, p.n_new, p.new_cap, d_idx, p.k_idx, d_vals, st));
            u.n_old = p.n_new;
        } else if (T) {
            u.d_idx = p.k_idx ? d_idx : nullptr;
            u.k_idx = p.k_idx;
            u.d_values = d_vals;
        }
        tree_desc(t, u);
    }
    if (jr) {
        mk_tree_set::Record& r = s->next;
        uint64_t bytes = 0;
        mk_tree_update jt[MK_TREES_MAX];  // the same array without the container
        for (uint32_t i = 0; i < nt; ++i) jt[i] = table[i], jt[i].container_off = MK_NO_CONTAINER;
        TRY(trees_journal_bytes(jt, nt, 0, &bytes));
        TRY(journal_room(s, bytes));
        TRY(trees_journal(false, jt, nt, nullptr, 0, nullptr, (uint8_t*)s->journal.p + s->used, bytes, st));
        r.climbed = true;
        r.off = s->used;
        r.bytes = bytes;
        r.nt = nt;
        for (uint32_t i = 0; i < nt; ++i) r.n_old[i] = table[i].n_old, r.n_new[i] = table[i].n_new, r.k_idx[i] = table[i].k_idx;
    }
    const uint32_t clen = nparts(s) ? s->container_len : 0;
    uint64_t need = 0;
    TRY(trees_update_workspace(table, nt, &need));
    TRY(grow(s->ws, need));
    return trees_update(table, nt, clen ? stage : nullptr, clen, clen ? s->croot.p : nullptr, s->ws.p, s->ws.cap, st);
}

// after the synchronise that followed flush(): the pending changes are the trees' content
void flushed(mk_tree_set* s) {
    if (!s->dirty || s->trees.empty()) return;
    for (size_t i = 0; i < s->trees.size(); ++i) {
        sp::commit(s->pend[i], s->plan.tree[i]);
        s->pend[i].cap = s->trees[i].h->cap;
        s->trees[i].h->count = s->pend[i].n;
    }
    s->dirty = false;
    commit_record(s);
}

// flush, 32 bytes at d_src (looked up after the flush: a grown tree moved) to the host, one synchronise
template <class Src>
int flush_read32(mk_tree_set* s, const Src& d_src, uint8_t* out) {
    TRY(bind_set(s));
    TRY(flush(s));
    hipStream_t st = ctx()->stream;
    HIPCHK(hipMemcpyAsync(out, d_src(), 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    flushed(s);
    return MK_OK;
}

int set_add(mk_tree_set* s, uint32_t kind, uint32_t item_len, const mk_field* fields, uint32_t nfields,
            uint64_t capacity, uint32_t container_off, uint32_t* tree) {
    if (!s || !tree) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->trees.size() >= MK_TREES_MAX) return fail(MK_EINVAL, "a set holds at most %d trees", MK_TREES_MAX);
    if (!s->cps.empty()) return fail(MK_EINVAL, "a tree added while %zu checkpoints are open", s->cps.size());
    const TreeKind* K = nullptr;
    StructTreeLayout L;
    if (kind == MK_TREE_LIST || kind == MK_TREE_BYTES) {
        if (fields || nfields) return fail(MK_EINVAL, "a field layout for a tree of kind %u", kind);
        K = kind == MK_TREE_LIST ? &list_tree_kind() : &bytes_tree_kind();
    } else if (kind == MK_TREE_STRUCT) {
        if (!fields || !nfields) return fail(MK_EINVAL, "a struct tree without its field layout");
        TRY(struct_tree_layout(fields, nfields, item_len, L));
        K = &struct_tree_kind();
    } else {
        return fail(MK_EINVAL, "unknown kind %u", kind);
    }
    TRY(K->check_shape(0, std::max<uint64_t>(capacity, 1), item_len));
    if (container_off != MK_NO_CONTAINER) {
        if (container_off % 4) return fail(MK_EINVAL, "container offset %u not 4-byte aligned", container_off);
        if ((uint64_t)container_off + 32 > s->container_len)
            return fail(MK_EINVAL, "root at offset %u beyond the %u-byte container", container_off, s->container_len);
        for (size_t j = 0; j < s->trees.size(); ++j) {
            const uint32_t o = s->trees[j].coff;
            if (o != MK_NO_CONTAINER && container_off < o + 32 && o < container_off + 32)
                return fail(MK_EINVAL, "the root overlaps tree %zu's in the container", j);
        }
    }
    TRY(bind_set(s));
    TreeHandle* h = kind == MK_TREE_LIST    ? list_tree_handle()
                    : kind == MK_TREE_BYTES ? bytes_tree_handle()
                                            : struct_tree_handle(L);
    TRY(tree_new(h, *K, item_len, capacity));  // frees h on failure
    mk_tree_set::Tree t;
    t.h = h;
    t.kind = kind;
    t.coff = container_off;
    if (fields) t.fields.assign(fields, fields + nfields);
    sp::Pending p;
    p.item_len = item_len;
    p.rebuild_div = K->rebuild_div;
    p.cap = h->cap;
    s->trees.push_back(std::move(t));
    s->pend.push_back(std::move(p));
    s->dirty = true;  // its root is not in the message yet
    *tree = (uint32_t)s->trees.size() - 1;
    return MK_OK;
}

int set_put(mk_tree_set* s, uint32_t off, const uint8_t* bytes, uint32_t len) {
    if (!s || (len && !bytes)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    if ((uint64_t)off + len > s->container_len)
        return fail(MK_EINVAL, "[%u, +%u) leaves the %u-byte container", off, len, s->container_len);
    for (size_t j = 0; len && j < s->trees.size(); ++j) {
        const uint32_t o = s->trees[j].coff;
        if (o != MK_NO_CONTAINER && off < o + 32 && o < (uint64_t)off + len)
            return fail(MK_EINVAL, "[%u, +%u) touches tree %zu's root at %u", off, len, j, o);
    }
    if (len) std::memcpy(s->msg.data() + off, bytes, len);
    s->dirty = true;
    return MK_OK;
}

int set_assign(mk_tree_set* s, uint32_t tree, const uint8_t* values, uint64_t n) {
    if (!s) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    TreeHandle* h = s->trees[tree].h;
    mk_tree_set::Record rec;  // a full record: what the tree was
    TRY(immediate_begin(s, tree, rec));
    const int rc = tree_assign(h, values, n);
    immediate_end(s, rec, rc);
    if (rc) return rc;
    sp::record_assign(s->pend[tree], n, h->cap);
    s->dirty = true;
    return MK_OK;
}

int set_update(mk_tree_set* s, uint32_t tree, const uint64_t* idx, const uint8_t* values, uint64_t k) {
    if (!s || (k && (!idx || !values))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    const TreeHandle* h = s->trees[tree].h;
    sp::Pending& p = s->pend[tree];
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= p.count())
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[i],
                        (unsigned long long)p.count(), h->kind->noun);
    if (k == 0) return MK_OK;
    if (h->kind->check_values) TRY(h->kind->check_values(*h, values, k));
    (void)sp::record_update(p, idx, values, k);
    s->dirty = true;
    return MK_OK;
}

int set_append(mk_tree_set* s, uint32_t tree, const uint8_t* values, uint64_t k) {
    if (!s || (k && !values)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    const TreeHandle* h = s->trees[tree].h;
    sp::Pending& p = s->pend[tree];
    if (k == 0) return MK_OK;
    if (k >= kMaxWork || p.count() + k < k)
        return fail(MK_EINVAL, "%llu %s in one append", (unsigned long long)k, h->kind->noun);
    if (h->kind->check_values) TRY(h->kind->check_values(*h, values, k));
    sp::record_append(p, values, k);
    s->dirty = true;
    return MK_OK;
}

// A shrink is not logged: everything pending is flushed (the
// ordinary flush), then the tree shrinks at once; it enters the next flush
// with nothing dirty, and the update over all the trees stores its new root
// into the message as it does for every tree.  erase: the k values at idx leave; else: truncate to n.
// A failed shrink leaves the set as the flush left it.
int set_shrink(mk_tree_set* s, uint32_t tree, bool erase, const uint64_t* idx, uint64_t k, uint64_t n) {
    if (!s || (erase && k && !idx)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    TreeHandle* h = s->trees[tree].h;
    sp::Pending& p = s->pend[tree];
    const uint64_t count = p.count();
    if (!erase && n > count)
        return fail(MK_EINVAL, "truncate to %llu of %llu %s", (unsigned long long)n, (unsigned long long)count,
                    h->kind->noun);
    for (uint64_t i = 0; erase && i < k; ++i)
        if (idx[i] >= count)
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[i], (unsigned long long)count,
                        h->kind->noun);
    if (erase ? k == 0 : n == count) return MK_OK;
    if (s->dirty) {
        TRY(bind_set(s));
        TRY(flush(s));
        HIPCHK(hipStreamSynchronize(ctx()->stream));
        flushed(s);
    }
    mk_tree_set::Record rec;  // a full record: what the tree was
    TRY(immediate_begin(s, tree, rec));
    const int rc = erase ? tree_erase(h, idx, k) : tree_truncate(h, n);
    immediate_end(s, rec, rc);
    if (rc) return rc;
    sp::record_assign(p, h->count, h->cap);
    s->dirty = true;  // its root in the message is the old one
    return MK_OK;
}

int set_root(mk_tree_set* s, uint8_t* root) {
    if (!s || !root) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->container_len == 0) return fail(MK_EINVAL, "a set without a container has no root");
    if (nparts(s) == 0) return fail(MK_EINVAL, "a container no tree takes part in");
    return flush_read32(s, [&] { return (const void*)s->croot.p; }, root);
}

int set_tree_root(mk_tree_set* s, uint32_t tree, uint8_t* root) {
    if (!s || !root) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    return flush_read32(s, [&] { return (const void*)s->trees[tree].h->root.p; }, root);
}

int set_items(mk_tree_set* s, uint32_t tree, uint64_t first, uint64_t cnt, uint8_t* out) {
    if (!s || (cnt && !out)) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    const sp::Pending& p = s->pend[tree];
    if (first > p.count() || cnt > p.count() - first)
        return fail(MK_EINVAL, "[%llu, +%llu) beyond %llu %s", (unsigned long long)first, (unsigned long long)cnt,
                    (unsigned long long)p.count(), s->trees[tree].h->kind->noun);
    if (s->dirty) {
        TRY(bind_set(s));
        TRY(flush(s));
        HIPCHK(hipStreamSynchronize(ctx()->stream));
        flushed(s);
    }
    return tree_read(s->trees[tree].h, first, cnt, out);
}

// Proofs out of one tree of the set: everything pending is
// flushed as for a root, then the tree's own launch and read-back, then the
// message as the device holds it, every tree's root in place -- what a
// verifier hashes with the proven list's root substituted.  No tree takes part
// in the container: the message is what put() wrote.
int set_branches(mk_tree_set* s, uint32_t tree, const uint64_t* idx, uint64_t k, uint8_t* values_out,
                 uint8_t* branches_out, uint8_t* container_out) {
    if (!s || (k && (!idx || !values_out || !branches_out))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    TreeHandle* h = s->trees[tree].h;
    const uint64_t count = s->pend[tree].count();
    for (uint64_t i = 0; i < k; ++i)
        if (idx[i] >= count)
            return fail(MK_EINVAL, "index %llu beyond %llu %s", (unsigned long long)idx[i], (unsigned long long)count,
                        h->kind->noun);
    if (k >= kMaxWork) return fail(MK_EINVAL, "%llu proofs in one call (limit 2^31 - 1)", (unsigned long long)k);
    const bool want_msg = container_out && s->container_len;
    if (k == 0 && !want_msg) return MK_OK;
    TRY(bind_set(s));
    if (s->dirty) {
        TRY(flush(s));
        HIPCHK(hipStreamSynchronize(ctx()->stream));
        flushed(s);
    }
    TRY(tree_branches(h, idx, k, values_out, branches_out));
    if (!want_msg) return MK_OK;
    if (nparts(s) == 0) {
        std::memcpy(container_out, s->msg.data(), s->container_len);
        return MK_OK;
    }
    hipStream_t st = ctx()->stream;
    HIPCHK(hipMemcpyAsync(container_out, s->stage.p, s->container_len, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// RepeatHash(reveal, layers) == commitment against the records of registry tree `tree`: what
// is pending goes to the device first, as for set_branches; then the handle's own verify.  Read-only.
int set_verify_repeat_hash(mk_tree_set* s, uint32_t tree, uint32_t commit_off, uint32_t layers_off,
                           const uint64_t* idx, const uint8_t* reveals, uint64_t m, uint32_t max_layers, uint8_t* ok) {
    if (!s || (m && (!idx || !reveals || !ok))) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    TreeHandle* h = s->trees[tree].h;
    if (s->trees[tree].kind != MK_TREE_STRUCT)
        return fail(MK_EINVAL, "tree %u is a %s: the verify takes a struct list tree", tree, h->kind->name);
    // against the pending count, before anything is flushed; the handle's verify checks the rest
    TRY(repeat_check_indices(idx, m, s->pend[tree].count(), h->kind->noun));
    TRY(repeat_check_offsets(h->item_len, commit_off, layers_off, "record length"));
    TRY(repeat_check_call(m, max_layers, MK_REPEAT_AUTO));
    if (m == 0) return MK_OK;
    TRY(bind_set(s));
    if (s->dirty) {
        TRY(flush(s));
        HIPCHK(hipStreamSynchronize(ctx()->stream));
        flushed(s);
    }
    return tree_verify_repeat_hash(h, commit_off, layers_off, idx, reveals, m, max_layers, ok);
}

// ---- clone, copy, reserve ---------------------------------------------------------
// everything pending onto the device and waited for: the handles hold what root() would describe
int settle(mk_tree_set* s) {
    if (!s->dirty || s->trees.empty()) return MK_OK;
    TRY(bind_set(s));
    TRY(flush(s));
    HIPCHK(hipStreamSynchronize(ctx()->stream));
    flushed(s);
    return MK_OK;
}

bool same_fields(const std::vector<mk_field>& a, const std::vector<mk_field>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(mk_field)));
}

// src (settled) into dst, whose trees are handles of src's shapes, tree by
// tree: every buffer a too-small destination tree needs first, then ONE copy
// launch over all the trees and the container root, the message as the device
// holds it (what mk_tree_set_branches hands out) behind it on the stream, one
// synchronise; then the host side.  Both sets locked, their device bound.
int copy_trees(mk_tree_set* dst, mk_tree_set* src) {
    const uint32_t nt = (uint32_t)src->trees.size();
    if (nt == 0) {
        dst->msg = src->msg;
        dst->dirty = false;
        return MK_OK;
    }
    hipStream_t st = ctx()->stream;
    std::vector<TreeBufs> nb(nt);
    mk_tree_copy table[MK_TREES_MAX] = {};
    const bool extra = src->container_len && nparts(src) && src->croot.p;
    int rc = MK_OK;
    for (uint32_t i = 0; i < nt && !rc; ++i) {  // a failed allocation leaves dst's trees as they were
        const TreeHandle& sh = *src->trees[i].h;
        const TreeHandle& dh = *dst->trees[i].h;
        const bool regrow = sh.count > dh.cap;
        if (regrow) rc = tree_bufs_alloc(sh, sh.cap, false, nb[i]);
        if (!rc) table[i] = tree_copy_desc(sh, dh, regrow ? &nb[i] : nullptr, regrow ? sh.cap : dh.cap);
    }
    if (!rc && extra) rc = grow(dst->croot, 32);
    if (!rc && extra) rc = grow(dst->stage, src->stage.cap);
    if (!rc) rc = trees_copy_check(table, nt, extra ? src->croot.p : nullptr, extra ? dst->croot.p : nullptr);
    if (!rc) rc = trees_copy_launch(table, nt, extra ? src->croot.p : nullptr, extra ? dst->croot.p : nullptr, st);
    if (!rc && extra &&
        hipMemcpyAsync(dst->stage.p, src->stage.p, src->container_len, hipMemcpyDeviceToDevice, st) != hipSuccess)
        rc = fail(MK_EHIP, "hipMemcpyAsync failed");
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(MK_EHIP, "hipStreamSynchronize failed");
    if (rc) {
        for (TreeBufs& b : nb) tree_bufs_free(b);
        dst->dirty = true;  // its message in HBM may be gone: the next flush writes it again
        return rc;
    }
    for (uint32_t i = 0; i < nt; ++i) {
        TreeHandle* dh = dst->trees[i].h;
        if (nb[i].items.p) tree_bufs_install(dh, nb[i], src->trees[i].h->cap);
        dh->count = src->trees[i].h->count;
        sp::record_assign(dst->pend[i], dh->count, dh->cap);  // its pending changes are dropped
    }
    dst->msg = src->msg;
    dst->dirty = false;
    return MK_OK;
}

// the two sets' mutexes, always the one at the lower address first (as tree_copy takes two handles')
struct LockBoth {
    std::mutex *a, *b;
    LockBoth(std::mutex& x, std::mutex& y) : a(&x), b(&y) {
        if (std::less<std::mutex*>()(b, a)) std::swap(a, b);
        a->lock();
        b->lock();
    }
    ~LockBoth() {
        b->unlock();
        a->unlock();
    }
};

int set_clone(mk_tree_set* src, mk_tree_set** out) {
    if (!src || !out) return fail(MK_EINVAL, "null pointer");
    *out = nullptr;
    std::lock_guard<std::mutex> lk(src->mu);
    TRY(settle(src));
    if (!src->trees.empty()) TRY(bind_set(src));
    auto* s = new (std::nothrow) mk_tree_set();
    if (!s) return fail(MK_ENOMEM, "tree set allocation failed");
    s->dev = src->dev;
    s->container_len = src->container_len;
    int rc = MK_OK;
    for (size_t i = 0; i < src->trees.size() && !rc; ++i) {
        const mk_tree_set::Tree& t = src->trees[i];
        mk_tree_set::Tree c;
        rc = tree_new_like(*t.h, &c.h);
        if (rc) break;
        c.kind = t.kind;
        c.coff = t.coff;
        c.fields = t.fields;
        sp::Pending p;
        p.item_len = t.h->item_len;
        p.rebuild_div = t.h->kind->rebuild_div;
        p.cap = c.h->cap;
        s->trees.push_back(std::move(c));
        s->pend.push_back(std::move(p));
    }
    if (!rc) rc = copy_trees(s, src);
    if (rc) {
        mk_tree_set_free(s);
        return rc;
    }
    *out = s;
    return MK_OK;
}

// what a copy and a diff ask of two sets (both locked): the same container length, device and, tree by tree,
// kind, item length, record layout and container offset
int sets_agree(const mk_tree_set* dst, const mk_tree_set* src) {
    if (dst->container_len != src->container_len)
        return fail(MK_EINVAL, "containers of %u and %u bytes", dst->container_len, src->container_len);
    if (dst->trees.size() != src->trees.size())
        return fail(MK_EINVAL, "sets of %zu and %zu trees", dst->trees.size(), src->trees.size());
    for (size_t i = 0; i < src->trees.size(); ++i) {
        const mk_tree_set::Tree &d = dst->trees[i], &t = src->trees[i];
        if (d.kind != t.kind || d.h->item_len != t.h->item_len || d.coff != t.coff || !same_fields(d.fields, t.fields))
            return fail(MK_EINVAL, "tree %zu differs in kind, item length, record layout or container offset", i);
    }
    if (!src->trees.empty() && dst->dev != src->dev)
        return fail(MK_EINVAL, "the sets live on devices %d and %d", dst->dev, src->dev);
    return MK_OK;
}

int set_copy(mk_tree_set* dst, mk_tree_set* src) {
    if (!dst || !src) return fail(MK_EINVAL, "null pointer");
    if (dst == src) return MK_OK;
    LockBoth lk(dst->mu, src->mu);
    TRY(sets_agree(dst, src));
    if (!dst->cps.empty())
        return fail(MK_EINVAL, "a copy into a set with %zu open checkpoints", dst->cps.size());
    TRY(settle(src));
    if (!src->trees.empty()) TRY(bind_set(src));
    return copy_trees(dst, src);
}

int set_reserve(mk_tree_set* s, uint32_t tree, uint64_t capacity) {
    if (!s) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    TRY(check_tree(s, tree));
    TRY(tree_reserve(s->trees[tree].h, capacity));  // what is pending stays pending
    s->pend[tree].cap = s->trees[tree].h->cap;
    return MK_OK;
}

// ---- checkpoints ------------------------------------------------------------------
int find_checkpoint(const mk_tree_set* s, uint64_t id, size_t* at) {
    for (size_t i = 0; i < s->cps.size(); ++i)
        if (s->cps[i].id == id) {
            *at = i;
            return MK_OK;
        }
    return fail(MK_EINVAL, "checkpoint %llu is not open", (unsigned long long)id);
}

int set_checkpoint(mk_tree_set* s, uint64_t* id) {
    if (!s || !id) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->cps.size() >= MK_CHECKPOINTS_MAX)
        return fail(MK_EINVAL, "%d checkpoints are open already", MK_CHECKPOINTS_MAX);
    TRY(settle(s));  // journaled when a checkpoint is open already
    mk_tree_set::Checkpoint c;
    c.id = s->next_id++;
    c.first_record = s->records.size();
    c.used = s->used;
    for (const auto& t : s->trees) c.counts.push_back(t.h->count);
    c.msg = s->msg;
    s->cps.push_back(std::move(c));
    *id = s->cps.back().id;
    return MK_OK;
}

// Undoes every record made since checkpoint id, newest first: a record's
// journal restored (mk_dev_ssz_trees_restore over the trees as they are now --
// a tree keeps the capacity it grew to), then its full copies home.  Then the
// counts and the message of the checkpoint, and one unjournaled flush with
// nothing dirty, which brings every tree's root into the message and the
// message's root up to date, with the call's synchronise.
int set_rollback(mk_tree_set* s, uint64_t id) {
    if (!s) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    size_t at = 0;
    TRY(find_checkpoint(s, id, &at));
    const uint32_t nt = (uint32_t)s->trees.size();
    if (nt) TRY(bind_set(s));
    drop_record(s->next);
    const mk_tree_set::Checkpoint& c = s->cps[at];
    for (size_t r = s->records.size(); r > c.first_record; --r) {
        mk_tree_set::Record& R = s->records[r - 1];
        if (R.climbed) {
            mk_tree_update table[MK_TREES_MAX] = {};
            for (uint32_t i = 0; i < R.nt; ++i) {
                tree_desc(s->trees[i], table[i]);
                table[i].n_old = R.n_old[i], table[i].n_new = R.n_new[i], table[i].k_idx = R.k_idx[i];
                table[i].container_off = MK_NO_CONTAINER;
            }
            TRY(trees_journal(true, table, R.nt, nullptr, 0, nullptr, (uint8_t*)s->journal.p + R.off, R.bytes,
                              ctx()->stream));
        }
        for (size_t f = R.full.size(); f > 0; --f) TRY(tree_copy(s->trees[R.full[f - 1].first].h, R.full[f - 1].second));
    }
    for (size_t r = c.first_record; r < s->records.size(); ++r) drop_record(s->records[r]);
    s->records.resize(c.first_record);
    s->used = c.used;
    for (uint32_t i = 0; i < nt; ++i) {
        TreeHandle* h = s->trees[i].h;
        h->count = c.counts[i];
        sp::record_assign(s->pend[i], h->count, h->cap);  // the pending changes are dropped
    }
    s->msg = c.msg;
    s->cps.resize(at);
    if (s->cps.empty()) s->used = s->base = 0;
    s->dirty = true;
    if (nt) {
        TRY(flush(s, false));
        HIPCHK(hipStreamSynchronize(ctx()->stream));
        flushed(s);
    }
    return MK_OK;
}

int set_release(mk_tree_set* s, uint64_t id) {
    if (!s) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    size_t at = 0;
    TRY(find_checkpoint(s, id, &at));
    s->cps.erase(s->cps.begin(), s->cps.begin() + at + 1);
    const size_t gone = s->cps.empty() ? s->records.size() : s->cps[0].first_record;
    for (size_t r = 0; r < gone; ++r) drop_record(s->records[r]);
    s->records.erase(s->records.begin(), s->records.begin() + gone);
    for (auto& c : s->cps) c.first_record -= gone;
    if (s->cps.empty()) {
        drop_record(s->next);
        s->used = s->base = 0;
    } else {
        s->base = s->cps[0].used;
    }
    return MK_OK;
}

uint64_t set_journal_bytes(const mk_tree_set* s) {
    uint64_t b = s->used - s->base;
    for (const auto& r : s->records)
        for (const auto& f : r.full) b += f.second->items.cap + f.second->level0.cap + f.second->levels.cap;
    return b;
}

int set_journal_reserve(mk_tree_set* s, uint64_t bytes) {  // bytes of live journal the buffer has room for
    if (!s) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t live = s->used - s->base;
    if (bytes <= live || s->journal.cap >= s->used + (bytes - live)) return MK_OK;
    TRY(bind_set(s));
    return journal_room(s, bytes - live);
}

// ---- audit ------------------------------------------------------------------------
// Everything pending is flushed and waited for, as for a root; then the chain
// of tree_audit_api.cpp over all the trees and the message as the device holds
// it, and one read-back of the count + 1 reports.  The set's workspace holds
// the reports (its front, 512 bytes) and the level-0 piece behind them.
int set_audit(mk_tree_set* s, mk_audit_report* out) {
    if (!s || !out) return fail(MK_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lk(s->mu);
    const uint32_t nt = (uint32_t)s->trees.size();
    if (nt == 0) return fail(MK_EINVAL, "a set without trees has nothing to audit");
    TRY(settle(s));
    const uint32_t clen = nparts(s) ? s->container_len : 0;
    mk_tree_audit table[MK_TREES_MAX] = {};
    const StructTreeLayout* layouts[MK_TREES_MAX] = {};
    for (uint32_t i = 0; i < nt; ++i) {
        const mk_tree_set::Tree& t = s->trees[i];
        table[i] = tree_audit_desc(*t.h, clen ? t.coff : MK_NO_CONTAINER);
        if (t.kind == MK_TREE_STRUCT) layouts[i] = struct_tree_layout_of(*t.h);
    }
    AuditCall c;
    TRY(trees_audit_prepare(table, nt, layouts, clen, c));
    TRY(bind_set(s));
    hipStream_t st = ctx()->stream;
    TRY(grow(s->ws, 512 + c.ws));
    uint8_t* ws = (uint8_t*)s->ws.p;
    const void* msg = clen ? s->stage.p : nullptr;
    const void* croot = clen ? s->croot.p : nullptr;
    TRY(trees_audit_check(table, nt, c, msg, clen, croot, ws, ws + 512, c.ws));
    TRY(trees_audit_launch(table, nt, c, msg, clen, croot, ws, ws + 512, st));
    HIPCHK(hipMemcpyAsync(out, ws, (nt + 1) * sizeof(mk_audit_report), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MK_OK;
}

// ---- diff -------------------------------------------------------------------------
// Both sets flushed and waited for, as for a root; then the one launch of
// tree_diff_api.cpp over all the pairs and one read-back.  a's workspace holds
// the reports (its front, 256 bytes) and the trees' slots behind them.  The
// container's report is the host's: the two messages outside the trees' roots.
int set_diff(mk_tree_set* a, mk_tree_set* b, mk_diff_report* reports, uint64_t* idx_out, uint64_t per) {
    if (!a || !b || !reports || (per && !idx_out)) return fail(MK_EINVAL, "null pointer");
    if (per >= (1ull << 56)) return fail(MK_EINVAL, "max_out_per_tree * 8 * %d overflows", MK_TREES_MAX);
    if (a == b) {
        std::lock_guard<std::mutex> lk(a->mu);
        for (size_t i = 0; i <= a->trees.size(); ++i) reports[i] = mk_diff_report{0, ~0ull};
        return MK_OK;
    }
    LockBoth lk(a->mu, b->mu);
    TRY(sets_agree(a, b));
    const uint32_t nt = (uint32_t)a->trees.size();
    TRY(settle(a));
    TRY(settle(b));
    for (uint32_t i = 0; i <= nt; ++i) reports[i] = mk_diff_report{0, ~0ull};
    if (nt) {
        TRY(bind_set(a));
        hipStream_t st = ctx()->stream;
        static_assert(MK_TREES_MAX * sizeof(mk_diff_report) <= 256, "the reports' room at the workspace's front");
        TRY(grow(a->ws, 256 + 8 * per * nt));
        uint8_t* ws = (uint8_t*)a->ws.p;
        mk_tree_diff table[MK_TREES_MAX] = {};
        for (uint32_t i = 0; i < nt; ++i)
            table[i] = tree_diff_desc(*a->trees[i].h, *b->trees[i].h, (uint64_t*)(ws + 256) + per * i, per);
        TRY(trees_diff_check(table, nt, ws));
        TRY(trees_diff_launch(table, nt, ws, st));
        std::vector<uint64_t> back(32 + per * nt);
        HIPCHK(hipMemcpyAsync(back.data(), ws, 8 * back.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < nt; ++i) {
            reports[i] = mk_diff_report{back[2 * i], back[2 * i + 1]};
            uint64_t* slots = back.data() + 32 + per * i;
            tree_diff_sort(slots, reports[i].total, per);
            if (per) std::memcpy(idx_out + per * i, slots, 8 * std::min(reports[i].total, per));
        }
    }
    // the message outside every tree's root: what put() wrote
    std::vector<uint8_t> skip(a->container_len, 0);
    for (const auto& t : a->trees)
        if (t.coff != MK_NO_CONTAINER) std::fill(skip.begin() + t.coff, skip.begin() + t.coff + 32, 1);
    for (uint32_t o = 0; o < a->container_len; ++o) {
        if (skip[o] || a->msg[o] == b->msg[o]) continue;
        if (reports[nt].total++ == 0) reports[nt].first_index = o;
    }
    return MK_OK;
}

}  // namespace

extern "C" {

int mk_tree_set_checkpoint(mk_call* call, mk_tree_set* s, uint64_t* id) {
    Scope S(call);
    return S.done(set_checkpoint(s, id));
}

int mk_tree_set_rollback(mk_call* call, mk_tree_set* s, uint64_t id) {
    Scope S(call);
    return S.done(set_rollback(s, id));
}

int mk_tree_set_release(mk_call* call, mk_tree_set* s, uint64_t id) {
    Scope S(call, false);
    return S.done(set_release(s, id));
}

uint64_t mk_tree_set_journal_bytes(const mk_tree_set* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lk(const_cast<mk_tree_set*>(s)->mu);
    return set_journal_bytes(s);
}

uint64_t mk_tree_set_journal_capacity(const mk_tree_set* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lk(const_cast<mk_tree_set*>(s)->mu);
    return s->journal.p ? s->journal.cap : 0;
}

int mk_tree_set_journal_reserve(mk_call* call, mk_tree_set* s, uint64_t bytes) {
    Scope S(call);
    return S.done(set_journal_reserve(s, bytes));
}

int mk_tree_set_diff(mk_call* call, mk_tree_set* a, mk_tree_set* b, mk_diff_report* reports, uint64_t* idx_out,
                     uint64_t max_out_per_tree) {
    Scope S(call);
    return S.done(set_diff(a, b, reports, idx_out, max_out_per_tree));
}

int mk_tree_set_audit(mk_call* call, mk_tree_set* s, mk_audit_report* out) {
    Scope S(call);
    return S.done(set_audit(s, out));
}

int mk_tree_set_clone(mk_call* call, mk_tree_set* src, mk_tree_set** out) {
    Scope S(call);
    return S.done(set_clone(src, out));
}

int mk_tree_set_copy(mk_call* call, mk_tree_set* dst, mk_tree_set* src) {
    Scope S(call);
    return S.done(set_copy(dst, src));
}

int mk_tree_set_reserve(mk_call* call, mk_tree_set* s, uint32_t tree, uint64_t capacity) {
    Scope S(call);
    return S.done(set_reserve(s, tree, capacity));
}

uint64_t mk_tree_set_capacity(const mk_tree_set* s, uint32_t tree) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lk(const_cast<mk_tree_set*>(s)->mu);
    return tree < s->trees.size() ? s->trees[tree].h->cap : 0;
}

// No device is needed before the first tree is added: a bad argument is MK_EINVAL on any machine.
int mk_tree_set_new(mk_call* call, uint32_t container_len, mk_tree_set** out) {
    Scope S(call, false);
    if (!out) return S.done(fail(MK_EINVAL, "null pointer"));
    *out = nullptr;
    if (container_len > MK_CONTAINER_MAX)
        return S.done(fail(MK_EINVAL, "container of %u bytes (limit %d)", container_len, MK_CONTAINER_MAX));
    auto* s = new (std::nothrow) mk_tree_set();
    if (!s) return S.done(fail(MK_ENOMEM, "tree set allocation failed"));
    s->dev = call ? call->device : -1;
    s->container_len = container_len;
    s->msg.assign(container_len, 0);
    *out = s;
    return S.done(MK_OK);
}

void mk_tree_set_free(mk_tree_set* s) {
    if (!s) return;
    for (auto& t : s->trees) tree_free(t.h);  // each restores the caller's device
    for (auto& r : s->records)
        for (auto& f : r.full) tree_free(f.second);
    for (auto& f : s->next.full) tree_free(f.second);
    if (s->dev >= 0 && (s->host || s->stage.p || s->ws.p || s->croot.p || s->journal.p)) {
        int saved = -1;
        const bool restore = hipGetDevice(&saved) == hipSuccess;
        (void)hipSetDevice(s->dev);
        if (s->host) (void)hipHostFree(s->host);
        for (DevBuf* b : {&s->stage, &s->ws, &s->croot, &s->journal})
            if (b->p) (void)hipFree(b->p);
        if (restore) (void)hipSetDevice(saved);
    }
    delete s;
}

int mk_tree_set_add(mk_call* call, mk_tree_set* s, uint32_t kind, uint32_t item_len, const mk_field* fields,
                    uint32_t nfields, uint64_t capacity, uint32_t container_off, uint32_t* tree) {
    Scope S(call);
    return S.done(set_add(s, kind, item_len, fields, nfields, capacity, container_off, tree));
}

int mk_tree_set_put(mk_call* call, mk_tree_set* s, uint32_t off, const uint8_t* bytes, uint32_t len) {
    Scope S(call, false);
    return S.done(set_put(s, off, bytes, len));
}

int mk_tree_set_assign(mk_call* call, mk_tree_set* s, uint32_t tree, const uint8_t* values, uint64_t n) {
    Scope S(call);
    return S.done(set_assign(s, tree, values, n));
}

int mk_tree_set_update(mk_call* call, mk_tree_set* s, uint32_t tree, const uint64_t* idx, const uint8_t* values,
                       uint64_t k) {
    Scope S(call, false);
    return S.done(set_update(s, tree, idx, values, k));
}

int mk_tree_set_append(mk_call* call, mk_tree_set* s, uint32_t tree, const uint8_t* values, uint64_t k) {
    Scope S(call, false);
    return S.done(set_append(s, tree, values, k));
}

int mk_tree_set_truncate(mk_call* call, mk_tree_set* s, uint32_t tree, uint64_t n) {
    Scope S(call);
    return S.done(set_shrink(s, tree, false, nullptr, 0, n));
}

int mk_tree_set_erase(mk_call* call, mk_tree_set* s, uint32_t tree, const uint64_t* idx, uint64_t k) {
    Scope S(call);
    return S.done(set_shrink(s, tree, true, idx, k, 0));
}

uint64_t mk_tree_set_count(const mk_tree_set* s, uint32_t tree) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lk(const_cast<mk_tree_set*>(s)->mu);
    return tree < s->pend.size() ? s->pend[tree].count() : 0;
}

int mk_tree_set_root(mk_call* call, mk_tree_set* s, uint8_t root[32]) {
    Scope S(call);
    return S.done(set_root(s, root));
}

int mk_tree_set_tree_root(mk_call* call, mk_tree_set* s, uint32_t tree, uint8_t root[32]) {
    Scope S(call);
    return S.done(set_tree_root(s, tree, root));
}

int mk_tree_set_items(mk_call* call, mk_tree_set* s, uint32_t tree, uint64_t first, uint64_t cnt, uint8_t* out) {
    Scope S(call);
    return S.done(set_items(s, tree, first, cnt, out));
}

int mk_tree_set_branches(mk_call* call, mk_tree_set* s, uint32_t tree, const uint64_t* idx, uint64_t k,
                         uint8_t* values_out, uint8_t* branches_out, uint8_t* container_out) {
    Scope S(call);
    return S.done(set_branches(s, tree, idx, k, values_out, branches_out, container_out));
}

int mk_tree_set_verify_repeat_hash(mk_call* call, mk_tree_set* s, uint32_t tree, uint32_t commit_off,
                                   uint32_t layers_off, const uint64_t* idx, const uint8_t* reveals, uint64_t m,
                                   uint32_t max_layers, uint8_t* ok) {
    Scope S(call);
    return S.done(set_verify_repeat_hash(s, tree, commit_off, layers_off, idx, reveals, m, max_layers, ok));
}

}  // extern "C"
