// Undo journal of resident trees: the device entries
// mk_dev_ssz_trees_journal and mk_dev_ssz_trees_restore -- every argument
// check, then the one launch of k_trees_journal / k_trees_restore.  Both take
// the array mk_dev_ssz_trees_update takes and its argument rules
// (trees_update_check); where a piece lies in the journal is tree_journal.hpp's.
#include "runtime.hpp"
#include "tree_journal.hpp"

using namespace mk;
using namespace mk::rt;

static_assert(MK_TREES_MAX == mk::kTreesMax, "MK_TREES_MAX and the kernel's descriptor table differ");
static_assert(sizeof(mk::JournalArgs) <= 4096, "the journal's segments travel in the kernel arguments");

namespace {

constexpr uint64_t kTreeBytesMax = 1ull << 56;  // one tree's region: sixteen of them add up without overflow

struct JournalLayout {
    JournalShape shape[MK_TREES_MAX];
    uint64_t off[MK_TREES_MAX];  // the tree's region
    uint64_t container = 0;      // the message's, then its root's
    uint64_t total = 0;
};

JournalShape shape_of(const mk_tree_update& t) {
    return journal_shape(t.n_old, t.n_new, t.capacity, t.k_idx, t.item_len, t.kind != MK_TREE_LIST);
}

// value pieces of 16 or 8 bytes when the length and the value buffer allow (the journal's side always does)
uint32_t unit_of(const mk_tree_update& t) {
    const uintptr_t a = (uintptr_t)t.d_items;
    return t.item_len % 16 == 0 && a % 16 == 0 ? 16 : t.item_len % 8 == 0 && a % 8 == 0 ? 8 : 1;
}

// the trees' own rules are checked by the caller; the layout needs none of the pointers
int make_layout(const mk_tree_update* trees, uint32_t ntrees, uint32_t container_len, JournalLayout& J) {
    uint64_t pos = 0;
    for (uint32_t i = 0; i < ntrees; ++i) {
        J.shape[i] = shape_of(trees[i]);
        const JournalShape& s = J.shape[i];
        if (s.W && journal_rec_bytes(s) > kTreeBytesMax / s.W)
            return fail(MK_EINVAL, "tree %u: a journal of %llu records of %llu bytes", i, (unsigned long long)s.W,
                        (unsigned long long)journal_rec_bytes(s));
        J.off[i] = pos;
        pos += journal_tree_bytes(s);
    }
    J.container = pos;
    J.total = pos + journal_container_bytes(container_len);
    return MK_OK;
}

int check_all(const mk_tree_update* trees, uint32_t ntrees, const void* d_container, uint32_t container_len,
              const void* d_container_root32, const void* d_journal, uint64_t journal_bytes, bool lists,
              JournalLayout& J) {
    if (!d_journal || ((uintptr_t)d_journal % 16)) return fail(MK_EINVAL, "null or misaligned (16 B) journal");
    // no workspace here: any aligned address satisfies the update's rule for it
    TRY(trees_update_check(trees, ntrees, d_container, container_len, d_container_root32, (const void*)16, lists));
    TRY(make_layout(trees, ntrees, container_len, J));
    if (journal_bytes < J.total)
        return fail(MK_ENOMEM, "journal of %llu bytes, %llu needed", (unsigned long long)journal_bytes,
                    (unsigned long long)J.total);
    return MK_OK;
}

int launch(bool restore, const mk_tree_update* trees, uint32_t ntrees, const JournalLayout& J, void* d_container,
           uint32_t container_len, void* d_container_root32, void* d_journal, hipStream_t st) {
    mk::JournalArgs a{};
    uint8_t* jr = (uint8_t*)d_journal;
    uint64_t pieces = container_len ? (container_len + 3) / 4 + 8 : 0;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        mk::JournalSeg& s = a.s[i];
        s.items = (uint8_t*)t.d_items, s.level0 = (uint8_t*)t.d_level0, s.levels = (uint8_t*)t.d_levels;
        s.root = (uint8_t*)t.d_root32;
        s.idx = restore ? nullptr : t.d_idx;
        s.jr = jr + J.off[i];
        s.n_old = t.n_old, s.n_new = t.n_new, s.capacity = t.capacity, s.k_idx = t.k_idx;
        s.item_len = t.item_len;
        s.unit = unit_of(t);
        pieces = std::max(pieces, journal_pieces(J.shape[i], s.unit));
    }
    a.ntrees = ntrees;
    a.container_len = container_len;
    if (container_len) {
        a.container = (uint8_t*)d_container;
        a.container_root = (uint8_t*)d_container_root32;
        a.jr_container = jr + J.container;
    }
    const uint64_t blocks = ceil_div(pieces, 256);
    if (blocks > 0x7fffffffull) return fail(MK_EINVAL, "%llu blocks of journal pieces", (unsigned long long)blocks);
    const dim3 grid((uint32_t)blocks, ntrees + (container_len ? 1 : 0));
    if (restore)
        hipLaunchKernelGGL(mk::k_trees_restore, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(mk::k_trees_journal, grid, dim3(256), 0, st, a);
    return launched();
}

}  // namespace

namespace mk::rt {
int trees_journal_bytes(const mk_tree_update* trees, uint32_t ntrees, uint32_t container_len, uint64_t* bytes) {
    uint64_t ws = 0;
    JournalLayout J;
    if (container_len > MK_CONTAINER_MAX)
        return fail(MK_EINVAL, "container of %u bytes (limit %d)", container_len, MK_CONTAINER_MAX);
    TRY(trees_update_workspace(trees, ntrees, &ws));
    TRY(make_layout(trees, ntrees, container_len, J));
    *bytes = J.total;
    return MK_OK;
}

int trees_journal(bool restore, const mk_tree_update* trees, uint32_t ntrees, void* d_container, uint32_t container_len,
                  void* d_container_root32, void* d_journal, uint64_t journal_bytes, hipStream_t st) {
    JournalLayout J;
    TRY(check_all(trees, ntrees, d_container, container_len, d_container_root32, d_journal, journal_bytes, !restore, J));
    return launch(restore, trees, ntrees, J, d_container, container_len, d_container_root32, d_journal, st);
}
}  // namespace mk::rt

extern "C" {

uint64_t mk_ssz_trees_journal_bytes(const mk_tree_update* trees, uint32_t ntrees, uint32_t container_len) {
    Scope S(nullptr, false);
    uint64_t ws = 0;
    JournalLayout J;
    if (container_len > MK_CONTAINER_MAX || trees_update_workspace(trees, ntrees, &ws) != MK_OK ||
        make_layout(trees, ntrees, container_len, J) != MK_OK)
        return 0;
    return J.total;
}

// Every argument check, the pointers included, comes before the stream's
// device is looked up: a bad call is MK_EINVAL / MK_ENOMEM on any machine.
// One launch each, nothing uploaded or allocated, no synchronise: capturable.
int mk_dev_ssz_trees_journal(mk_call* call, const mk_tree_update* trees, uint32_t ntrees, const void* d_container,
                             uint32_t container_len, const void* d_container_root32, void* d_journal,
                             uint64_t journal_bytes, void* stream) {
    Scope S(call);
    JournalLayout J;
    int rc = check_all(trees, ntrees, d_container, container_len, d_container_root32, d_journal, journal_bytes, true, J);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = launch(false, trees, ntrees, J, (void*)d_container, container_len, (void*)d_container_root32, d_journal,
                    (hipStream_t)stream);
    return S.done(rc);
}

int mk_dev_ssz_trees_restore(mk_call* call, const mk_tree_update* trees, uint32_t ntrees, void* d_container,
                             uint32_t container_len, void* d_container_root32, const void* d_journal,
                             uint64_t journal_bytes, void* stream) {
    Scope S(call);
    JournalLayout J;
    int rc = check_all(trees, ntrees, d_container, container_len, d_container_root32, d_journal, journal_bytes, false, J);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = launch(true, trees, ntrees, J, d_container, container_len, d_container_root32, (void*)d_journal,
                    (hipStream_t)stream);
    return S.done(rc);
}

}  // extern "C"
