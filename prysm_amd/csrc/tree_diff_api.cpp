// Two resident trees diffed on the device by Merkle descent:
// the device entry mk_dev_ssz_trees_diff -- every argument check, then the
// reports cleared and the one launch of k_trees_diff.  The handle calls
// (mk_*_tree_diff, mk_tree_set_diff) are tree_handle.cpp's and
// tree_set_api.cpp's over the same two functions; the rule is tree_diff.hpp's.
#include "runtime.hpp"
#include "tree_diff.hpp"

using namespace mk;
using namespace mk::rt;

static_assert(MK_TREES_MAX == mk::kTreesMax, "MK_TREES_MAX and the kernel's descriptor table differ");
static_assert(sizeof(mk_diff_report) == sizeof(mk::DiffReport) && sizeof(mk_diff_report) == 16,
              "mk_diff_report and the kernel's report differ");

namespace {

// Workgroups of k_trees_diff: eight of 256 threads per CU, the rest of the work items by grid stride.  An
// item whose root is equal costs two 32-byte loads, so most turns are short.
constexpr uint64_t kDiffGridMax = 2048;

struct Extent {
    uintptr_t lo, hi;  // [lo, hi), never empty
};

bool level0_kind(uint32_t kind) { return kind != MK_TREE_LIST; }
uint32_t len0_of(const mk_tree_diff& t) { return level0_kind(t.kind) ? 32u : t.item_len; }

DiffShape shape_of(const mk_tree_diff& t) {
    return diff_shape(t.n_a, t.capacity_a, t.n_b, t.capacity_b, len0_of(t));
}

void add_extent(std::vector<Extent>& v, const void* p, uint64_t bytes) {
    if (p && bytes) v.push_back({(uintptr_t)p, (uintptr_t)p + bytes});
}

// what one side of a pair may be read from: its values, its level 0 and its levels from the first stored
// node to the top of its own tree (one extent, as the copy counts them)
void side_extents(std::vector<Extent>& v, const mk_tree_diff& t, uint64_t n, uint64_t capacity, const void* items,
                  const void* level0, const void* levels) {
    const CopyShape c = copy_shape(n, capacity, capacity, t.item_len, level0_kind(t.kind));
    add_extent(v, items, copy_seg_bytes(c, 0));
    add_extent(v, level0, copy_seg_bytes(c, 1));
    if (c.D) add_extent(v, levels, 32 * (copy_level_off(c.cap_src_chunks, c.D) + copy_level_count(c, c.D)));
}

bool overlaps(const Extent& a, const Extent& b) { return a.lo < b.hi && b.lo < a.hi; }

int check_tree(const mk_tree_diff& t, uint32_t i, uint64_t& items) {
    if (t.kind != MK_TREE_LIST && t.kind != MK_TREE_STRUCT && t.kind != MK_TREE_BYTES)
        return fail(MK_EINVAL, "pair %u: unknown kind %u", i, t.kind);
    if (t.item_len == 0) return fail(MK_EINVAL, "pair %u: item_len == 0", i);
    if (t.kind == MK_TREE_LIST && t.item_len > kDiffItemMax)
        return fail(MK_EINVAL, "pair %u: item_len %u above %u", i, t.item_len, kDiffItemMax);
    if (t.item_len > (1u << 30)) return fail(MK_EINVAL, "pair %u: item_len %u above 2^30", i, t.item_len);
    if (t.n_a > t.capacity_a || t.n_b > t.capacity_b)
        return fail(MK_EINVAL, "pair %u: %llu values > capacity %llu (a) or %llu > %llu (b)", i,
                    (unsigned long long)t.n_a, (unsigned long long)t.capacity_a, (unsigned long long)t.n_b,
                    (unsigned long long)t.capacity_b);
    if (std::max(t.capacity_a, t.capacity_b) > UINT64_MAX / std::max<uint32_t>(t.item_len, 32))
        return fail(MK_EINVAL, "pair %u: capacity * item_len overflows", i);
    const bool l0 = level0_kind(t.kind);
    if (!l0 && (t.d_a_level0 || t.d_b_level0)) return fail(MK_EINVAL, "pair %u: a level 0 for a list tree", i);
    const DiffShape s = shape_of(t);
    const void* leaves_a = l0 ? t.d_a_level0 : t.d_a_items;
    const void* leaves_b = l0 ? t.d_b_level0 : t.d_b_items;
    if (s.m && (!leaves_a || !leaves_b))
        return fail(MK_EINVAL, "pair %u: null pointer (%s)", i, l0 ? "level 0" : "values");
    if (s.h0 && (!t.d_a_levels || !t.d_b_levels)) return fail(MK_EINVAL, "pair %u: null level array", i);
    const uintptr_t a = (uintptr_t)t.d_a_level0 | (uintptr_t)t.d_b_level0 | (uintptr_t)t.d_a_levels |
                        (uintptr_t)t.d_b_levels;
    if (a % 16) return fail(MK_EINVAL, "pair %u: level 0 or level array misaligned (16 B)", i);
    if (t.max_out && !t.d_idx_out) return fail(MK_EINVAL, "pair %u: null index buffer for %llu slots", i,
                                               (unsigned long long)t.max_out);
    if ((uintptr_t)t.d_idx_out % 8) return fail(MK_EINVAL, "pair %u: index buffer misaligned (8 B)", i);
    if (t.max_out > UINT64_MAX / 8) return fail(MK_EINVAL, "pair %u: max_out * 8 overflows", i);
    items += diff_items(s);
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int trees_diff_check(const mk_tree_diff* trees, uint32_t ntrees, const void* d_reports) {
    if (ntrees == 0 || ntrees > MK_TREES_MAX)
        return fail(MK_EINVAL, "%u tree pairs in one call (1 .. %d)", ntrees, MK_TREES_MAX);
    if (!trees) return fail(MK_EINVAL, "null pointer");
    if (!d_reports) return fail(MK_EINVAL, "null pointer (reports)");
    if ((uintptr_t)d_reports % 8) return fail(MK_EINVAL, "reports misaligned (8 B)");
    uint64_t items = 0;
    for (uint32_t i = 0; i < ntrees; ++i) TRY(check_tree(trees[i], i, items));
    if (items >= kMaxWork)
        return fail(MK_EINVAL, "%llu work items in one diff (limit 2^31 - 1)", (unsigned long long)items);
    // no range the call writes may overlap a range it reads, or another it writes: the order is unspecified
    std::vector<Extent> in, out;
    add_extent(out, d_reports, (uint64_t)ntrees * sizeof(mk_diff_report));
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_diff& t = trees[i];
        side_extents(in, t, t.n_a, t.capacity_a, t.d_a_items, t.d_a_level0, t.d_a_levels);
        side_extents(in, t, t.n_b, t.capacity_b, t.d_b_items, t.d_b_level0, t.d_b_levels);
        add_extent(out, t.d_idx_out, 8 * t.max_out);
    }
    for (size_t o = 0; o < out.size(); ++o) {
        for (const Extent& s : in)
            if (overlaps(out[o], s))
                return fail(MK_EINVAL, "an output range [%p, +%llu) overlaps an input range [%p, +%llu)",
                            (void*)out[o].lo, (unsigned long long)(out[o].hi - out[o].lo), (void*)s.lo,
                            (unsigned long long)(s.hi - s.lo));
        for (size_t k = 0; k < o; ++k)
            if (overlaps(out[o], out[k]))
                return fail(MK_EINVAL, "two output ranges overlap: [%p, +%llu) and [%p, +%llu)", (void*)out[o].lo,
                            (unsigned long long)(out[o].hi - out[o].lo), (void*)out[k].lo,
                            (unsigned long long)(out[k].hi - out[k].lo));
    }
    return MK_OK;
}

int trees_diff_launch(const mk_tree_diff* trees, uint32_t ntrees, void* d_reports, hipStream_t st) {
    mk::DiffReport* reports = (mk::DiffReport*)d_reports;
    hipLaunchKernelGGL(mk::k_diff_reports, dim3(1), dim3(64), 0, st, reports, ntrees);
    TRY(launched());
    mk::TreesDiffArgs a{};
    uint64_t items = 0;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_diff& t = trees[i];
        const bool l0 = level0_kind(t.kind);
        mk::DiffTree& T = a.t[i];
        T.a_leaves = (const uint8_t*)(l0 ? t.d_a_level0 : t.d_a_items);
        T.b_leaves = (const uint8_t*)(l0 ? t.d_b_level0 : t.d_b_items);
        T.a_levels = (const uint8_t*)t.d_a_levels;
        T.b_levels = (const uint8_t*)t.d_b_levels;
        T.n_a = t.n_a, T.cap_a = t.capacity_a, T.n_b = t.n_b, T.cap_b = t.capacity_b;
        T.idx_out = t.d_idx_out;
        T.max_out = t.max_out;
        T.len0 = len0_of(t);
        items += diff_items(shape_of(t));
    }
    if (items == 0) return MK_OK;  // nothing below min(n_a, n_b) anywhere: the cleared reports are the answer
    a.reports = reports;
    a.ntrees = ntrees;
    const uint64_t grid = std::min<uint64_t>(items, kDiffGridMax);
    hipLaunchKernelGGL(mk::k_trees_diff, dim3((uint32_t)grid), dim3(mk::kDiffThreads), 0, st, a);
    return launched();
}

}  // namespace mk::rt

extern "C" {

// Every argument check comes before the stream's device is looked up: a bad
// call is MK_EINVAL on any machine.  Nothing uploaded or allocated, no
// workspace, no synchronise: capturable.
int mk_dev_ssz_trees_diff(mk_call* call, const mk_tree_diff* trees, uint32_t ntrees, void* d_reports, void* stream) {
    Scope S(call);
    int rc = trees_diff_check(trees, ntrees, d_reports);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = trees_diff_launch(trees, ntrees, d_reports, (hipStream_t)stream);
    return S.done(rc);
}

}  // extern "C"
