// Resident trees copied on the device between the layouts of two capacities
// (DESIGN.md §5m): the device entry mk_dev_ssz_trees_copy -- every argument
// check, then the one launch of k_trees_copy.  The handle calls (mk_*_tree_clone
// / _copy / _reserve, mk_tree_set_clone / _copy / _reserve) are tree_handle.cpp's
// and tree_set_api.cpp's over the same two functions; the piece map is
// tree_copy.hpp's.
#include "runtime.hpp"
#include "tree_copy.hpp"

using namespace mk;
using namespace mk::rt;

static_assert(MK_TREES_MAX == mk::kTreesMax, "MK_TREES_MAX and the kernel's descriptor table differ");

namespace {

// Workgroups of the copy: four per CU are resident beside their 27 KB of LDS
// and hold 64 KiB of loads in flight per CU; the rest of the pieces by grid stride.
constexpr uint64_t kCopyGridMax = 1024;

struct Extent {
    uintptr_t lo, hi;  // [lo, hi), never empty
};

bool level0_kind(uint32_t kind) { return kind != MK_TREE_LIST; }

CopyShape shape_of(const mk_tree_copy& t) {
    return copy_shape(t.n, t.src_capacity, t.dst_capacity, t.item_len, level0_kind(t.kind));
}

void add_extent(std::vector<Extent>& v, const void* p, uint64_t bytes) {
    if (bytes) v.push_back({(uintptr_t)p, (uintptr_t)p + bytes});
}

// what one side of a tree's copy touches: the values, level 0, the levels from the first stored node to
// the top (one extent: the gaps between two levels' live nodes count as touched) and the root
void tree_extents(std::vector<Extent>& v, const CopyShape& c, uint64_t cap_chunks, const void* items,
                  const void* level0, const void* levels, const void* root) {
    add_extent(v, items, copy_seg_bytes(c, 0));
    add_extent(v, level0, copy_seg_bytes(c, 1));
    if (c.D) add_extent(v, levels, 32 * (copy_level_off(cap_chunks, c.D) + copy_level_count(c, c.D)));
    add_extent(v, root, 32);
}

int check_tree(const mk_tree_copy& t, uint32_t i) {
    if (t.kind != MK_TREE_LIST && t.kind != MK_TREE_STRUCT && t.kind != MK_TREE_BYTES)
        return fail(MK_EINVAL, "tree %u: unknown kind %u", i, t.kind);
    if (t.item_len == 0) return fail(MK_EINVAL, "tree %u: item_len == 0", i);
    if (t.item_len > (1u << 30)) return fail(MK_EINVAL, "tree %u: item_len %u above 2^30", i, t.item_len);
    if (t.n > t.src_capacity || t.n > t.dst_capacity)
        return fail(MK_EINVAL, "tree %u: %llu values > capacity %llu (source) or %llu (destination)", i,
                    (unsigned long long)t.n, (unsigned long long)t.src_capacity, (unsigned long long)t.dst_capacity);
    if (std::max(t.src_capacity, t.dst_capacity) > UINT64_MAX / std::max<uint32_t>(t.item_len, 32))
        return fail(MK_EINVAL, "tree %u: capacity * item_len overflows", i);
    const bool l0 = level0_kind(t.kind);
    if (!l0 && (t.d_src_level0 || t.d_dst_level0)) return fail(MK_EINVAL, "tree %u: a level 0 for a list tree", i);
    if (!t.d_src_root32 || !t.d_dst_root32) return fail(MK_EINVAL, "tree %u: null pointer (root)", i);
    if (t.n && (!t.d_src_items || !t.d_dst_items)) return fail(MK_EINVAL, "tree %u: null pointer (values)", i);
    if (t.n && l0 && (!t.d_src_level0 || !t.d_dst_level0)) return fail(MK_EINVAL, "tree %u: null pointer (level 0)", i);
    if (shape_of(t).D && (!t.d_src_levels || !t.d_dst_levels)) return fail(MK_EINVAL, "tree %u: null level array", i);
    const uintptr_t a = (uintptr_t)t.d_src_level0 | (uintptr_t)t.d_dst_level0 | (uintptr_t)t.d_src_levels |
                        (uintptr_t)t.d_dst_levels | (uintptr_t)t.d_src_root32 | (uintptr_t)t.d_dst_root32;
    if (a % 16) return fail(MK_EINVAL, "tree %u: level 0, level array or root misaligned (16 B)", i);
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int trees_copy_check(const mk_tree_copy* trees, uint32_t ntrees, const void* d_src_extra32,
                     const void* d_dst_extra32) {
    if (ntrees > MK_TREES_MAX) return fail(MK_EINVAL, "%u trees in one call (0 .. %d)", ntrees, MK_TREES_MAX);
    if (ntrees && !trees) return fail(MK_EINVAL, "null pointer");
    if (!d_src_extra32 != !d_dst_extra32) return fail(MK_EINVAL, "the 32-byte extra needs a source and a destination");
    if (((uintptr_t)d_src_extra32 | (uintptr_t)d_dst_extra32) % 16) return fail(MK_EINVAL, "the 32-byte extra misaligned (16 B)");
    for (uint32_t i = 0; i < ntrees; ++i) TRY(check_tree(trees[i], i));
    // no source range of the call may overlap a destination range: the pieces move in no order
    std::vector<Extent> src, dst;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_copy& t = trees[i];
        const CopyShape c = shape_of(t);
        tree_extents(src, c, c.cap_src_chunks, t.d_src_items, t.d_src_level0, t.d_src_levels, t.d_src_root32);
        tree_extents(dst, c, c.cap_dst_chunks, t.d_dst_items, t.d_dst_level0, t.d_dst_levels, t.d_dst_root32);
    }
    add_extent(src, d_src_extra32, d_src_extra32 ? 32 : 0);
    add_extent(dst, d_dst_extra32, d_dst_extra32 ? 32 : 0);
    for (const Extent& s : src)
        for (const Extent& d : dst)
            if (s.lo < d.hi && d.lo < s.hi)
                return fail(MK_EINVAL, "a source range [%p, +%llu) overlaps a destination range [%p, +%llu)",
                            (void*)s.lo, (unsigned long long)(s.hi - s.lo), (void*)d.lo,
                            (unsigned long long)(d.hi - d.lo));
    return MK_OK;
}

int trees_copy_launch(const mk_tree_copy* trees, uint32_t ntrees, const void* d_src_extra32, void* d_dst_extra32,
                      hipStream_t st) {
    mk::TreesCopyArgs a{};
    uint64_t pieces = d_dst_extra32 ? 32 / kCopyPiece : 0;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_copy& t = trees[i];
        mk::CopyTree& c = a.t[i];
        c.src_items = (const uint8_t*)t.d_src_items, c.dst_items = (uint8_t*)t.d_dst_items;
        c.src_level0 = (const uint8_t*)t.d_src_level0, c.dst_level0 = (uint8_t*)t.d_dst_level0;
        c.src_levels = (const uint8_t*)t.d_src_levels, c.dst_levels = (uint8_t*)t.d_dst_levels;
        c.src_root = (const uint8_t*)t.d_src_root32, c.dst_root = (uint8_t*)t.d_dst_root32;
        c.n = t.n, c.cap_src = t.src_capacity, c.cap_dst = t.dst_capacity;
        c.item_len = t.item_len;
        c.level0 = level0_kind(t.kind);
        pieces += copy_pieces(shape_of(t));
    }
    if (pieces == 0) return MK_OK;
    a.extra_src = (const uint8_t*)d_src_extra32;
    a.extra_dst = (uint8_t*)d_dst_extra32;
    a.ntrees = ntrees;
    const uint64_t grid = std::min<uint64_t>(ceil_div(pieces, (uint64_t)mk::kCopyThreads * mk::kCopyUnroll), kCopyGridMax);
    hipLaunchKernelGGL(mk::k_trees_copy, dim3((uint32_t)grid), dim3(mk::kCopyThreads), 0, st, a);
    return launched();
}

}  // namespace mk::rt

extern "C" {

// Every argument check comes before the stream's device is looked up: a bad
// call is MK_EINVAL on any machine.  One launch, nothing uploaded or allocated,
// no synchronise: capturable.
int mk_dev_ssz_trees_copy(mk_call* call, const mk_tree_copy* trees, uint32_t ntrees, const void* d_src_extra32,
                          void* d_dst_extra32, void* stream) {
    Scope S(call);
    int rc = trees_copy_check(trees, ntrees, d_src_extra32, d_dst_extra32);
    if (!rc && ntrees == 0 && !d_dst_extra32) return S.done(MK_OK);  // nothing to do: no device needed
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc) rc = trees_copy_launch(trees, ntrees, d_src_extra32, d_dst_extra32, (hipStream_t)stream);
    return S.done(rc);
}

}  // extern "C"
