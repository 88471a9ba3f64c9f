// Several device-resident trees in one call: every tree's
// stage 0 by the launchers of its own update entry point (list_tree_api,
// struct_tree_api, bytes_tree_api), then all the climbs, the trees of one
// chunk and the hash of the struct that holds them in ONE launch
// (k_trees_update) -- mk_dev_ssz_trees_update.
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

static_assert(MK_TREES_MAX == mk::kTreesMax, "MK_TREES_MAX and the kernel's descriptor table differ");
static_assert(sizeof(mk::TreesArgs) <= 4096, "the tree descriptors travel in the kernel arguments");

constexpr uint64_t kCounterBytes = 256;  // the container's arrival counter, a part of its own

// Layout of the workspace: the arrival words of every tree side by side (so
// one memset zeroes them and the counter behind them), the counter, then each
// STRUCT tree's gather / message / roots scratch.
struct Part {
    uint64_t T = 0;                          // work items
    uint64_t arrive = 0, arrive_bytes = 0;   // offset and size of the arrival words
    uint64_t scratch = 0, scratch_bytes = 0; // STRUCT: offset and size of the scratch
    StructTreeLayout L{};                    // STRUCT
};
struct WsLayout {
    Part part[MK_TREES_MAX];
    uint64_t counter = 0, total = 0;
};

// the host-checkable arguments of every tree (each kind's own) and the workspace layout; no device needed
int make_plan(const mk_tree_update* trees, uint32_t ntrees, WsLayout& P) {
    if (ntrees == 0 || ntrees > MK_TREES_MAX)
        return fail(MK_EINVAL, "%u trees in one call (1 .. %d)", ntrees, MK_TREES_MAX);
    if (!trees) return fail(MK_EINVAL, "null pointer");
    uint64_t pos = 0;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        Part& p = P.part[i];
        switch (t.kind) {
            case MK_TREE_LIST:
                TRY(list_tree_check_update(t.n_old, t.n_new, t.capacity, t.item_len, t.k_idx, UINT64_MAX));
                p.T = t.k_idx + (t.n_new - t.n_old);
                p.arrive_bytes = mk_ssz_list_tree_update_workspace_bytes(p.T);
                break;
            case MK_TREE_STRUCT: {
                TRY(struct_tree_layout(t.fields, t.nfields, t.item_len, p.L));
                TRY(struct_tree_check_update(p.L, t.n_old, t.n_new, t.capacity, t.k_idx, UINT64_MAX));
                p.T = t.k_idx + (t.n_new - t.n_old);
                const uint64_t all = struct_tree_update_ws(p.L, p.T, &p.arrive_bytes);
                p.scratch_bytes = all - p.arrive_bytes;
                break;
            }
            case MK_TREE_BYTES:
                TRY(bytes_tree_check_update(t.n_old, t.n_new, t.capacity, t.item_len, t.k_idx, UINT64_MAX));
                p.T = t.k_idx + (t.n_new - t.n_old);
                p.arrive_bytes = mk_ssz_bytes_list_tree_update_workspace_bytes(p.T, t.item_len);
                break;
            default:
                return fail(MK_EINVAL, "tree %u: unknown kind %u", i, t.kind);
        }
        p.arrive = pos;
        pos += p.arrive_bytes;  // every part is a multiple of 256 B
    }
    P.counter = pos;
    pos += kCounterBytes;
    for (uint32_t i = 0; i < ntrees; ++i) {
        P.part[i].scratch = pos;
        pos += P.part[i].scratch_bytes;
    }
    P.total = pos;
    return MK_OK;
}

// the container's arguments; *nparts: the trees that take part in it
int check_container(const mk_tree_update* trees, uint32_t ntrees, uint32_t container_len, uint32_t* nparts) {
    if (container_len > MK_CONTAINER_MAX)
        return fail(MK_EINVAL, "container of %u bytes (limit %d)", container_len, MK_CONTAINER_MAX);
    uint32_t n = 0;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const uint32_t off = trees[i].container_off;
        if (off == MK_NO_CONTAINER) continue;
        if (off % 4) return fail(MK_EINVAL, "tree %u: container offset %u not 4-byte aligned", i, off);
        if ((uint64_t)off + 32 > container_len)
            return fail(MK_EINVAL, "tree %u: root at offset %u beyond the %u-byte container", i, off, container_len);
        for (uint32_t j = 0; j < i; ++j) {
            const uint32_t o = trees[j].container_off;
            if (o != MK_NO_CONTAINER && off < o + 32 && o < off + 32)
                return fail(MK_EINVAL, "trees %u and %u: roots overlap in the container", j, i);
        }
        ++n;
    }
    if (container_len && n == 0) return fail(MK_EINVAL, "a container no tree takes part in");
    *nparts = n;
    return MK_OK;
}

// every pointer: each kind's own checks, and d_level0 against the kind
int check_ptrs(const mk_tree_update* trees, uint32_t ntrees, const void* d_container, uint32_t container_len,
               const void* d_container_root32, const void* d_ws) {
    if (!d_ws || ((uintptr_t)d_ws % 16)) return fail(MK_EINVAL, "null or misaligned (16 B) workspace");
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        if (t.kind == MK_TREE_LIST) {
            if (t.d_level0) return fail(MK_EINVAL, "tree %u: a list tree has no d_level0", i);
            TRY(list_tree_check_ptrs(t.d_items, t.n_new, t.capacity, t.item_len, t.d_levels, t.d_root32, d_ws));
        } else if (t.kind == MK_TREE_STRUCT) {
            if (!t.d_level0) return fail(MK_EINVAL, "tree %u: null d_level0 (the struct roots)", i);
            TRY(struct_tree_check_ptrs(t.d_items, t.n_new, t.capacity, t.d_level0, t.d_levels, t.d_root32, d_ws));
            if ((uintptr_t)t.d_values % 4) return fail(MK_EINVAL, "tree %u: new records not 4-byte aligned", i);
        } else {
            if (!t.d_level0) return fail(MK_EINVAL, "tree %u: null d_level0 (the element digests)", i);
            TRY(bytes_tree_check_ptrs(t.d_items, t.n_new, t.capacity, t.d_level0, t.d_levels, t.d_root32, d_ws));
        }
        if (t.k_idx && (!t.d_idx || ((uintptr_t)t.d_idx % 8)))
            return fail(MK_EINVAL, "tree %u: null or misaligned index array", i);
    }
    if (container_len && (!d_container || !d_container_root32 || ((uintptr_t)d_container % 4) ||
                          ((uintptr_t)d_container_root32 % 4)))
        return fail(MK_EINVAL, "null or misaligned (4 B) container or container root");
    return MK_OK;
}

int launch(const mk_tree_update* trees, uint32_t ntrees, const WsLayout& P, void* d_container, uint32_t container_len,
           uint32_t nparts, void* d_container_root32, void* d_ws, hipStream_t st) {
    uint8_t* ws = (uint8_t*)d_ws;
    HIPCHK(hipMemsetAsync(ws, 0, P.counter + (container_len ? kCounterBytes : 0), st));
    mk::TreesArgs g{};
    uint64_t blocks = 1;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        const Part& p = P.part[i];
        const void* level0 = t.d_level0;
        uint32_t len0 = 32;
        if (t.kind == MK_TREE_LIST) {
            if (t.d_values)
                TRY(list_tree_scatter(t.d_items, t.d_idx, t.k_idx, t.n_old, t.n_new - t.n_old, t.item_len, t.d_values,
                                      st));
            level0 = t.d_items;
            len0 = t.item_len;
        } else if (t.kind == MK_TREE_STRUCT) {
            TRY(struct_tree_stage0(p.L, t.d_items, t.n_old, t.n_new, t.d_level0, t.d_idx, t.k_idx, t.d_values,
                                   ws + p.scratch, st));
        } else {
            TRY(bytes_tree_stage0(t.d_items, t.n_old, t.n_new, t.item_len, t.d_level0, t.d_idx, t.k_idx, t.d_values,
                                  st));
        }
        g.t[i] = list_tree_args(level0, t.d_levels, t.d_idx, t.k_idx, t.n_old, t.n_new, t.capacity, len0, t.d_root32,
                                ws + p.arrive);
        g.coff[i] = container_len ? t.container_off : MK_NO_CONTAINER;
        blocks = std::max(blocks, ceil_div(2 * p.T, 256));
    }
    if (container_len) {
        g.container = (uint8_t*)d_container;
        g.counter = (uint32_t*)(ws + P.counter);
        g.container_root = (uint32_t*)d_container_root32;
        g.container_len = container_len;
        g.nparts = nparts;
    }
    hipLaunchKernelGGL(mk::k_trees_update, dim3((uint32_t)blocks, ntrees), dim3(256), 0, st, g);
    return launched();
}

}  // namespace

extern "C" {

uint64_t mk_ssz_trees_update_workspace_bytes(const mk_tree_update* trees, uint32_t ntrees) {
    Scope S(nullptr, false);
    WsLayout P;
    if (make_plan(trees, ntrees, P) != MK_OK) return 0;
    return P.total;
}

// Every argument check, the pointers included, comes before the stream's
// device is looked up: a bad call is MK_EINVAL / MK_ENOMEM on any machine.
int mk_dev_ssz_trees_update(mk_call* call, const mk_tree_update* trees, uint32_t ntrees, void* d_container,
                            uint32_t container_len, void* d_container_root32, void* d_ws, uint64_t ws_bytes,
                            void* stream) {
    Scope S(call);
    WsLayout P;
    uint32_t nparts = 0;
    int rc = make_plan(trees, ntrees, P);
    if (!rc) rc = check_container(trees, ntrees, container_len, &nparts);
    if (!rc && ws_bytes < P.total) rc = fail(MK_ENOMEM, "workspace too small");
    if (!rc) rc = check_ptrs(trees, ntrees, d_container, container_len, d_container_root32, d_ws);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = launch(trees, ntrees, P, d_container, container_len, nparts, d_container_root32, d_ws,
                    (hipStream_t)stream);
    return S.done(rc);
}

}  // extern "C"
