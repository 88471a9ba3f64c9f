// Several device-resident trees in one call: every
// tree's stage 0, then all the climbs, the trees of one chunk and the hash of
// the struct that holds them in ONE launch (k_trees_update) --
// mk_dev_ssz_trees_update.  Stage 0 is either the launchers of each tree's own
// update entry point (list_tree_api, struct_tree_api, bytes_tree_api) one tree
// after the other, or batched across the trees (k_trees_stage0).
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

namespace {

static_assert(MK_TREES_MAX == mk::kTreesMax, "MK_TREES_MAX and the kernel's descriptor table differ");
static_assert(sizeof(mk::TreesArgs) <= 4096, "the tree descriptors travel in the kernel arguments");

constexpr uint64_t kCounterBytes = 256;  // the container's arrival counter, a part of its own

// Stage 0 batched across the trees (1) or tree by tree (0); the result is the
// same byte for byte.  The shipped choice and its measurement: DESIGN.md §5j
// (tools/state_tree_probe.py on both builds, profiles/tree_set/stage0_ab.json).
#ifndef MK_TREES_STAGE0_BATCHED
#define MK_TREES_STAGE0_BATCHED 1
#endif

static_assert(sizeof(mk::Stage0Args) <= 4096, "the stage-0 segments travel in the kernel arguments");
static_assert(mk::kStage0SegsMax >= 2 * MK_TREES_MAX, "a scatter and a digest segment per tree");

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
// (lists: the index arrays and the staged values too -- a restore reads neither)
int check_ptrs(const mk_tree_update* trees, uint32_t ntrees, const void* d_container, uint32_t container_len,
               const void* d_container_root32, const void* d_ws, bool lists = true) {
    if (!d_ws || ((uintptr_t)d_ws % 16)) return fail(MK_EINVAL, "null or misaligned (16 B) workspace");
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        if (t.kind == MK_TREE_LIST) {
            if (t.d_level0) return fail(MK_EINVAL, "tree %u: a list tree has no d_level0", i);
            TRY(list_tree_check_ptrs(t.d_items, t.n_new, t.capacity, t.item_len, t.d_levels, t.d_root32, d_ws));
        } else if (t.kind == MK_TREE_STRUCT) {
            if (!t.d_level0) return fail(MK_EINVAL, "tree %u: null d_level0 (the struct roots)", i);
            TRY(struct_tree_check_ptrs(t.d_items, t.n_new, t.capacity, t.d_level0, t.d_levels, t.d_root32, d_ws));
            if (lists && (uintptr_t)t.d_values % 4) return fail(MK_EINVAL, "tree %u: new records not 4-byte aligned", i);
        } else {
            if (!t.d_level0) return fail(MK_EINVAL, "tree %u: null d_level0 (the element digests)", i);
            TRY(bytes_tree_check_ptrs(t.d_items, t.n_new, t.capacity, t.d_level0, t.d_levels, t.d_root32, d_ws));
        }
        if (lists && t.k_idx && (!t.d_idx || ((uintptr_t)t.d_idx % 8)))
            return fail(MK_EINVAL, "tree %u: null or misaligned index array", i);
    }
    if (container_len && (!d_container || !d_container_root32 || ((uintptr_t)d_container % 4) ||
                          ((uintptr_t)d_container_root32 % 4)))
        return fail(MK_EINVAL, "null or misaligned (4 B) container or container root");
    return MK_OK;
}

// one scatter segment (k_list_tree_scatter's rule and its choice of the unit)
mk::Stage0Seg scatter_seg(void* dst, const void* vals, const mk_tree_update& t, uint32_t item_len, uint64_t* blocks) {
    mk::Stage0Seg s{};
    s.dst = (uint8_t*)dst;
    s.vals = (const uint8_t*)vals;
    s.idx = t.d_idx;
    s.k_idx = t.k_idx;
    s.n_old = t.n_old;
    s.n_app = t.n_new - t.n_old;
    s.item_len = item_len;
    s.mode = item_len % 8 == 0 && ((uintptr_t)dst % 8) == 0 && ((uintptr_t)vals % 8) == 0 ? 8 : 1;
    *blocks = std::max(*blocks, ceil_div((s.k_idx + s.n_app) * (item_len / s.mode), 256));
    return s;
}

int launch_stage0(const mk::Stage0Args& a, uint32_t nseg, uint64_t blocks, hipStream_t st) {
    if (nseg == 0) return MK_OK;
    if (blocks > 0x7fffffffull) return fail(MK_EINVAL, "%llu blocks of stage 0", (unsigned long long)blocks);
    hipLaunchKernelGGL(mk::k_trees_stage0, dim3((uint32_t)std::max<uint64_t>(blocks, 1), nseg), dim3(256), 0, st, a);
    return launched();
}

// Stage 0 of every tree, batched: ONE launch that scatters every tree's values
// and digests every BYTES tree's work items from the staged values, the
// struct-roots launch of each STRUCT tree (from its staged values), ONE launch
// that scatters every STRUCT tree's new roots.  A tree of one chunk has no
// levels: every root or digest again from the scattered list, as in
// struct_tree_stage0 / bytes_tree_stage0.  A tree with d_values == NULL (its
// values are in place) keeps its own stage 0.
int stage0_batched(const mk_tree_update* trees, uint32_t ntrees, const WsLayout& P, uint8_t* ws, hipStream_t st) {
    mk::Stage0Args a{}, b{};
    uint32_t na = 0, nb = 0;
    uint64_t blocks_a = 1, blocks_b = 1;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        if (!t.d_values) continue;
        a.s[na++] = scatter_seg(t.d_items, t.d_values, t, t.item_len, &blocks_a);
        if (t.kind == MK_TREE_BYTES && ceil_div(t.n_new, 4) > 1) {
            mk::Stage0Seg& s = a.s[na++];
            s = a.s[na - 2];
            s.dst = (uint8_t*)t.d_level0;
            s.mode = t.item_len == 32 && ((uintptr_t)t.d_values % 16) == 0 ? mk::kStage0Digest32 : mk::kStage0Digest;
            blocks_a = std::max(blocks_a, ceil_div(s.k_idx + s.n_app, 256));
        }
    }
    TRY(launch_stage0(a, na, blocks_a, st));
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        const Part& p = P.part[i];
        if (t.kind == MK_TREE_STRUCT && t.d_values) {
            const void* roots = nullptr;
            TRY(struct_tree_stage0_roots(p.L, t.d_items, t.n_new, p.T, t.d_values, t.d_level0, ws + p.scratch, &roots,
                                         st));
            if (roots) b.s[nb++] = scatter_seg(t.d_level0, roots, t, 32, &blocks_b);
        } else if (t.kind == MK_TREE_STRUCT) {
            TRY(struct_tree_stage0(p.L, t.d_items, t.n_old, t.n_new, t.d_level0, t.d_idx, t.k_idx, nullptr,
                                   ws + p.scratch, st));
        } else if (t.kind == MK_TREE_BYTES && t.d_values) {
            if (ceil_div(t.n_new, 4) <= 1) TRY(launch_elem_digests(t.d_items, t.n_new, t.item_len, t.d_level0, st));
        } else if (t.kind == MK_TREE_BYTES) {
            TRY(bytes_tree_stage0(t.d_items, t.n_old, t.n_new, t.item_len, t.d_level0, t.d_idx, t.k_idx, nullptr, st));
        }
    }
    return launch_stage0(b, nb, blocks_b, st);
}

// each tree's own stage 0, one tree after the other
int stage0_per_tree(const mk_tree_update* trees, uint32_t ntrees, const WsLayout& P, uint8_t* ws, hipStream_t st) {
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        const Part& p = P.part[i];
        if (t.kind == MK_TREE_LIST) {
            if (t.d_values)
                TRY(list_tree_scatter(t.d_items, t.d_idx, t.k_idx, t.n_old, t.n_new - t.n_old, t.item_len, t.d_values,
                                      st));
        } else if (t.kind == MK_TREE_STRUCT) {
            TRY(struct_tree_stage0(p.L, t.d_items, t.n_old, t.n_new, t.d_level0, t.d_idx, t.k_idx, t.d_values,
                                   ws + p.scratch, st));
        } else {
            TRY(bytes_tree_stage0(t.d_items, t.n_old, t.n_new, t.item_len, t.d_level0, t.d_idx, t.k_idx, t.d_values,
                                  st));
        }
    }
    return MK_OK;
}

int launch(const mk_tree_update* trees, uint32_t ntrees, const WsLayout& P, void* d_container, uint32_t container_len,
           uint32_t nparts, void* d_container_root32, void* d_ws, hipStream_t st) {
    uint8_t* ws = (uint8_t*)d_ws;
    HIPCHK(hipMemsetAsync(ws, 0, P.counter + (container_len ? kCounterBytes : 0), st));
    if (MK_TREES_STAGE0_BATCHED)
        TRY(stage0_batched(trees, ntrees, P, ws, st));
    else
        TRY(stage0_per_tree(trees, ntrees, P, ws, st));
    mk::TreesArgs g{};
    uint64_t blocks = 1;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_update& t = trees[i];
        const Part& p = P.part[i];
        const bool list = t.kind == MK_TREE_LIST;
        g.t[i] = list_tree_args(list ? t.d_items : t.d_level0, t.d_levels, t.d_idx, t.k_idx, t.n_old, t.n_new,
                                t.capacity, list ? t.item_len : 32, t.d_root32, ws + p.arrive);
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

int check_all(const mk_tree_update* trees, uint32_t ntrees, WsLayout& P, const void* d_container,
              uint32_t container_len, uint32_t* nparts, const void* d_container_root32, const void* d_ws,
              uint64_t ws_bytes) {
    TRY(make_plan(trees, ntrees, P));
    TRY(check_container(trees, ntrees, container_len, nparts));
    if (ws_bytes < P.total) return fail(MK_ENOMEM, "workspace too small");
    return check_ptrs(trees, ntrees, d_container, container_len, d_container_root32, d_ws);
}

}  // namespace

namespace mk::rt {
int trees_update_workspace(const mk_tree_update* trees, uint32_t ntrees, uint64_t* bytes) {
    WsLayout P;
    TRY(make_plan(trees, ntrees, P));
    *bytes = P.total;
    return MK_OK;
}

int trees_update_check(const mk_tree_update* trees, uint32_t ntrees, const void* d_container, uint32_t container_len,
                       const void* d_container_root32, const void* d_ws16, bool lists) {
    WsLayout P;
    uint32_t nparts = 0;
    TRY(make_plan(trees, ntrees, P));
    TRY(check_container(trees, ntrees, container_len, &nparts));
    return check_ptrs(trees, ntrees, d_container, container_len, d_container_root32, d_ws16, lists);
}

int trees_update(const mk_tree_update* trees, uint32_t ntrees, void* d_container, uint32_t container_len,
                 void* d_container_root32, void* d_ws, uint64_t ws_bytes, hipStream_t st) {
    WsLayout P;
    uint32_t nparts = 0;
    TRY(check_all(trees, ntrees, P, d_container, container_len, &nparts, d_container_root32, d_ws, ws_bytes));
    return launch(trees, ntrees, P, d_container, container_len, nparts, d_container_root32, d_ws, st);
}
}  // namespace mk::rt

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
    int rc = check_all(trees, ntrees, P, d_container, container_len, &nparts, d_container_root32, d_ws, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = launch(trees, ntrees, P, d_container, container_len, nparts, d_container_root32, d_ws,
                    (hipStream_t)stream);
    return S.done(rc);
}

}  // extern "C"
