// Resident trees audited on the device: the device entry
// mk_dev_ssz_trees_audit -- every argument check, then a linear chain: the
// reports cleared, level 0 of the struct / bytes trees in pieces through the
// struct-roots / digest launches with a compare launch behind each, the one
// launch of k_trees_audit over every node of level >= 1, the roots and the
// container, the keys unpacked.  The handle calls (mk_*_tree_audit,
// mk_tree_set_audit) are tree_handle.cpp's and tree_set_api.cpp's over the same
// three functions; the work-item map is tree_audit.hpp's.
#include "runtime.hpp"
#include "tree_audit.hpp"

using namespace mk;
using namespace mk::rt;

static_assert(MK_TREES_MAX == mk::kTreesMax, "MK_TREES_MAX and the kernel's descriptor table differ");
static_assert(MK_AUDIT_ROOT == mk::kAuditRoot && MK_AUDIT_CONTAINER == mk::kAuditContainer &&
                  MK_AUDIT_NONE == mk::kAuditNone,
              "the header's mismatch levels and tree_audit.hpp's differ");
static_assert(sizeof(mk_audit_report) == sizeof(mk::AuditReport) && sizeof(mk_audit_report) == 24,
              "mk_audit_report and the kernels' report differ");

namespace {

// Level 0 is hashed again in pieces of this many values: the workspace holds one piece's 32-B entries (and
// its struct messages) whatever n is.  A multiple of 16: a piece starts as aligned as the list does.  At 65536
// the audit of 2^20 validators was 32 launches of pieces too small to fill the chip and ran 1.21x its build
// (DESIGN.md §5n); 2^18 values are 8 MB of entries and four pieces for that registry.
constexpr uint64_t kAuditPiece = 262144;
// Workgroups of k_trees_audit: compute-bound, about five workgroups of 256 are resident per CU beside 26 KB
// of LDS each; eight per CU give the dispatcher room, the rest of the items by grid stride.
constexpr uint64_t kAuditGridMax = 2048;

bool level0_kind(uint32_t kind) { return kind != MK_TREE_LIST; }
uint32_t len0_of(const mk_tree_audit& t) { return level0_kind(t.kind) ? 32u : t.item_len; }

uint64_t piece_msg_bytes(const StructTreeLayout& L, uint64_t m) { return L.fused ? 0 : align256(m * L.sp.msg_len); }

// workspace of one tree's level-0 check: a piece's messages (struct, not fused), then its 32-B entries
uint64_t tree_ws(const mk_tree_audit& t, const StructTreeLayout* L) {
    if (!level0_kind(t.kind) || t.n == 0) return 0;
    const uint64_t m = std::min<uint64_t>(t.n, kAuditPiece);
    return (L ? piece_msg_bytes(*L, m) : 0) + align256(32 * m);
}

int check_tree(const mk_tree_audit& t, uint32_t i, const StructTreeLayout* given, AuditCall& c) {
    if (t.kind != MK_TREE_LIST && t.kind != MK_TREE_STRUCT && t.kind != MK_TREE_BYTES)
        return fail(MK_EINVAL, "tree %u: unknown kind %u", i, t.kind);
    if (t.item_len == 0) return fail(MK_EINVAL, "tree %u: item_len == 0", i);
    if (t.kind == MK_TREE_LIST && t.item_len > kBranchItemMax)
        return fail(MK_EINVAL, "tree %u: item_len %u above %u", i, t.item_len, kBranchItemMax);
    if (t.item_len > (1u << 30)) return fail(MK_EINVAL, "tree %u: item_len %u above 2^30", i, t.item_len);
    if (t.n > t.capacity)
        return fail(MK_EINVAL, "tree %u: %llu values > capacity %llu", i, (unsigned long long)t.n,
                    (unsigned long long)t.capacity);
    if (t.capacity > UINT64_MAX / std::max<uint32_t>(t.item_len, 32))
        return fail(MK_EINVAL, "tree %u: capacity * item_len overflows", i);
    const bool l0 = level0_kind(t.kind);
    if (!l0 && t.d_level0) return fail(MK_EINVAL, "tree %u: a level 0 for a list tree", i);
    if (t.kind == MK_TREE_STRUCT) {
        if (given) {
            c.L[i] = given;
        } else {
            if (!t.fields || !t.nfields) return fail(MK_EINVAL, "tree %u: a struct tree without its field layout", i);
            StructTreeLayout L;
            TRY(struct_tree_layout(t.fields, t.nfields, t.item_len, L));
            c.own.push_back(L);  // reserved by the caller: the addresses stay
            c.L[i] = &c.own.back();
        }
    } else if (t.fields || t.nfields) {
        return fail(MK_EINVAL, "tree %u: a field layout for a tree of kind %u", i, t.kind);
    }
    if (!t.d_root32) return fail(MK_EINVAL, "tree %u: null pointer (root)", i);
    if (t.n && !t.d_items) return fail(MK_EINVAL, "tree %u: null pointer (values)", i);
    if (t.n && l0 && !t.d_level0) return fail(MK_EINVAL, "tree %u: null pointer (level 0)", i);
    const AuditShape b = audit_shape(t.n, t.capacity, len0_of(t));
    if (b.D && !t.d_levels) return fail(MK_EINVAL, "tree %u: null level array", i);
    if (((uintptr_t)t.d_level0 | (uintptr_t)t.d_levels | (uintptr_t)t.d_root32) % 16)
        return fail(MK_EINVAL, "tree %u: level 0, level array or root misaligned (16 B)", i);
    if (t.kind == MK_TREE_STRUCT && (uintptr_t)t.d_items % 4)
        return fail(MK_EINVAL, "tree %u: records misaligned (4 B)", i);
    c.items += audit_items(b) + (l0 ? t.n : 0);
    c.ws = std::max(c.ws, tree_ws(t, c.L[i]));
    return MK_OK;
}

}  // namespace

namespace mk::rt {

int trees_audit_prepare(const mk_tree_audit* trees, uint32_t ntrees, const StructTreeLayout* const* layouts,
                        uint32_t container_len, AuditCall& c) {
    if (ntrees == 0 || ntrees > MK_TREES_MAX)
        return fail(MK_EINVAL, "%u trees in one call (1 .. %d)", ntrees, MK_TREES_MAX);
    if (!trees) return fail(MK_EINVAL, "null pointer");
    if (container_len > MK_CONTAINER_MAX)
        return fail(MK_EINVAL, "container of %u bytes (limit %d)", container_len, MK_CONTAINER_MAX);
    c.own.reserve(ntrees);
    for (uint32_t i = 0; i < ntrees; ++i) {
        TRY(check_tree(trees[i], i, layouts ? layouts[i] : nullptr, c));
        const uint32_t o = trees[i].container_off;
        if (o == MK_NO_CONTAINER) continue;
        if (container_len == 0) return fail(MK_EINVAL, "tree %u: a container offset without a container", i);
        if (o % 4) return fail(MK_EINVAL, "tree %u: container offset %u not 4-byte aligned", i, o);
        if ((uint64_t)o + 32 > container_len)
            return fail(MK_EINVAL, "tree %u: root at offset %u beyond the %u-byte container", i, o, container_len);
        for (uint32_t j = 0; j < i; ++j) {
            const uint32_t p = trees[j].container_off;
            if (p != MK_NO_CONTAINER && o < p + 32 && p < o + 32)
                return fail(MK_EINVAL, "tree %u: its root overlaps tree %u's in the container", i, j);
        }
    }
    if (container_len) c.items += 1 + ntrees;
    if (c.items >= kMaxWork)
        return fail(MK_EINVAL, "%llu work items in one audit (limit 2^31 - 1)", (unsigned long long)c.items);
    return MK_OK;
}

int trees_audit_check(const mk_tree_audit* trees, uint32_t ntrees, const AuditCall& c, const void* d_container,
                      uint32_t container_len, const void* d_container_root32, const void* d_reports, const void* d_ws,
                      uint64_t ws_bytes) {
    (void)trees, (void)ntrees;
    if (container_len && (!d_container || !d_container_root32)) return fail(MK_EINVAL, "null pointer (container)");
    if (container_len && ((uintptr_t)d_container | (uintptr_t)d_container_root32) % 4)
        return fail(MK_EINVAL, "container or container root misaligned (4 B)");
    if (!d_reports) return fail(MK_EINVAL, "null pointer (reports)");
    if ((uintptr_t)d_reports % 8) return fail(MK_EINVAL, "reports misaligned (8 B)");
    if (c.ws && !d_ws) return fail(MK_EINVAL, "null pointer (workspace)");
    if (c.ws && (uintptr_t)d_ws % 16) return fail(MK_EINVAL, "workspace misaligned (16 B)");
    if (ws_bytes < c.ws)
        return fail(MK_ENOMEM, "workspace too small: %llu of %llu bytes", (unsigned long long)ws_bytes,
                    (unsigned long long)c.ws);
    return MK_OK;
}

int trees_audit_launch(const mk_tree_audit* trees, uint32_t ntrees, const AuditCall& c, const void* d_container,
                       uint32_t container_len, const void* d_container_root32, void* d_reports, void* d_ws,
                       hipStream_t st) {
    mk::AuditReport* reports = (mk::AuditReport*)d_reports;
    hipLaunchKernelGGL(mk::k_audit_reports, dim3(1), dim3(64), 0, st, reports, ntrees + 1, 0u);
    TRY(launched());
    mk::TreesAuditArgs a{};
    for (uint32_t i = 0; i < ntrees; ++i) {
        const mk_tree_audit& t = trees[i];
        const bool l0 = level0_kind(t.kind);
        mk::AuditTree& T = a.t[i];
        T.level0 = (const uint8_t*)(l0 ? t.d_level0 : t.d_items);
        T.levels = (const uint8_t*)t.d_levels;
        T.root = (const uint8_t*)t.d_root32;
        T.n = t.n, T.capacity = t.capacity;
        T.len0 = len0_of(t);
        T.coff = container_len ? t.container_off : MK_NO_CONTAINER;
        // level 0: a piece's entries hashed again into the workspace, then compared with the stored ones
        for (uint64_t first = 0; l0 && first < t.n; first += kAuditPiece) {
            const uint64_t m = std::min<uint64_t>(kAuditPiece, t.n - first);
            const uint8_t* vals = (const uint8_t*)t.d_items + first * t.item_len;
            uint8_t* fresh = (uint8_t*)d_ws;
            if (t.kind == MK_TREE_STRUCT) {
                fresh += piece_msg_bytes(*c.L[i], std::min<uint64_t>(t.n, kAuditPiece));
                TRY(struct_launch_roots(vals, m, c.L[i]->sp, d_ws, fresh, st));
            } else {
                TRY(launch_elem_digests(vals, m, t.item_len, fresh, st));
            }
            hipLaunchKernelGGL(mk::k_audit_compare, dim3((uint32_t)ceil_div(m, 256)), dim3(256), 0, st,
                               (const uint4*)fresh, (const uint4*)t.d_level0, first, m, reports + i);
            TRY(launched());
        }
    }
    a.container = container_len ? (const uint8_t*)d_container : nullptr;
    a.container_root = (const uint8_t*)d_container_root32;
    a.reports = reports;
    a.container_len = container_len;
    a.ntrees = ntrees;
    uint64_t items = container_len ? 1 + ntrees : 0;
    for (uint32_t i = 0; i < ntrees; ++i) items += audit_items(audit_shape(trees[i].n, trees[i].capacity, len0_of(trees[i])));
    const uint64_t grid = std::min<uint64_t>(ceil_div(items, mk::kAuditThreads), kAuditGridMax);
    hipLaunchKernelGGL(mk::k_trees_audit, dim3((uint32_t)grid), dim3(mk::kAuditThreads), 0, st, a);
    TRY(launched());
    hipLaunchKernelGGL(mk::k_audit_reports, dim3(1), dim3(64), 0, st, reports, ntrees + 1, 1u);
    return launched();
}

}  // namespace mk::rt

extern "C" {

uint64_t mk_ssz_trees_audit_workspace_bytes(const mk_tree_audit* trees, uint32_t ntrees) {
    Scope S(nullptr, false);
    AuditCall c;
    uint32_t clen = 0;  // the offsets are the call's to refuse: any message long enough lets them pass here
    for (uint32_t i = 0; trees && i < ntrees && i < MK_TREES_MAX; ++i)
        if (trees[i].container_off != MK_NO_CONTAINER) clen = MK_CONTAINER_MAX;
    if (trees_audit_prepare(trees, ntrees, nullptr, clen, c) != MK_OK) return 0;
    return c.ws;
}

// Every argument check comes before the stream's device is looked up: a bad
// call is MK_EINVAL / MK_ENOMEM on any machine.  Nothing uploaded or allocated,
// no synchronise: capturable.
int mk_dev_ssz_trees_audit(mk_call* call, const mk_tree_audit* trees, uint32_t ntrees, const void* d_container,
                           uint32_t container_len, const void* d_container_root32, void* d_reports, void* d_ws,
                           uint64_t ws_bytes, void* stream) {
    Scope S(call);
    AuditCall c;
    int rc = trees_audit_prepare(trees, ntrees, nullptr, container_len, c);
    if (!rc) rc = trees_audit_check(trees, ntrees, c, d_container, container_len, d_container_root32, d_reports, d_ws, ws_bytes);
    if (!rc) rc = bind_stream((hipStream_t)stream);
    if (!rc)
        rc = trees_audit_launch(trees, ntrees, c, d_container, container_len, d_container_root32, d_reports, d_ws,
                                (hipStream_t)stream);
    return S.done(rc);
}

}  // extern "C"
