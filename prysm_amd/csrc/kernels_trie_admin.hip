// Roll back, fork point, audit and copy of the resident deposit trie (the rules:
// trie_admin.hpp).  A part of the one kernel translation unit: merkle_kernels.hip includes it after
// kernels_tree.hip, whose audit helpers it uses.  Built as an object of its own it would emit other code for the
// same text ("Kernel files").
#ifndef MK_KERNEL_UNIT
#error "kernels_trie_admin.hip is built through merkle_kernels.hip"
#endif
#include "hash_dev.hpp"
#include "trie_admin.hpp"

namespace mk {

namespace {

// first node of level L of a level array of capacity cap: one lane per level
__device__ __forceinline__ uint64_t ta_lane_off(uint64_t cap, uint32_t L) {
    uint64_t off = 0, capd = cap;
    for (uint32_t d = 0; d < L; ++d) {
        off += capd;
        capd = (capd + 1) / 2;
    }
    return off;
}

}  // namespace

// Roll back to c <= count on one wave.  The straddling nodes E_d are the chain
// of k_trie_branches_at's wave 0, in the same spread form with the left
// siblings prefetched into LDS (lane d loads level d's) -- a copy of that
// chain, so that kernel stays as it is; here every E_d is also stored, at node
// (c - 1) >> d of level d, and E_depth is the root.  Every load of the level
// array comes before the barrier, every store after it, and no stored node is
// a node the chain reads: the siblings lie one to the left of the path.
__global__ __launch_bounds__(64) void k_trie_truncate(uint4* levels, uint64_t cap, uint64_t count, uint64_t c,
                                                      uint32_t depth, uint4* root_out) {
    __shared__ uint4 sib[64][2];    // level d's left sibling
    __shared__ uint64_t lvoff[64];  // first node of level d
    const uint32_t L = threadIdx.x;
    const uint64_t last = c - 1;
    const uint32_t d0 = ta_chain_first(count, c, depth);  // wave-uniform; 0: no level straddles
    uint2* lv2 = reinterpret_cast<uint2*>(levels);
    if (L <= depth) {
        const uint64_t off = ta_lane_off(cap, L);
        lvoff[L] = off;
        if (d0 && L + 1 >= d0 && L < depth && ta_path_right(c, L)) {
            const uint64_t node = off + ta_path_node(c, L) - 1;
            sib[L][0] = levels[2 * node];
            sib[L][1] = levels[2 * node + 1];
        }
    }
    __syncthreads();
    if (d0 == 0) {  // the stored top node is the root; an empty trie's is 0^32, in both places
        if (L < 2u) {
            uint4 r = make_uint4(0, 0, 0, 0);
            if (c != 0)
                r = levels[2 * lvoff[depth] + L];
            else if (cap != 0)
                levels[2 * lvoff[depth] + L] = r;
            root_out[L] = r;
        }
        return;
    }
    const spread::LaneLH cst = spread::lane_consts_lh(L);
    const uint32_t ci = cst.i;
    uint32_t plo = 0u, phi = 0u;  // the path node's word ci on lanes ci < 4
    if (ci < 4u) {
        const uint2 v = lv2[4 * (lvoff[d0 - 1] + (last >> (d0 - 1))) + ci];
        plo = v.x;
        phi = v.y;
    }
    for (uint32_t d = d0 - 1; d < depth; ++d) {
        const bool right = ((last >> d) & 1u) != 0;  // wave-uniform
        // path words moved to Keccak lanes 4..7 (GPU lanes 0..3 hold 0..3)
        const uint32_t src = 4u * ((ci - 4u) & 3u);
        const uint32_t mlo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)plo);
        const uint32_t mhi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)phi);
        uint32_t lo = 0u, hi = 0u;
        if (ci < 4u) {
            if (right) {
                const uint4 h = sib[d][ci >> 1];
                lo = (ci & 1u) ? h.z : h.x;
                hi = (ci & 1u) ? h.w : h.y;
            } else {
                lo = plo;
                hi = phi;
            }
        } else if (ci < 8u && right) {
            lo = mlo;
            hi = mhi;
        } else if (ci == 8u) {
            lo = 1u;
        }
        if (ci == 16u) hi = 0x80000000u;
        spread::keccak_f_lh(lo, hi, cst);
        plo = lo;
        phi = hi;
        if (L < 4u) lv2[4 * (lvoff[d + 1] + (last >> (d + 1))) + L] = make_uint2(lo, hi);
    }
    if (L < 4u) reinterpret_cast<uint2*>(root_out)[L] = make_uint2(plo, phi);
}

// Fork point of two tries on one wave.  Lane d <= depth takes the subtree of
// bit d of m = min(count_a, count_b) and compares its two stored roots; the
// highest differing lane is the leftmost differing subtree.  Then one step
// per level: lanes 0..7 load the 16-B halves of both children of both tries
// (lane = trie * 4 + child * 2 + half) and lane l < 4 compares with lane l + 4.
__global__ __launch_bounds__(64) void k_trie_fork_point(const uint4* __restrict__ a, uint64_t cap_a, uint64_t count_a,
                                                        const uint4* __restrict__ b, uint64_t cap_b, uint64_t count_b,
                                                        uint32_t depth, uint64_t* __restrict__ out) {
    __shared__ uint64_t off_a[64], off_b[64];
    const uint32_t L = threadIdx.x;
    const uint64_t m = count_a < count_b ? count_a : count_b;
    bool ne = false;
    if (L <= depth) {
        const uint64_t oa = ta_lane_off(cap_a, L), ob = ta_lane_off(cap_b, L);
        off_a[L] = oa;
        off_b[L] = ob;
        if (ta_fork_has(m, L)) {
            const uint64_t j = ta_fork_sub(m, L);
            ne = audit_differs(a[2 * (oa + j)], a[2 * (oa + j) + 1], b[2 * (ob + j)], b[2 * (ob + j) + 1]);
        }
    }
    __syncthreads();
    const uint64_t mask = __ballot(ne);
    uint64_t res = m;
    if (mask) {  // wave-uniform
        uint32_t d = 63u - (uint32_t)__builtin_clzll(mask);
        uint64_t j = ta_fork_sub(m, d);
        for (; d > 0; --d) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (L < 8u) {
                const uint64_t node = (L < 4u ? off_a[d - 1] : off_b[d - 1]) + 2 * j + ((L >> 1) & 1u);
                v = (L < 4u ? a : b)[2 * node + (L & 1u)];
            }
            const uint32_t x = (v.x ^ (uint32_t)__shfl_xor((int)v.x, 4)) | (v.y ^ (uint32_t)__shfl_xor((int)v.y, 4)) |
                               (v.z ^ (uint32_t)__shfl_xor((int)v.z, 4)) | (v.w ^ (uint32_t)__shfl_xor((int)v.w, 4));
            const uint64_t dm = __ballot(x != 0u);
            j = (dm & 3ull) ? 2 * j : 2 * j + 1;  // the left child differs: left; else right
        }
        res = j;
    }
    if (L == 0) *out = res;
}

// Audit: one work item per live node of level 1 .. depth and one for the
// root, numbered level after level (trie_admin.hpp), a bounded grid striding
// over them with one Keccak state per lane: K(left || right) through hash_pair
// against the stored node.  A level's first item and its two offsets are
// per-workgroup LDS, a lane per level.  Nothing depends on another lane, so
// the narrow top levels are just more lanes.  A mismatch is the rare path of
// the list-tree audit (audit_mismatch: the count and the smallest key, two
// agent-scope atomics); nothing else is written.
__global__ __launch_bounds__(kAuditThreads, 4) void k_trie_audit(const uint4* __restrict__ levels, uint64_t cap,
                                                                  uint64_t count, uint32_t depth,
                                                                  const uint4* __restrict__ root,
                                                                  AuditReport* report) {
    __shared__ uint64_t sfirst[66];  // first item of slot s (level s + 1; depth: the root; depth + 1: the total)
    __shared__ uint64_t lvoff[64];
    const uint32_t T = threadIdx.x;
    if (T <= depth) lvoff[T] = ta_lane_off(cap, T);
    if (T >= 64u && T - 64u <= depth + 1) sfirst[T - 64u] = ta_audit_first(count, depth, T - 64u);
    __syncthreads();
    const uint64_t total = sfirst[depth + 1];
    const uint64_t stride = (uint64_t)gridDim.x * kAuditThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kAuditThreads + T; q < total; q += stride) {
        uint32_t lo = 0, hi = depth;  // the last slot that starts at or below q
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (sfirst[mid] <= q)
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint4 z = make_uint4(0, 0, 0, 0);
        if (lo == depth) {  // the root against the top node (0^32 for an empty trie)
            uint4 t0 = z, t1 = z;
            if (count) {
                t0 = levels[2 * lvoff[depth]];
                t1 = levels[2 * lvoff[depth] + 1];
            }
            if (audit_differs(t0, t1, root[0], root[1])) audit_mismatch(report, kAuditRoot, 0);
            continue;
        }
        const uint32_t d = lo + 1;
        const uint64_t j = q - sfirst[lo];
        const uint4* ch = levels + 2 * (lvoff[d - 1] + 2 * j);
        const uint4 l0 = ch[0], l1 = ch[1];
        uint4 r0 = z, r1 = z;
        if (ta_audit_right(count, d, j)) {
            r0 = ch[2];
            r1 = ch[3];
        }
        uint4 d0, d1;
        hash_pair(l0, l1, r0, r1, false, d0, d1);
        const uint4* node = levels + 2 * (lvoff[d] + j);
        if (audit_differs(d0, d1, node[0], node[1])) audit_mismatch(report, d, j);
    }
}

// Copy: the 16-byte halves of every live node of level 0 .. depth from the
// layout of cap_src into that of cap_dst, then the root's two; a bounded grid
// strides over the pieces, every thread writes only its own.
__global__ __launch_bounds__(kCopyThreads) void k_trie_copy(const uint4* __restrict__ src, uint64_t cap_src,
                                                            uint64_t count, uint4* __restrict__ dst, uint64_t cap_dst,
                                                            uint32_t depth, const uint4* __restrict__ src_root,
                                                            uint4* __restrict__ dst_root) {
    __shared__ uint64_t pfirst[66];  // first piece of level d (depth + 1: the levels' pieces)
    __shared__ uint64_t soff[64], doff[64];
    const uint32_t T = threadIdx.x;
    if (T <= depth) {
        soff[T] = ta_lane_off(cap_src, T);
        doff[T] = ta_lane_off(cap_dst, T);
    }
    if (T >= 64u && T - 64u <= depth + 1) pfirst[T - 64u] = ta_copy_first(count, T - 64u);
    __syncthreads();
    const uint64_t in_levels = pfirst[depth + 1], total = in_levels + (src_root ? 2 : 0);
    const uint64_t stride = (uint64_t)gridDim.x * kCopyThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kCopyThreads + T; q < total; q += stride) {
        if (q >= in_levels) {
            dst_root[q - in_levels] = src_root[q - in_levels];
            continue;
        }
        uint32_t lo = 0, hi = depth;  // the last level that starts at or below q
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (pfirst[mid] <= q)
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint64_t r = q - pfirst[lo];
        dst[2 * doff[lo] + r] = src[2 * soff[lo] + r];
    }
}

}  // namespace mk
