// Device-resident tree kernels of the MI355X Merkleization engine (gfx950 only).
// A part of the one kernel translation unit: merkle_kernels.hip includes it.  Built as an object of its own it would
// emit other code for the same text ("Kernel files").
#ifndef MK_KERNEL_UNIT
#error "kernels_tree.hip is built through merkle_kernels.hip"
#endif
#include "elem_dev.hpp"
#include "hash_dev.hpp"
#include "list_branch.hpp"
#include "spread3_dev.hpp"
#include "tree_audit.hpp"
#include "tree_compact.hpp"
#include "tree_copy.hpp"
#include "tree_diff.hpp"
#include "tree_journal.hpp"

namespace mk {

// ----------------------------------------------------------------------------
// Device-resident list tree: merkleHash (hash.go:194-239) of
// a list whose every level stays in HBM, re-hashed from the changed items
// only.  Level d >= 1 of the level array starts at node sum_{1<=i<d}
// ceil(cap_chunks / 2^i); level 0 is the item buffer itself.
//
// Work item t < T = k_idx + (n_new - n_old) is one dirty item: idx[t] for
// t < k_idx (ascending; an index >= n_old is read as the last old item, whose
// ancestors are then recomputed to the values they already have), after them
// the appended items n_old .. n_new - 1.  A lane pair (mk::ilv) serves a work
// item.  The pair of the FIRST work item under a level-1 node hashes that node
// from the item buffer and climbs; every node it finishes is stored, and it
// owns the work items [o, e) under that node.  Whether the sibling changed
// too is decided locally from the sorted list (item o - 1 for a left
// sibling, item e for a right one):
//   clean: the sibling (or the 0^128 pad when it does not exist) is read from
//          the level array, which an earlier launch wrote;
//   dirty: both children's pairs OR bit d into the arrival word of the
//          parent's first work item; the pair that finds the bit set (the
//          second to arrive) hashes the parent, the other one exits.
// No pair ever waits for another, so the launch completes whatever the grid
// size and dispatch order.  Ordering contract of the hand-off (the fence form,
// both sides): node stores -> __threadfence() (agent release) -> acq_rel
// agent-scope atomic OR; the second arriver: that atomic -> __threadfence()
// (agent acquire) -> loads of the sibling (agent-scope, so neither the
// compiler nor the CU's L1 can serve them from before the fence).
// The arrival words (one per work item, zeroed on the stream by the same
// call) are the caller's workspace: two trees never share one.
namespace {

__device__ __forceinline__ uint64_t lt_chunk(const ListTreeArgs& a, uint64_t t) {
    uint64_t x;
    if (t < a.k_idx) {
        x = a.idx[t];
        const uint64_t last = a.n_old ? a.n_old - 1 : 0;
        if (x > last) x = last;
    } else {
        x = a.n_old + (t - a.k_idx);
    }
    return x / a.per;
}

// first work item in [from, T] whose level-d node is above j (T: none); a
// gallop then a bisection, both bounded for any list contents
__device__ __forceinline__ uint64_t lt_upper(const ListTreeArgs& a, uint64_t from, uint64_t T, uint32_t d,
                                             uint64_t j) {
    uint64_t lo = from, hi = T, step = 1;
    while (lo < hi && step <= hi - lo) {
        const uint64_t probe = lo + step - 1;
        if ((lt_chunk(a, probe) >> d) > j) {
            hi = probe;
            break;
        }
        lo = probe + 1;
        step <<= 1;
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((lt_chunk(a, mid) >> d) > j)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// first work item in [0, upto] whose level-d node is at least j (item `upto` is one)
__device__ __forceinline__ uint64_t lt_lower(const ListTreeArgs& a, uint64_t upto, uint32_t d, uint64_t j) {
    uint64_t lo = 0, hi = upto, step = 1;
    while (lo < hi && step <= hi - lo) {
        const uint64_t probe = hi - step;
        if ((lt_chunk(a, probe) >> d) >= j) {
            hi = probe;
            step <<= 1;
        } else {
            lo = probe + 1;
            break;
        }
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((lt_chunk(a, mid) >> d) >= j)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// plain node j of a level -> this lane's parity words, agent-scope loads
__device__ __forceinline__ void lt_load_node(const uint32_t* lv, uint64_t j, uint32_t p, uint32_t (&w4)[4]) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(lv) + 4 * j;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t v = __hip_atomic_load(q + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w4[w] = ilv::to_ilv((uint32_t)v, (uint32_t)(v >> 32), p);
    }
}

// The climb of one tree by the lane pair (t, p) of work item t: the body of
// k_list_tree_update and of one tree's slice of k_trees_update.  True in the
// one pair that stored the root, whose parity words it leaves in r.
__device__ __forceinline__ bool lt_update(const ListTreeArgs& a, uint64_t t, uint32_t p, uint32_t (&r)[4]) {
    const uint64_t T = a.k_idx + (a.n_new - a.n_old);
    const uint64_t cb = (uint64_t)a.per * a.item_len, total = a.n_new * a.item_len;
    const uint64_t nch = (a.n_new + a.per - 1) / a.per;  // >= 2 (smaller lists: k_final_small, k_trees_update itself)
    uint64_t cnt = (nch + 1) >> 1, off = 0, capd = (a.cap_chunks + 1) >> 1;  // level d: nodes, offset, room
    uint32_t d = 1;
    uint32_t h[4];
    if (T == 0) {  // nothing changed: the root again, from the stored top node
        if (t != 0) return false;
        while (cnt > 1) {
            off += capd;
            capd = (capd + 1) >> 1;
            cnt = (cnt + 1) >> 1;
        }
        lt_load_node(a.levels + 8 * off, 0, p, h);
    } else {
        if (t >= T) return false;
        uint64_t j = lt_chunk(a, t) >> 1;
        if (t > 0 && (lt_chunk(a, t - 1) >> 1) == j) return false;  // not the first work item of its level-1 node
        uint64_t o = t, e = lt_upper(a, t + 1, T, 1, j);
        {  // level-1 node j: bytes [2 j cb, min(total, (2 j + 2) cb)), then 0^128 when chunk 2 j + 1 is absent
            const uint64_t b0 = 2 * j * cb;
            const bool pad = 2 * j + 1 >= nch;
            const uint64_t la = total - b0 < 2 * cb ? total - b0 : 2 * cb;
            const uint8_t* src = a.items + b0;
            if (la == 256 && !pad && (((uintptr_t)src) & 15u) == 0) {
                hash_window3(reinterpret_cast<const uint4*>(src), p, h);
            } else {
                uint4 d0, d1;
                sponge_generic(src, la, pad ? 128u : 0u, false, 0, d0, d1);
                h[0] = ilv::to_ilv(d0.x, d0.y, p);
                h[1] = ilv::to_ilv(d0.z, d0.w, p);
                h[2] = ilv::to_ilv(d1.x, d1.y, p);
                h[3] = ilv::to_ilv(d1.z, d1.w, p);
            }
        }
        for (;;) {
            uint32_t* lv = a.levels + 8 * off;
            store_node3(lv, j, false, p, h);
            if (cnt == 1) break;  // the top node
            const uint64_t sib = j ^ 1u;
            const bool right = (j & 1u) != 0;  // this node is the right child
            bool sib_dirty;
            if (right)
                sib_dirty = o > 0 && (lt_chunk(a, o - 1) >> d) == sib;
            else
                sib_dirty = e < T && (lt_chunk(a, e) >> d) == sib;
            if (sib_dirty) {
                if (right)
                    o = lt_lower(a, o - 1, d, sib);
                else
                    e = lt_upper(a, e + 1, T, d, sib);
                __threadfence();  // release: this pair's node stores before its arrival
                uint32_t second = 0;
                if (p == 0) {
                    const uint64_t old = __hip_atomic_fetch_or(a.arrive + o, 1ull << d, __ATOMIC_ACQ_REL,
                                                               __HIP_MEMORY_SCOPE_AGENT);
                    second = (uint32_t)(old >> d) & 1u;
                }
                second |= (uint32_t)__shfl_xor((int)second, 1);
                if (!second) return false;  // first to arrive: the sibling's pair hashes the parent
                __threadfence();           // acquire: the sibling's stores before the loads below
            }
            uint32_t s[4] = {0u, 0u, 0u, 0u}, q[4];
            const bool padded = sib >= cnt;  // only ever a missing RIGHT child
            if (!padded) lt_load_node(lv, sib, p, s);
            if (right)
                hash_pair3(s, h, false, p, q);
            else
                hash_pair3(h, s, padded, p, q);
#pragma unroll
            for (int w = 0; w < 4; ++w) h[w] = q[w];
            j >>= 1;
            off += capd;
            capd = (capd + 1) >> 1;
            cnt = (cnt + 1) >> 1;
            ++d;
        }
    }
    // root = K(top || le64(n) || 0^24) (hash.go:237-238)
    uint32_t m[4] = {ilv::to_ilv((uint32_t)a.n_new, (uint32_t)(a.n_new >> 32), p), 0u, 0u, 0u};
    hash_pair3(h, m, false, p, r);
    store_node3(a.root_out, 0, false, p, r);
    return true;
}

}  // namespace

__global__ __launch_bounds__(256) void k_list_tree_update(ListTreeArgs a) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t r[4];
    (void)lt_update(a, gid >> 1, (uint32_t)(gid & 1u), r);
}

// ----------------------------------------------------------------------------
// Several resident trees in one launch: slice blockIdx.y of
// the grid is k_list_tree_update over tree g.t[blockIdx.y] -- the descriptors
// travel by value in the kernel arguments, nothing is uploaded.  A tree of at
// most one chunk has no levels: the first pair of its slice hashes the raw
// chunk with the mix-in, as k_final_small does.
// Container (hash.go:141-159, a struct whose list fields are these trees): the
// pair that stores tree i's root also stores it at container + coff[i]; the
// last of the nparts participating trees to arrive hashes the whole container
// message.  Ordering contract, the one of the climb's hand-off: root stores ->
// __threadfence() (agent release) -> acq_rel agent-scope atomic add on the
// counter (zeroed on the stream by the same call); the last arriver: that
// atomic -> __threadfence() (agent acquire) -> agent-scope loads of the
// container.  Exactly one pair per tree arrives and none waits, so the launch
// completes whatever the dispatch order.
namespace {

// K(p[0, len)), p 4-B aligned, every byte by an agent-scope load
__device__ __noinline__ void sponge_acquired(const uint8_t* p, uint32_t len, uint4& d0, uint4& d1) {
    const uint32_t nb = len / 136 + 1;
    State s;
    zero(s);
    for (uint32_t b = 0; b < nb; ++b) {
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            uint32_t v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t m = b * 136 + 8u * w + 4u * h;
                uint32_t x = 0;
                if (m + 4 <= len) {
                    x = __hip_atomic_load(reinterpret_cast<const uint32_t*>(p + m), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
                } else {
#pragma unroll 1
                    for (uint32_t k = 0; m + k < len; ++k)  // the last 1..3 bytes
                        x |= (uint32_t)__hip_atomic_load(p + m + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                             << (8 * k);
                }
                if (m <= len && len < m + 4) x ^= 1u << (8 * (len - m));  // domain pad byte 0x01
                v[h] = x;
            }
            if (b == nb - 1 && w == 16) v[1] ^= 0x80000000u;
            s.lo[w] ^= v[0];
            s.hi[w] ^= v[1];
        }
        keccak_f(s);
    }
    digest(s, d0, d1);
}

}  // namespace

__global__ __launch_bounds__(256) void k_trees_update(TreesArgs g) {
    const ListTreeArgs& a = g.t[blockIdx.y];
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t = gid >> 1;
    const uint32_t p = (uint32_t)(gid & 1u);
    uint32_t r[4];
    if ((a.n_new + a.per - 1) / a.per <= 1) {  // no levels: root = K(raw chunk (0^128 when empty) || le64(n) || 0^24)
        if (t != 0) return;
        uint4 d0, d1;
        sponge_generic(a.items, a.n_new * a.item_len, a.n_new == 0 ? 128u : 0u, true, a.n_new, d0, d1);
        r[0] = ilv::to_ilv(d0.x, d0.y, p);
        r[1] = ilv::to_ilv(d0.z, d0.w, p);
        r[2] = ilv::to_ilv(d1.x, d1.y, p);
        r[3] = ilv::to_ilv(d1.z, d1.w, p);
        store_node3(a.root_out, 0, false, p, r);
    } else if (!lt_update(a, t, p, r)) {
        return;
    }
    const uint32_t coff = g.coff[blockIdx.y];
    if (coff == 0xffffffffu) return;  // this tree is no field of the container
    store_node3(reinterpret_cast<uint32_t*>(g.container + coff), 0, false, p, r);
    __threadfence();  // release: this pair's root stores before its arrival
    uint32_t last = 0;
    if (p == 0)
        last = __hip_atomic_fetch_add(g.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == g.nparts;
    last |= (uint32_t)__shfl_xor((int)last, 1);
    if (!last) return;
    __threadfence();  // acquire: every tree's root stores before the loads of the container
    uint4 d0, d1;
    sponge_acquired(g.container, g.container_len, d0, d1);
    if (p == 0) {
        const uint32_t d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int w = 0; w < 8; ++w) g.container_root[w] = d[w];
    }
}

// list[idx[v]] = values[v] for v < k_idx (an index >= n_old is skipped), then
// the n_app appended values to items n_old ..; `unit`-byte pieces (8 when
// everything is 8-B aligned, else 1), one per thread
__global__ __launch_bounds__(256) void k_list_tree_scatter(uint8_t* __restrict__ items,
                                                           const uint64_t* __restrict__ idx, uint64_t k_idx,
                                                           uint64_t n_old, uint64_t n_app, uint32_t item_len,
                                                           uint32_t unit, const uint8_t* __restrict__ vals) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = item_len / unit;
    const uint64_t v = g / per;
    const uint32_t w = (uint32_t)(g - v * per);
    if (v >= k_idx + n_app) return;
    const uint64_t x = v < k_idx ? idx[v] : n_old + (v - k_idx);
    if (v < k_idx && x >= n_old) return;
    const uint64_t src = v * item_len + (uint64_t)w * unit, dst = x * item_len + (uint64_t)w * unit;
    if (unit == 8)
        *reinterpret_cast<uint64_t*>(items + dst) = *reinterpret_cast<const uint64_t*>(vals + src);
    else
        items[dst] = vals[src];
}

// ----------------------------------------------------------------------------
// Device-resident registry tree: TreeHash of a list of flat
// structs (hash.go:118-159, 194-239) re-hashed from the changed RECORDS.  The
// tree is the list tree above over the buffer of 32-B struct roots; an update
// gathers the dirty records, hashes them with the struct-roots kernels,
// scatters the roots (k_list_tree_scatter) and climbs (k_list_tree_update).
// The gather: the first `ext` bytes (a multiple of 4) of the record of every
// work item (idx[t] clamped to the last old record as in lt_chunk, then the
// appended records) to out + t * ext, one dword per thread
__global__ __launch_bounds__(256) void k_struct_tree_gather(const uint8_t* __restrict__ rec,
                                                            const uint64_t* __restrict__ idx, uint64_t k_idx,
                                                            uint64_t n_old, uint64_t n_app, uint32_t rec_len,
                                                            uint32_t ext, uint8_t* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = ext / 4;
    const uint64_t t = g / per;
    const uint32_t w = (uint32_t)(g - t * per);
    if (t >= k_idx + n_app) return;
    uint64_t x;
    if (t < k_idx) {
        x = idx[t];
        const uint64_t last = n_old ? n_old - 1 : 0;
        if (x > last) x = last;
    } else {
        x = n_old + (t - k_idx);
    }
    reinterpret_cast<uint32_t*>(out + t * ext)[w] = reinterpret_cast<const uint32_t*>(rec + x * rec_len)[w];
}

// ----------------------------------------------------------------------------
// Device-resident tree of a list of byte strings: TreeHash of
// a [][N]byte (hash.go:100-107, 118-139, 194-239) re-hashed from the changed
// ELEMENTS.  The tree is the list tree above over the buffer of 32-B element
// digests K(le32(elem_len) || e_i); an update digests the dirty elements in
// place (this kernel) and climbs (k_list_tree_update).
// One thread per work item (the listed indices, then the appended elements,
// as in lt_chunk) reads its element from `elems` and stores the digest at
// digests[index]; a listed index >= n_old writes nothing.  fast32: 32-B
// elements at a 16-B aligned base (elem32_digest, one block), otherwise the
// general sponge of k_elem_digests<false>.
__global__ __launch_bounds__(256) void k_bytes_tree_digest(const uint8_t* __restrict__ elems, uint32_t elem_len,
                                                           uint32_t fast32, const uint64_t* __restrict__ idx,
                                                           uint64_t k_idx, uint64_t n_old, uint64_t n_app,
                                                           uint4* __restrict__ digests) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= k_idx + n_app) return;
    uint64_t x;
    if (w < k_idx) {
        x = idx[w];
        if (x >= n_old) return;
    } else {
        x = n_old + (w - k_idx);
    }
    uint32_t d[8];
    if (fast32)
        elem32_digest(reinterpret_cast<const uint4*>(elems) + 2 * x, d);
    else
        elem_digest_any(elems + x * (uint64_t)elem_len, elem_len, d);
    digests[2 * x] = make_uint4(d[0], d[1], d[2], d[3]);
    digests[2 * x + 1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// ----------------------------------------------------------------------------
// Stage 0 of several resident trees in one launch: slice
// blockIdx.y of the grid is one segment of g.s -- k_list_tree_scatter's rule
// (values into an item buffer, struct roots into a level 0), or
// k_bytes_tree_digest's rule with the element read from the STAGED values
// (vals + w * elem_len) instead of the element buffer, so a tree's digest
// segment does not wait for its scatter segment of the same launch.  Every
// thread writes only its own piece or digest: no counters, no hand-off.
__global__ __launch_bounds__(256) void k_trees_stage0(Stage0Args g) {
    const Stage0Seg& s = g.s[blockIdx.y];
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t T = s.k_idx + s.n_app;
    if (s.mode >= kStage0Digest) {  // one thread per work item
        const uint64_t w = gid;
        if (w >= T) return;
        uint64_t x;
        if (w < s.k_idx) {
            x = s.idx[w];
            if (x >= s.n_old) return;
        } else {
            x = s.n_old + (w - s.k_idx);
        }
        uint32_t d[8];
        if (s.mode == kStage0Digest32)
            elem32_digest(reinterpret_cast<const uint4*>(s.vals) + 2 * w, d);
        else
            elem_digest_any(s.vals + w * (uint64_t)s.item_len, s.item_len, d);
        uint4* digests = reinterpret_cast<uint4*>(s.dst);
        digests[2 * x] = make_uint4(d[0], d[1], d[2], d[3]);
        digests[2 * x + 1] = make_uint4(d[4], d[5], d[6], d[7]);
        return;
    }
    const uint32_t unit = s.mode;  // 8 or 1
    const uint32_t per = s.item_len / unit;
    const uint64_t v = gid / per;
    const uint32_t w = (uint32_t)(gid - v * per);
    if (v >= T) return;
    const uint64_t x = v < s.k_idx ? s.idx[v] : s.n_old + (v - s.k_idx);
    if (v < s.k_idx && x >= s.n_old) return;
    const uint64_t src = v * s.item_len + (uint64_t)w * unit, dst = x * s.item_len + (uint64_t)w * unit;
    if (unit == 8)
        *reinterpret_cast<uint64_t*>(s.dst + dst) = *reinterpret_cast<const uint64_t*>(s.vals + src);
    else
        s.dst[dst] = s.vals[src];
}

// ----------------------------------------------------------------------------
// Stable erase of a resident tree, gather form: one thread per
// `unit`-byte piece of a destination value in [first, first + moved); segment
// blockIdx.y is the value buffer or level 0.  Destination q reads source
// q + j, j from the index map of tree_compact.hpp.  A block searches the whole
// removal list twice -- for its first and its last destination -- and every
// thread then bisects between the two, which for all but the blocks that span
// a removed run is no step at all.  Out of place: dst never overlaps a source,
// so every thread writes only its own piece: no counters, no hand-off.  With
// k_rm == 0 (j == 0) it is the copy that puts the moved range back.
__global__ __launch_bounds__(256) void k_tree_compact(CompactArgs g) {
    const CompactSeg& s = g.s[blockIdx.y];
    const uint32_t per = s.item_len / s.unit;
    const uint64_t pieces = g.moved * per;
    const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x;
    if (g0 >= pieces) return;  // the whole block: the other segment is the larger one
    __shared__ uint64_t jb[2];
    if (g.k_rm) {  // uniform over the launch
        if (threadIdx.x < 2) {
            const uint64_t last = g0 + blockDim.x - 1 < pieces ? g0 + blockDim.x - 1 : pieces - 1;
            jb[threadIdx.x] = compact_skip(g.rm, g.k_rm, g.first + (threadIdx.x ? last : g0) / per);
        }
        __syncthreads();
    }
    const uint64_t gid = g0 + threadIdx.x;
    if (gid >= pieces) return;
    const uint64_t v = gid / per;
    const uint32_t w = (uint32_t)(gid - v * per);
    const uint64_t j = g.k_rm ? compact_skip_in(g.rm, jb[0], jb[1], g.first + v) : 0;  // <= k_rm for any list
    const uint8_t* src = s.src + (v + j) * s.item_len + (uint64_t)w * s.unit;
    uint8_t* dst = s.dst + v * s.item_len + (uint64_t)w * s.unit;
    if (s.unit == 16)
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else if (s.unit == 8)
        *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(src);
    else if (s.unit == 4)
        *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
    else
        *dst = *src;
}

// ----------------------------------------------------------------------------
// Merkle proofs out of a resident list tree: a gather.  Each
// wave writes one record per turn (grid stride over the indices) as one
// contiguous run of 16-B pieces: piece q < 16 is bytes [16 q, 16 q + 16) of
// the item's 256-B window -- one 16-B load where the window's base is 16-B
// aligned and the piece lies inside the list, byte loads below `total`
// otherwise (an item length such as 100 puts windows at 200 j), zero without a
// load past the window's end -- and lane pair (16 + 2 (d - 1), + 1) takes the
// two halves of sib[d], the stored level-d node (j >> (d - 1)) ^ 1, read only
// when it is below the level's count of the CURRENT list (list_branch.hpp):
// what a shrink left to the right of the new end is never loaded.  An index
// >= n gives a zero record.  No hand-off between waves, no counter, no
// workspace; the level offsets are per-workgroup LDS.
__global__ __launch_bounds__(64 * kBranchWaves) void k_list_tree_branches(
    const uint8_t* __restrict__ level0, const uint4* __restrict__ levels, uint64_t n, uint64_t capacity,
    uint32_t item_len, const uint64_t* __restrict__ indices, uint64_t k, uint4* __restrict__ out) {
    __shared__ uint64_t lvoff[64];  // first node of level d in the level array
    const BranchShape b = branch_shape(n, capacity, item_len);
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    if (w == 0) lvoff[L] = (L >= 1 && L < b.D) ? branch_level_off(b, L) : 0;
    __syncthreads();
    const uint32_t pieces = (uint32_t)(branch_record_bytes(b) / 16);
    const uint64_t stride = (uint64_t)gridDim.x * kBranchWaves;
    for (uint64_t g = (uint64_t)blockIdx.x * kBranchWaves + w; g < k; g += stride) {
        const uint64_t i = indices[g];
        const bool live = i < n;  // wave-uniform
        uint64_t j = 0, lo = 0;
        uint32_t wl = 0;
        if (live) {
            j = branch_window_index(b, i);
            branch_window(b, j, &lo, &wl);
        }
        const uint8_t* wsrc = level0 + lo;
        const bool aligned = (((uintptr_t)wsrc) & 15u) == 0;
        for (uint32_t q = L; q < pieces; q += 64) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (live && q < 16u) {
                const uint32_t a = 16u * q;
                if (aligned && a + 16u <= wl) {
                    v = *reinterpret_cast<const uint4*>(wsrc + a);
                } else if (a < wl) {
                    uint32_t t[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (uint32_t e = 0; e < 16u; ++e)
                        if (a + e < wl) t[e >> 2] |= (uint32_t)wsrc[a + e] << (8u * (e & 3u));
                    v = make_uint4(t[0], t[1], t[2], t[3]);
                }
            } else if (live) {
                const uint32_t d = 1u + ((q - 16u) >> 1), h = (q - 16u) & 1u;
                uint64_t node;
                if (branch_sibling(b, j, d, &node)) v = levels[2 * (lvoff[d] + node) + h];
            }
            out[(uint64_t)pieces * g + q] = v;
        }
    }
}

// ----------------------------------------------------------------------------
// Copy of resident trees between the layouts of two capacities (DESIGN.md
// §5m): the live part of up to kTreesMax trees and one 32-byte extra, cut into
// 16-byte pieces by tree_copy.hpp; nothing is hashed.  The pieces of the whole
// call are numbered through, tree after tree, and a bounded grid strides over
// them: a thread issues the loads of kCopyUnroll pieces, kCopyThreads apart (a
// wave's load is 1 KiB contiguous inside a segment), then their stores.  Where
// a tree's pieces start, where each of its segments starts and the two base
// addresses of every segment -- the level offsets of the two layouts in them --
// are per-workgroup LDS, filled by one wave per tree, a lane per segment.  A
// piece of the values whose addresses are not 16-byte aligned, or the short
// last one, goes in units of 8, 4 or 1 bytes and only as far as the segment
// reaches; level 0, the levels and the roots are 16-byte aligned by contract.
// Every thread writes only its own pieces: no counter, no hand-off, no workspace.
__device__ __forceinline__ void copy_units(uint8_t* dst, const uint8_t* src, uint32_t valid) {
    const uintptr_t a = (uintptr_t)dst | (uintptr_t)src;
    uint32_t i = 0;
    if ((a & 7u) == 0)
        for (; i + 8 <= valid; i += 8) *reinterpret_cast<uint64_t*>(dst + i) = *reinterpret_cast<const uint64_t*>(src + i);
    if ((a & 3u) == 0)
        for (; i + 4 <= valid; i += 4) *reinterpret_cast<uint32_t*>(dst + i) = *reinterpret_cast<const uint32_t*>(src + i);
    for (; i < valid; ++i) dst[i] = src[i];
}

// a 16-byte piece in registers, and HBM named as such: an address read back from LDS is otherwise a flat one
typedef uint32_t copy_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) copy_u32x4 copy_global_u32x4;

__global__ __launch_bounds__(kCopyThreads) void k_trees_copy(TreesCopyArgs g) {
    __shared__ CopyShape shp[kTreesMax];
    __shared__ uint64_t tfirst[kTreesMax + 1];                // the call's first piece of tree t; [ntrees]: the extra's
    __shared__ uint64_t sfirst[kTreesMax][kCopySegsMax + 1];  // tree t's first piece of segment s; [segs]: its total
    __shared__ const uint8_t* ssrc[kTreesMax][kCopySegsMax];  // where segment s starts in the source ...
    __shared__ uint8_t* sdst[kTreesMax][kCopySegsMax];        // ... and in the destination
    const uint32_t nt = g.ntrees < kTreesMax ? g.ntrees : kTreesMax;
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    for (uint32_t t0 = 0; t0 < nt; t0 += kCopyThreads / 64) {
        const uint32_t t = __builtin_amdgcn_readfirstlane(t0 + w);  // wave-uniform: the descriptor by scalar loads
        if (t >= nt) continue;
        const CopyTree& T = g.t[t];
        const CopyShape c = copy_shape(T.n, T.cap_src, T.cap_dst, T.item_len, T.level0 != 0);
        if (L == 0) shp[t] = c;
        const uint32_t segs = copy_segs(c);
        for (uint32_t s = L; s <= segs; s += 64) {
            sfirst[t][s] = copy_seg_first(c, s);
            if (s == segs) break;
            uint64_t so, dof;
            copy_seg_offs(c, s, &so, &dof);
            const uint32_t b = copy_seg_buf(c, s);
            const uint8_t* sp = b == kCopyItems    ? T.src_items
                                : b == kCopyLevel0 ? T.src_level0
                                : b == kCopyLevels ? T.src_levels
                                                   : T.src_root;
            uint8_t* dp = b == kCopyItems    ? T.dst_items
                          : b == kCopyLevel0 ? T.dst_level0
                          : b == kCopyLevels ? T.dst_levels
                                             : T.dst_root;
            ssrc[t][s] = sp + so;
            sdst[t][s] = dp + dof;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            tfirst[t] = a;
            a += sfirst[t][copy_segs(shp[t])];
        }
        tfirst[nt] = a;
    }
    __syncthreads();
    const uint64_t in_trees = tfirst[nt], total = in_trees + (g.extra_dst ? 32 / kCopyPiece : 0);
    const uint64_t turn = (uint64_t)kCopyThreads * kCopyUnroll;
    for (uint64_t base = blockIdx.x * turn; base < total; base += gridDim.x * turn) {
        copy_u32x4 v[kCopyUnroll];
        const uint8_t* sp[kCopyUnroll];
        uint8_t* dp[kCopyUnroll];
        uint32_t valid[kCopyUnroll];
        bool whole[kCopyUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            const uint64_t p = base + u * kCopyThreads + threadIdx.x;
            valid[u] = 0;
            sp[u] = nullptr;
            dp[u] = nullptr;
            if (p >= total) {
            } else if (p >= in_trees) {
                sp[u] = g.extra_src + kCopyPiece * (p - in_trees);
                dp[u] = g.extra_dst + kCopyPiece * (p - in_trees);
                valid[u] = kCopyPiece;
            } else {
                uint32_t t = 0, s = 0;
                while (p >= tfirst[t + 1]) ++t;  // p < tfirst[nt]
                const uint64_t q = p - tfirst[t];
                while (q >= sfirst[t][s + 1]) ++s;  // q < sfirst[t][segs]; an empty segment is stepped over
                const CopyPiece pc = copy_piece_in(shp[t], s, q - sfirst[t][s], 0, 0);
                sp[u] = ssrc[t][s] + pc.src_off;
                dp[u] = sdst[t][s] + pc.dst_off;
                valid[u] = pc.valid;
            }
            whole[u] = valid[u] == kCopyPiece && (((uintptr_t)sp[u] | (uintptr_t)dp[u]) & 15u) == 0;
            v[u] = copy_u32x4{0u, 0u, 0u, 0u};
            if (whole[u]) v[u] = *reinterpret_cast<const copy_global_u32x4*>((uintptr_t)sp[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            if (whole[u]) *reinterpret_cast<copy_global_u32x4*>((uintptr_t)dp[u]) = v[u];
        }
        // the pieces that go in smaller units, apart: the stores above wait for their own loads only
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            if (!whole[u] && valid[u]) copy_units(dp[u], sp[u], valid[u]);
        }
    }
}

// The byte sponge of sponge_generic over a message whose bytes [sub_lo, sub_lo
// + sub_len) come from `sub` instead of p: message = A' || 0^lz || (lenc ?
// le64(nval) || 0^24 : -), A'[m] = sub(m - sub_lo) inside the range, p[m]
// elsewhere (m < la).  The source switches per byte, so no thread keeps a copy
// of the message.
template <class Sub>
__device__ __forceinline__ void sponge_subst(const uint8_t* __restrict__ p, uint32_t la, uint32_t sub_lo,
                                             uint32_t sub_len, const Sub& sub, uint32_t lz, bool lenc, uint64_t nval,
                                             uint4& d0, uint4& d1) {
    const uint32_t len = la + lz + (lenc ? 32u : 0u);
    const uint32_t nb = len / 136 + 1;
    const bool aligned = (((uintptr_t)p) & 7u) == 0;
    State s;
    zero(s);
    for (uint32_t blk = 0; blk < nb; ++blk) {
        const uint32_t base = blk * 136;
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            const uint32_t m0 = base + 8u * w;
            uint32_t lo = 0, hi = 0;
            if (aligned && m0 + 8 <= la && (m0 + 8 <= sub_lo || m0 >= sub_lo + sub_len)) {
                const uint2 v = *reinterpret_cast<const uint2*>(p + m0);
                lo = v.x;
                hi = v.y;
            } else if (m0 < len) {
#pragma unroll 1
                for (int q = 0; q < 8; ++q) {
                    const uint32_t m = m0 + q;
                    uint32_t byte = 0;
                    if (m < la) {
                        byte = (m - sub_lo < sub_len) ? sub(m - sub_lo) : (uint32_t)p[m];
                    } else if (m >= la + lz && m < len) {
                        const uint32_t e = m - la - lz;  // lenc byte
                        byte = e < 8 ? (uint32_t)((nval >> (8 * e)) & 0xFF) : 0u;
                    }
                    if (q < 4)
                        lo |= byte << (8 * q);
                    else
                        hi |= byte << (8 * (q - 4));
                }
            }
            if (m0 <= len && len < m0 + 8) {  // domain pad byte 0x01
                const uint32_t q = len - m0;
                if (q < 4)
                    lo ^= 1u << (8 * q);
                else
                    hi ^= 1u << (8 * (q - 4));
            }
            if (blk == nb - 1 && w == 16) hi ^= 0x80000000u;
            s.lo[w] ^= lo;
            s.hi[w] ^= hi;
        }
        keccak_f(s);
    }
    digest(s, d0, d1);
}

// Batched verification of list-tree proofs, one proof per
// thread: the window with the caller's value written over the item's bytes
// through the byte sponge (at most 384 B: the window, 0^128 when its second
// chunk does not exist), the fold over sib[1 .. D - 1] (64-B messages, 160-B
// ones where the sibling does not exist: its slot is not read), the mix-in of
// n, and with a container the hash of its message with the list root in place
// of bytes [container_off, +32).  Compared with the batch's one root
// (root_stride == 0) or root g (32).  A dependent chain of D + 2 .. D + 6
// permutations per thread and a handful of loads: latency-bound, as
// k_verify_deposits.
__global__ __launch_bounds__(256) void k_verify_list_branches(
    const uint8_t* __restrict__ values, const uint64_t* __restrict__ indices, uint64_t k, uint64_t n,
    uint32_t item_len, const uint8_t* __restrict__ branches, const uint8_t* __restrict__ roots, uint32_t root_stride,
    const uint8_t* __restrict__ container, uint32_t container_len, uint32_t container_off,
    uint8_t* __restrict__ ok) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= k) return;
    const uint64_t i = indices[g];
    if (i >= n) {
        ok[g] = 0;
        return;
    }
    const BranchShape b = branch_shape(n, n, item_len);  // the capacity only places the levels
    const uint8_t* rec = branches + branch_record_bytes(b) * g;
    const uint8_t* val = values + (uint64_t)item_len * g;
    const uint64_t j = branch_window_index(b, i);
    const uint32_t pos = branch_item_pos(b, i);
    uint64_t lo;
    uint32_t wl;
    branch_window(b, j, &lo, &wl);
    const auto value_byte = [&](uint32_t e) { return (uint32_t)val[e]; };
    uint4 v0, v1;
    if (b.nchunks < 2) {  // the top is the raw chunk
        sponge_subst(rec, wl, pos, item_len, value_byte, 0u, true, n, v0, v1);
    } else {
        sponge_subst(rec, wl, pos, item_len, value_byte, branch_window_padded(b, j) ? 128u : 0u, false, 0, v0, v1);
        const uint4* sib = reinterpret_cast<const uint4*>(rec + kBranchWindow);
        for (uint32_t d = 1; d < b.D; ++d) {
            const uint64_t q = j >> (d - 1);
            const bool right = (q & 1u) != 0, pad = !right && q + 1 >= branch_level_count(b, d);
            uint4 s0 = make_uint4(0, 0, 0, 0), s1 = s0;
            if (!pad) {
                s0 = sib[2 * (d - 1)];
                s1 = sib[2 * (d - 1) + 1];
            }
            if (right)
                hash_pair(s0, s1, v0, v1, false, v0, v1);
            else
                hash_pair(v0, v1, s0, s1, pad, v0, v1);
        }
        hash_final(v0, v1, n, v0, v1);
    }
    if (container) {
        const uint4 r0 = v0, r1 = v1;
        const auto root_byte = [&](uint32_t e) {
            const uint32_t wd = e >> 2;
            const uint32_t x = wd == 0   ? r0.x
                               : wd == 1 ? r0.y
                               : wd == 2 ? r0.z
                               : wd == 3 ? r0.w
                               : wd == 4 ? r1.x
                               : wd == 5 ? r1.y
                               : wd == 6 ? r1.z
                                         : r1.w;
            return (x >> (8u * (e & 3u))) & 0xFFu;
        };
        sponge_subst(container, container_len, container_off, 32u, root_byte, 0u, false, 0, v0, v1);
    }
    const uint32_t* rt = reinterpret_cast<const uint32_t*>(roots + (root_stride ? 32 * g : 0));
    ok[g] = (v0.x == rt[0] && v0.y == rt[1] && v0.z == rt[2] && v0.w == rt[3] && v1.x == rt[4] && v1.y == rt[5] &&
             v1.z == rt[6] && v1.w == rt[7]);
}

// ----------------------------------------------------------------------------
// Audit of resident trees: is every stored node what the level
// below it says?  A stored level-d node is checked against the STORED level
// d - 1, so nothing depends on anything the launch computes: the work items of
// tree_audit.hpp -- every node of level 1 .. D and the root of every tree, then
// the container checks -- are numbered through and a bounded grid strides over
// them, one Keccak state per lane.  Where a tree's items start, where each of
// its levels' items start and the two base addresses of every level (the level
// below it and its own stored nodes) are per-workgroup LDS, filled by one wave
// per tree, a lane per level.  A window of 256 bytes at a 16-byte aligned
// address is sixteen 16-byte loads (block 2 after the first permutation, as in
// hash_window256_split); any other window and the raw chunk under the root of a
// short list go through sponge_generic, which reads no byte beyond the message.
// Nodes are 16-byte aligned by contract.  A lane that finds a mismatch adds one
// to the tree's count and lowers the tree's key, both agent-scope atomics; no
// other word is written: no hand-off, no arrival counter, no workspace.
namespace {

// 16 bytes of HBM named as such: an address read back from LDS is otherwise a flat one
__device__ __forceinline__ uint4 audit_ld16(const uint8_t* p) {
    const copy_u32x4 v = *reinterpret_cast<const copy_global_u32x4*>((uintptr_t)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void audit_window256(const uint8_t* w, uint4& d0, uint4& d1) {
    State s;
    uint4 v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = audit_ld16(w + 16 * k);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s.lo[2 * k] = v[k].x;
        s.hi[2 * k] = v[k].y;
        s.lo[2 * k + 1] = v[k].z;
        s.hi[2 * k + 1] = v[k].w;
    }
    s.lo[16] = v[8].x;
    s.hi[16] = v[8].y;
    const uint32_t t0 = v[8].z, t1 = v[8].w;
#pragma unroll
    for (int k = 17; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
    keccak_f(s);
    s.lo[0] ^= t0;
    s.hi[0] ^= t1;
    uint4 u[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = audit_ld16(w + 16 * (9 + k));
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        s.lo[1 + 2 * k] ^= u[k].x;
        s.hi[1 + 2 * k] ^= u[k].y;
        s.lo[2 + 2 * k] ^= u[k].z;
        s.hi[2 + 2 * k] ^= u[k].w;
    }
    s.lo[15] ^= 1u;  // byte 256 = byte 120 of block 1
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, d0, d1);
}

__device__ __forceinline__ bool audit_differs(uint4 a0, uint4 a1, uint4 b0, uint4 b1) {
    return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) |
            (a1.z ^ b1.z) | (a1.w ^ b1.w)) != 0;
}

// the rare path: one more bad node of this report, and the smallest (level, index) so far
__device__ __noinline__ void audit_mismatch(AuditReport* r, uint32_t level, uint64_t index) {
    (void)__hip_atomic_fetch_add(&r->bad, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_min(&r->key, audit_key(level, index), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

__global__ __launch_bounds__(kAuditThreads, 4) void k_trees_audit(TreesAuditArgs g) {
    constexpr uint32_t kSlots = kCopyLevelsMax + 1;      // levels 1 .. D <= 64 and the root
    __shared__ AuditShape shp[kTreesMax];
    __shared__ uint64_t tfirst[kTreesMax + 1];          // the call's first item of tree t; [ntrees]: the container's
    __shared__ uint64_t sfirst[kTreesMax][kSlots + 1];  // tree t's first item of slot s; [slots]: its total
    __shared__ const uint8_t* schild[kTreesMax][kSlots];  // where slot s's messages start ...
    __shared__ const uint8_t* snode[kTreesMax][kSlots];   // ... and its stored nodes
    __shared__ uint32_t scoff[kTreesMax];
    const uint32_t nt = g.ntrees < kTreesMax ? g.ntrees : kTreesMax;
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    for (uint32_t t0 = 0; t0 < nt; t0 += kAuditThreads / 64) {
        const uint32_t t = __builtin_amdgcn_readfirstlane(t0 + w);  // wave-uniform: the descriptor by scalar loads
        if (t >= nt) continue;
        const AuditTree& T = g.t[t];
        const AuditShape b = audit_shape(T.n, T.capacity, T.len0);
        if (L == 0) {
            shp[t] = b;
            scoff[t] = T.coff;
        }
        const uint32_t slots = audit_slots(b);
        for (uint32_t s = L; s <= slots; s += 64) {
            sfirst[t][s] = audit_slot_first(b, s);
            if (s == slots) break;
            uint32_t cb, nb;
            uint64_t co, no;
            audit_slot_child(b, s, &cb, &co);
            audit_slot_node(b, s, &nb, &no);
            schild[t][s] = (cb == kAuditLevel0 ? T.level0 : T.levels) + co;
            snode[t][s] = (nb == kAuditRootBuf ? T.root : T.levels) + no;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            tfirst[t] = a;
            a += sfirst[t][audit_slots(shp[t])];
        }
        tfirst[nt] = a;
    }
    __syncthreads();
    const uint64_t in_trees = tfirst[nt], total = in_trees + (g.container ? 1 + nt : 0);
    const uint64_t stride = (uint64_t)gridDim.x * kAuditThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kAuditThreads + threadIdx.x; q < total; q += stride) {
        uint4 d0, d1, s0, s1;
        if (q >= in_trees) {  // the container: K(message), then each tree's 32 bytes of it against the tree's root
            const uint32_t c = (uint32_t)(q - in_trees);
            const uint32_t *have, *want;
            if (c == 0) {
                sponge_generic(g.container, g.container_len, 0u, false, 0, d0, d1);
                want = reinterpret_cast<const uint32_t*>(g.container_root);
                have = nullptr;
            } else {
                const uint32_t coff = scoff[c - 1];
                if (coff == 0xffffffffu) continue;  // no field of the container
                have = reinterpret_cast<const uint32_t*>(g.container + coff);
                want = reinterpret_cast<const uint32_t*>(snode[c - 1][shp[c - 1].D]);
                d0 = make_uint4(have[0], have[1], have[2], have[3]);
                d1 = make_uint4(have[4], have[5], have[6], have[7]);
            }
            s0 = make_uint4(want[0], want[1], want[2], want[3]);
            s1 = make_uint4(want[4], want[5], want[6], want[7]);
            if (audit_differs(d0, d1, s0, s1)) audit_mismatch(g.reports + nt, kAuditContainer, c);
            continue;
        }
        uint32_t t = 0;
        while (q >= tfirst[t + 1]) ++t;  // q < tfirst[nt]
        const uint64_t r = q - tfirst[t];
        const AuditShape& b = shp[t];
        uint32_t lo = 0, hi = b.D;  // the last slot that starts at or below r (audit_slot_of, over the LDS copy)
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (sfirst[t][mid] <= r)
                lo = mid;
            else
                hi = mid - 1;
        }
        const AuditItem it = audit_item_in(b, lo, r - sfirst[t][lo]);
        const uint8_t* src = schild[t][lo] + it.child_off;
        const uint8_t* node = snode[t][lo] + it.node_off;
        if (it.level == 1) {
            if (it.msg_len == 256u && it.zeros == 0u && (((uintptr_t)src) & 15u) == 0)
                audit_window256(src, d0, d1);
            else
                sponge_generic(src, it.msg_len, it.zeros, false, 0, d0, d1);
        } else if (it.child_buf == kAuditLevel0) {  // the root of a list of at most one chunk
            sponge_generic(src, it.msg_len, it.zeros, true, b.n, d0, d1);
        } else {  // two nodes, a node and 0^128, or the top node and the length
            const uint4 l0 = audit_ld16(src), l1 = audit_ld16(src + 16);
            uint4 r0 = make_uint4((uint32_t)b.n, (uint32_t)(b.n >> 32), 0u, 0u), r1 = make_uint4(0u, 0u, 0u, 0u);
            if (it.msg_len == 64u) {
                r0 = audit_ld16(src + 32);
                r1 = audit_ld16(src + 48);
            }
            hash_pair(l0, l1, r0, r1, it.zeros != 0u, d0, d1);
        }
        s0 = audit_ld16(node);
        s1 = audit_ld16(node + 16);
        if (audit_differs(d0, d1, s0, s1)) audit_mismatch(g.reports + t, it.level, it.index);
    }
}

__global__ __launch_bounds__(256) void k_audit_compare(const uint4* __restrict__ fresh, const uint4* __restrict__ stored,
                                                       uint64_t first, uint64_t m, AuditReport* report) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (audit_differs(fresh[2 * i], fresh[2 * i + 1], stored[2 * (first + i)], stored[2 * (first + i) + 1]))
        audit_mismatch(report, 0u, first + i);
}

__global__ __launch_bounds__(64) void k_audit_reports(AuditReport* reports, uint32_t count, uint32_t finish) {
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    AuditReport& r = reports[i];
    if (!finish) {
        r.bad = 0;
        r.key = kAuditKeyNone;
        r.first_level = kAuditNone;
        r.pad = 0;
    } else if (r.key != kAuditKeyNone) {
        r.first_level = (uint32_t)(r.key >> kAuditKeyShift);
        r.key &= (1ull << kAuditKeyShift) - 1;
    }
}

// ----------------------------------------------------------------------------
// Diff of two resident trees by Merkle descent (the rule:
// tree_diff.hpp).  A work item is one subtree of height h0 of one pair; a
// prefix of the pairs' item counts in LDS maps a workgroup's turn to (pair,
// subtree), the turns by grid stride.  Every thread loads the subtree's root
// from both trees (the same 2 x 32 bytes: workgroup-uniform); comparable and
// equal ends the item there, without a barrier.  Otherwise the workgroup walks
// down with the frontier in LDS, as indices local to the subtree: a lane takes
// one frontier node, compares it when it is comparable and counts the children
// that go on (0, 1 or 2); their places come from two wave ballots and one LDS
// add per wave.  The level-1 nodes that remain name the leaves: a lane per
// value below m, 2 x 16-B loads for a 32-B entry, for list items 16-B loads
// where both sides' addresses are equally aligned with byte loads around them,
// byte loads otherwise.  A wave reserves its slots with one add on the pair's
// total and lowers first_index with one min; an index is stored only below
// max_out.  No workgroup waits for another and every loop is bounded by a
// count computed from n_a and n_b.
namespace {

__device__ __forceinline__ bool diff_node_ne(const uint8_t* a, const uint8_t* b) {
    const uint4 a0 = audit_ld16(a), a1 = audit_ld16(a + 16), b0 = audit_ld16(b), b1 = audit_ld16(b + 16);
    return audit_differs(a0, a1, b0, b1);
}

// s bytes at pa against s bytes at pb; no byte outside them is read
__device__ __forceinline__ bool diff_leaf_ne(const uint8_t* pa, const uint8_t* pb, uint32_t s) {
    uint32_t k = 0, acc = 0;
    if (((((uintptr_t)pa) ^ ((uintptr_t)pb)) & 15u) == 0) {
        const uint32_t lead = (16u - (uint32_t)(((uintptr_t)pa) & 15u)) & 15u, head = lead < s ? lead : s;
        for (; k < head; ++k) acc |= (uint32_t)(pa[k] ^ pb[k]);
        for (; k + 16u <= s; k += 16u) {
            const uint4 x = audit_ld16(pa + k), y = audit_ld16(pb + k);
            acc |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
        }
    }
    for (; k < s; ++k) acc |= (uint32_t)(pa[k] ^ pb[k]);
    return acc != 0;
}

__device__ __forceinline__ uint32_t diff_lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace

__global__ __launch_bounds__(kDiffThreads) void k_trees_diff(TreesDiffArgs g) {
    __shared__ uint64_t ifirst[kTreesMax + 1];      // the call's first work item of pair t; [ntrees]: the total
    __shared__ uint32_t front[2][kDiffFrontMax];    // a level's frontier, local to the subtree; then the level-1 nodes
    __shared__ uint32_t cnt[kDiffHeight + 1];       // nodes in the frontier of level d; [0]: level-1 nodes that remain
    const uint32_t nt = g.ntrees < kTreesMax ? g.ntrees : kTreesMax;
    const uint32_t L = threadIdx.x & 63u;
    if (threadIdx.x == 0) {
        uint64_t a = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            const DiffTree& T = g.t[t];
            ifirst[t] = a;
            a += diff_items(diff_shape(T.n_a, T.cap_a, T.n_b, T.cap_b, T.len0));
        }
        ifirst[nt] = a;
    }
    __syncthreads();
    const uint64_t total = ifirst[nt];
    for (uint64_t q = blockIdx.x; q < total; q += gridDim.x) {
        uint32_t t = 0;
        while (q >= ifirst[t + 1]) ++t;  // q < ifirst[nt]
        t = __builtin_amdgcn_readfirstlane(t);  // workgroup-uniform: the descriptor by scalar loads
        const DiffTree& T = g.t[t];
        const DiffShape s = diff_shape(T.n_a, T.cap_a, T.n_b, T.cap_b, T.len0);
        const uint64_t j0 = q - ifirst[t];
        const uint32_t h0 = s.h0;
        // the subtree's root: the common case ends here
        if (h0 >= 1 && diff_comparable(s, h0, j0) &&
            !diff_node_ne(T.a_levels + 32 * diff_node_a(s, h0, j0), T.b_levels + 32 * diff_node_b(s, h0, j0)))
            continue;
        __syncthreads();  // the lists of this workgroup's previous item are free
        if (threadIdx.x == 0) {
            for (uint32_t d = 0; d <= kDiffHeight; ++d) cnt[d] = 0;
            front[0][0] = 0;
            if (h0 >= 2) {
                front[0][1] = 1;
                cnt[h0 - 1] = diff_visited(s, h0 - 1, 2 * j0 + 1) ? 2u : 1u;
            } else {
                cnt[0] = 1;  // level-1 node j0, or chunk 0 of a tree without levels
            }
        }
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t d = h0 >= 2 ? h0 - 1 : 0; d >= 1; --d) {
            const uint32_t F = cnt[d];                 // <= 2^(h0 - d)
            const uint64_t jbase = j0 << (h0 - d);     // the subtree's first node of level d
            const uint8_t* la = T.a_levels + 32 * diff_node_a(s, d, jbase);
            const uint8_t* lb = T.b_levels + 32 * diff_node_b(s, d, jbase);
            for (uint32_t base = 0; base < F; base += kDiffThreads) {
                const uint32_t f = base + threadIdx.x;
                uint32_t local = 0;
                bool go = false, two = false;
                if (f < F) {
                    local = front[cur][f];
                    const uint64_t j = jbase + local;
                    go = !diff_comparable(s, d, j) || diff_node_ne(la + 32ull * local, lb + 32ull * local);
                    two = go && d >= 2 && diff_visited(s, d - 1, 2 * j + 1);
                }
                const uint64_t b1 = __ballot(go), b2 = __ballot(two);
                if (b1 == 0) continue;  // wave-uniform
                const uint32_t add = (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
                uint32_t at = 0;
                if (L == 0) at = atomicAdd(&cnt[d - 1], add);  // one LDS add per wave
                at = __builtin_amdgcn_readfirstlane(at) + diff_lanes_below(b1) + diff_lanes_below(b2);
                if (go) {
                    front[cur ^ 1][at] = d >= 2 ? 2 * local : local;
                    if (two) front[cur ^ 1][at + 1] = 2 * local + 1;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        // the leaves under the level-1 nodes that remain: per values each, those below m
        const uint32_t F = cnt[0], per = 2 * s.p, E = F * per;  // <= 2^9 * 256
        const uint64_t j1base = h0 >= 1 ? j0 << (h0 - 1) : 0;
        DiffReport* rep = g.reports + t;
        for (uint32_t base = 0; base < E; base += kDiffThreads) {
            const uint32_t e = base + threadIdx.x;
            bool ne = false;
            uint64_t i = 0;
            if (e < E) {
                const uint32_t f = e / per, v = e - f * per;
                i = (j1base + front[cur][f]) * per + v;
                if (i < s.m) {
                    if (s.len0 == 32u && ((((uintptr_t)T.a_leaves) | ((uintptr_t)T.b_leaves)) & 15u) == 0)
                        ne = diff_node_ne(T.a_leaves + 32 * i, T.b_leaves + 32 * i);
                    else
                        ne = diff_leaf_ne(T.a_leaves + i * s.len0, T.b_leaves + i * s.len0, s.len0);
                }
            }
            const uint64_t bal = __ballot(ne);
            if (bal == 0) continue;  // wave-uniform
            const uint32_t leader = (uint32_t)__ffsll((long long)bal) - 1u;
            uint32_t lo = 0, hi = 0;
            if (L == leader) {  // one add per wave reserves its slots
                const uint64_t got = __hip_atomic_fetch_add(&rep->total, (uint64_t)__popcll(bal), __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT);
                lo = (uint32_t)got, hi = (uint32_t)(got >> 32);
            }
            lo = __builtin_amdgcn_readlane(lo, leader), hi = __builtin_amdgcn_readlane(hi, leader);
            const uint64_t slot = (((uint64_t)hi << 32) | lo) + diff_lanes_below(bal);
            if (ne && slot < T.max_out) T.idx_out[slot] = i;
            uint64_t mn = ne ? i : ~0ull;
#pragma unroll
            for (uint32_t o = 32; o >= 1; o >>= 1) {
                const uint64_t other = __shfl_xor(mn, (int)o);
                mn = other < mn ? other : mn;
            }
            if (L == leader)
                (void)__hip_atomic_fetch_min(&rep->first_index, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(64) void k_diff_reports(DiffReport* reports, uint32_t count) {
    if (threadIdx.x >= count) return;
    reports[threadIdx.x].total = 0;
    reports[threadIdx.x].first_index = ~0ull;
}

// ----------------------------------------------------------------------------
// Undo journal of resident trees (the slot map:
// tree_journal.hpp).  k_trees_journal runs BEFORE an update of the same trees
// on the same stream and saves what that update may overwrite of the old
// state: per work item (a listed index, or the last old value when the list
// grows) the value, its level-0 entry and node (chunk >> d) of every stored
// level, then the tree's root, and the container message with its root.
// k_trees_restore is the same walk with the two sides swapped; a work item's
// value index then comes from the journal (clamped again, so a journal that
// was never written still reaches no byte outside the tree).  Slice blockIdx.y
// of the grid is one tree, the slice behind the trees the container; a thread
// moves one piece of tree_journal.hpp and writes nothing else: a gather and a
// scatter, no counters, no hand-off.  Two work items under one node write the
// same bytes to it on the way back.
namespace {

__device__ __forceinline__ void journal_move(uint8_t* dst, const uint8_t* src, uint32_t len) {
    if (len == 16)
        *reinterpret_cast<copy_global_u32x4*>((uintptr_t)dst) = *reinterpret_cast<const copy_global_u32x4*>((uintptr_t)src);
    else if (len == 8)
        *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(src);
    else if (len == 4)
        *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
    else
        *dst = *src;
}

template <bool RESTORE>
__device__ __forceinline__ void journal_run(const JournalArgs& g) {
    const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x, gid = g0 + threadIdx.x;
    if (blockIdx.y >= g.ntrees) {  // the container: 4-byte pieces of the message (the last one in bytes), then of its root
        const uint32_t words = (g.container_len + 3) / 4;
        if (gid >= words + 8) return;
        uint8_t *t, *j;
        uint32_t len = 4;
        if (gid < words) {
            t = g.container + 4 * gid;
            j = g.jr_container + 4 * gid;
            if (4 * gid + 4 > g.container_len) len = g.container_len - 4 * (uint32_t)gid;  // 1 .. 3
        } else {
            t = g.container_root + 4 * (gid - words);
            j = g.jr_container + journal_up16(g.container_len) + 4 * (gid - words);
        }
        if (len == 4) {
            journal_move(RESTORE ? t : j, RESTORE ? j : t, 4);
        } else {
            for (uint32_t b = 0; b < len; ++b) (RESTORE ? t : j)[b] = (RESTORE ? j : t)[b];
        }
        return;
    }
    const JournalSeg& s = g.s[blockIdx.y];
    const JournalShape sh = journal_shape(s.n_old, s.n_new, s.capacity, s.k_idx, s.item_len, s.level0 != nullptr);
    if (g0 >= journal_pieces(sh, s.unit)) return;  // the whole block: another segment is the larger one
    const JournalPiece pc = journal_piece(sh, s.unit, gid);
    if (pc.kind == kJournalNone) return;
    uint8_t* j = s.jr + pc.jr_off;
    if (pc.kind == kJournalRoot) {
        uint8_t* t = s.root + pc.at;
        journal_move(RESTORE ? t : j, RESTORE ? j : t, 4);
        return;
    }
    const uint64_t* listed = RESTORE ? reinterpret_cast<const uint64_t*>(s.jr) : s.idx;
    const uint64_t x = journal_value(sh, pc.w, pc.w < sh.k_idx ? listed[pc.w] : 0);
    if (pc.kind == kJournalIndex) {
        if (!RESTORE) *reinterpret_cast<uint64_t*>(j) = x;
        return;
    }
    uint8_t* t = pc.kind == kJournalItem     ? s.items + x * s.item_len + pc.at
                 : pc.kind == kJournalLevel0 ? s.level0 + 32 * x + pc.at
                                             : s.levels + journal_node_off(sh, x, pc.level) + pc.at;
    journal_move(RESTORE ? t : j, RESTORE ? j : t, pc.len);
}

}  // namespace

__global__ __launch_bounds__(256) void k_trees_journal(JournalArgs g) { journal_run<false>(g); }
__global__ __launch_bounds__(256) void k_trees_restore(JournalArgs g) { journal_run<true>(g); }

}  // namespace mk
