// The fused tree tops: the arrival counters g_arrive, every kernel that touches them
// (k_trie_top_fused, k_merkle_top_fused, k_struct_list_fused) and k_spread_leaf, which shares their
// level helpers.  g_arrive is private to the translation unit and named in no other file.
// A part of the one kernel translation unit: merkle_kernels.hip includes it inside its open `namespace mk`,
// where these lines have always stood, so this file opens no namespace of its own (closing the namespace
// between two parts moves kernels in the code object).  Built as an object of its own it would emit other
// code for the same text ("Kernel files").
#ifndef MK_KERNEL_UNIT
#error "kernels_top.hip is built through merkle_kernels.hip"
#endif

// ----------------------------------------------------------------------------
// Fused tree tops (round 6): every level above a complete level of a tree in
// ONE launch, for the callers that build one tree at a time (one trie from
// its deposits, powchain/service.go:366-386; one state root,
// core/state/state.go:168-174), where the latency-bound levels, not the
// throughput passes, set the call's time.  Workgroup b reduces its NT nodes
// of the start level to one node log2(NT) levels up inside the workgroup --
// per level, bit-interleaved lane pairs (mk::ilv) while the parents outnumber
// the waves, one state per wave (mk::spread) after (a level of <= 16 parents
// costs one spread permutation, ~6.3 k cycles, instead of one lane-pair
// permutation, ~12.8 k) -- then publishes that node (write-through store,
// drained) and bumps an arrival counter; the LAST workgroup to arrive loads
// the published nodes and reduces them to the root.  No launch boundary, no
// narrow one-workgroup launch waiting for the wide one.

// Arrival counters of the fused tops, one per launch in flight (the host
// hands out slots round-robin, merkle_api.cpp next_arrive_slots); zero at module
// load, and the last arriver of a launch resets its slot, so at most
// kArriveSlots fused launches may be in flight on one device.
__device__ uint32_t g_arrive[kArriveSlots];
// Diagnostic build only (tools/top_probe.hip: -DMK_TOP_STAMPS=1; the default, 0,
// is in hash_dev.hpp): s_memtime at each level of a fused top, per workgroup;
// never in the shipped library.
#if MK_TOP_STAMPS
__device__ uint64_t g_top_stamps[1024 * 64];
#define TOP_STAMP(k) \
    do { if (threadIdx.x == 0) g_top_stamps[blockIdx.x * 64 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TOP_STAMP(k) \
    do { (void)(k); } while (0)
#endif

namespace {

// ilv words (e, o) of a 64-bit lane -> its plain (lo, hi) dwords
__device__ __forceinline__ void ilv_to_plain(uint32_t e, uint32_t o, uint32_t& lo, uint32_t& hi) {
    lo = ilv::spread16(e) | (ilv::spread16(o) << 1);
    hi = ilv::spread16(e >> 16) | (ilv::spread16(o >> 16) << 1);
}

// One level of a fused top inside the workgroup (every thread calls it): the
// m <= NT nodes in lds (ilv words: node k at lds[8 k + 2 w + p]) -> ceil(m/2)
// parents at lds[8 j ..].  TRIE: K(l || r) with a missing r = 0^32, 64 B
// (deposit_trie.go:33-38); otherwise merkleHash's rule: the unpaired last
// node is K(l || 0^128), 160 B (hash.go:229-236).  The form follows the
// parent count (cycles per level measured in-kernel, tools/top_probe.hip):
//   > 256 parents: one state per lane (two waves per SIMD; 512 parents
//       ~39 k cycles, against ~44 k as lane pairs at four waves per SIMD;
//       256 parents as lane pairs at two waves per SIMD: one trie -0.6 us,
//       one state -0.9 us against one state per lane at one wave per SIMD,
//       3 interleaved rounds, profiles/r06/lane257/);
//   > NT/128: bit-interleaved lane pairs (mk::ilv: ~13 k cycles a level for
//       up to one wave per SIMD; 16 parents in one wave 12.8 k, against
//       17.8 k as 16 spread waves, four per SIMD);
//   <= NT/128 (<= two waves per SIMD): one state per wave (mk::spread).
// Each parent also goes to lane_out(j, d0, d1) (plain digest), pair_out(j,
// words, p) (ilv words of a lane pair) or wave_out(j, e, o, L) (lanes 0..3
// of the wave hold the digest's ilv words).
// parents from which a level runs one state per lane (below: lane pairs)
constexpr uint32_t kTopLaneMin = 257;
template <uint32_t NT, bool TRIE, typename LaneOut, typename PairOut, typename WaveOut>
__device__ __forceinline__ void wg_level(uint32_t* lds, uint32_t m, const spread::Lane& cst, LaneOut&& lane_out,
                                         PairOut&& pair_out, WaveOut&& wave_out) {
    const uint32_t tid = threadIdx.x, mn = (m + 1) / 2;
    const uint32_t w = tid >> 6, L = tid & 63u, i = cst.i;
    // spread form (one parent per wave): wave `sw` hashes parent `j`
    auto spread_load = [&](uint32_t j, uint32_t& e, uint32_t& o) {
        const bool right = 2 * j + 1 < m;
        e = o = 0u;
        if (i < 4u) {
            e = lds[16 * j + 2 * i];
            o = lds[16 * j + 2 * i + 1];
        } else if (i < 8u && right) {
            e = lds[16 * j + 8 + 2 * (i - 4u)];
            o = lds[16 * j + 8 + 2 * (i - 4u) + 1];
        }
    };
    auto spread_hash = [&](uint32_t j, uint32_t& e, uint32_t& o) {
        if (!TRIE && !(2 * j + 1 < m)) {  // K(l || 0^128): 160 bytes, two blocks
            spread::keccak_f(e, o, cst);
            if (i == 3u) e ^= 1u;
        } else if (i == 8u) {
            e ^= 1u;
        }
        if (i == 16u) o ^= 0x80000000u;
        spread::keccak_f(e, o, cst);
    };
    auto spread_store = [&](uint32_t j, uint32_t e, uint32_t o) {
        if (L < 4u) {
            lds[8 * j + 2 * L] = e;
            lds[8 * j + 2 * L + 1] = o;
            wave_out(j, e, o, L);
        }
    };
    if (mn > NT / 128) {
        // The unpaired last node of an odd merkleHash level is K(l || 0^128),
        // two permutations: the last wave hashes it in spread form (2 x ~7 k
        // cycles) beside the lane / pair forms' one permutation (13-20 k),
        // where as one of theirs it doubled the level (C3's registry top: the
        // 123 -> 62 and 31 -> 16 levels 29.6 k and 32.5 k cycles,
        // tools/top_probe.hip)
        const bool side = !TRIE && (m & 1u) && 2 * (mn - 1) <= NT - 64;
        const uint32_t mh = side ? mn - 1 : mn;  // parents of the lane / pair forms
        const bool sw = side && w == NT / 64 - 1;
        uint32_t e = 0u, o = 0u;
        if (sw) spread_load(mn - 1, e, o);
        if (mh >= kTopLaneMin) {  // one state per lane
            const bool act = tid < mh;
            const bool right = 2 * tid + 1 < m;
            State s;
            if (act) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ilv_to_plain(lds[16 * tid + 2 * q], lds[16 * tid + 2 * q + 1], s.lo[q], s.hi[q]);
                    if (right)
                        ilv_to_plain(lds[16 * tid + 8 + 2 * q], lds[16 * tid + 8 + 2 * q + 1], s.lo[4 + q],
                                     s.hi[4 + q]);
                    else
                        s.lo[4 + q] = s.hi[4 + q] = 0u;
                }
            }
            __syncthreads();
            if (act) {
#pragma unroll
                for (int q = 8; q < 25; ++q) s.lo[q] = s.hi[q] = 0u;
                if (!TRIE && !right) {  // K(l || 0^128): block 1 = l || 0, block 2 = 0^24 || pad
                    keccak_f(s);
                    s.lo[3] ^= 1u;
                } else {
                    s.lo[8] ^= 1u;  // byte 64
                }
                s.hi[16] ^= 0x80000000u;
                keccak_f_digest(s);
                uint4 d0, d1;
                digest(s, d0, d1);
                const uint32_t lo4[4] = {d0.x, d0.z, d1.x, d1.z}, hi4[4] = {d0.y, d0.w, d1.y, d1.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    lds[8 * tid + 2 * q] = ilv::to_ilv(lo4[q], hi4[q], 0);
                    lds[8 * tid + 2 * q + 1] = ilv::to_ilv(lo4[q], hi4[q], 1);
                }
                lane_out(tid, d0, d1);
            }
        } else {  // lane pairs
            const uint32_t k = tid >> 1, p = tid & 1u;
            const bool act = k < mh;
            uint32_t a[4], b[4] = {0, 0, 0, 0};
            bool padded = false;
            if (act) {
                const bool right = 2 * k + 1 < m;
                padded = !TRIE && !right;
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = lds[16 * k + 2 * q + p];
                if (right) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) b[q] = lds[16 * k + 8 + 2 * q + p];
                }
            }
            __syncthreads();
            if (act) {
                uint32_t h[4];
                hash_pair3(a, b, padded, p, h);
#pragma unroll
                for (int q = 0; q < 4; ++q) lds[8 * k + 2 * q + p] = h[q];
                pair_out(k, h, p);
            }
        }
        if (sw) {
            spread_hash(mn - 1, e, o);
            spread_store(mn - 1, e, o);
        }
    } else {  // one parent per wave
        // parent j on wave j: a workgroup's waves go to its SIMDs round-robin
        // (wave w on SIMD w mod 4), so the first 4 parents get a SIMD each
        // (parents 0..3 on waves 0, 4, 8, 12 -- one SIMD -- took 15.9 k
        // cycles a level against 7.8 k, tools/top_probe.hip, profiles/r06/single/)
        const uint32_t j = w;
        uint32_t e = 0u, o = 0u;
        if (j < mn) spread_load(j, e, o);  // wave-uniform
        __syncthreads();
        if (j < mn) {
            spread_hash(j, e, o);
            spread_store(j, e, o);
        }
    }
    __syncthreads();
}

// plain node j of `in` (32 B, `stride` nodes apart) -> lds as ilv words,
// thread t loading node t; SC1: agent-scope loads (nodes another CU
// published in this launch)
template <bool SC1>
__device__ __forceinline__ void wg_load_nodes(uint32_t* lds, const uint32_t* in, uint32_t m, uint32_t stride = 1) {
    const uint32_t t = threadIdx.x;
    if (t < m) {
        const uint64_t* q = reinterpret_cast<const uint64_t*>(in) + 4 * (uint64_t)t * stride;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint64_t v = SC1 ? __hip_atomic_load(q + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : q[w];
            lds[8 * t + 2 * w] = ilv::to_ilv((uint32_t)v, (uint32_t)(v >> 32), 0);
            lds[8 * t + 2 * w + 1] = ilv::to_ilv((uint32_t)v, (uint32_t)(v >> 32), 1);
        }
    }
    __syncthreads();
}

// node 0 of lds (ilv words) -> plain 32 B at out, by wave 0's lanes 0..3;
// SC1: a write-through store, drained, so another CU may read it after the
// arrival counter says so
template <bool SC1>
__device__ __forceinline__ void wg_store_node0(const uint32_t* lds, uint32_t* out) {
    const uint32_t tid = threadIdx.x;
    if (tid < 4u) {
        const uint32_t e = lds[2 * tid], o = lds[2 * tid + 1];
        const uint64_t v = (uint64_t)(ilv::spread16(e) | (ilv::spread16(o) << 1)) |
                           ((uint64_t)(ilv::spread16(e >> 16) | (ilv::spread16(o >> 16) << 1)) << 32);
        uint64_t* q = reinterpret_cast<uint64_t*>(out) + tid;
        if (SC1)
            __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            *q = v;
    }
    if (SC1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Arrival of this workgroup (after its published node's store drained); true
// in every thread of the last of `total` workgroups, which also resets the slot.
__device__ __forceinline__ bool wg_arrive_last(uint32_t slot, uint32_t total, uint32_t* flag) {
    if (threadIdx.x == 0) {
        const uint32_t old = __hip_atomic_fetch_add(&g_arrive[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = old + 1 == total;
        if (last) __hip_atomic_store(&g_arrive[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = last ? 1u : 0u;
    }
    __syncthreads();
    return *flag != 0u;
}

}  // namespace

// The deposit trie above its complete level d0 (c0 nodes) up to the root, in
// one launch: workgroup b takes level-d0 nodes [NT b, NT b +
// NT) up to level d0 + log2(NT) (every node stored: GenerateMerkleBranch reads
// them), the last workgroup to arrive the rest, including the zero-sibling
// levels (deposit_trie.go:33-38) and the root.  grid = ceil(c0 / NT) <= NT;
// a grid of more than kTopGroup workgroups also uses the arrival slots after
// `slot`, one per group of each stage: the top_arrive_slots(grid) slots the
// host reserved for this launch (never more than kTopGroupSlots).
template <uint32_t NT>
__global__ __launch_bounds__(NT) void k_trie_top_fused(uint32_t* __restrict__ levels, uint64_t cap, uint64_t c0,
                                                       uint32_t d0, uint32_t depth, uint32_t* __restrict__ root_out,
                                                       uint32_t slot) {
    constexpr uint32_t kLog = NT == 1024 ? 10 : NT == 512 ? 9 : NT == 256 ? 8 : NT == 128 ? 7 : 6;
    __shared__ uint32_t lds[8 * NT];
    __shared__ uint32_t flag;
    uint64_t off = 0, capd = cap;  // node offset and capacity of level d
    for (uint32_t k = 0; k < d0; ++k) {
        off += capd;
        capd = (capd + 1) / 2;
    }
    const uint32_t dtop = depth - d0 < kLog ? depth : d0 + kLog;  // this workgroup's part ends at level dtop
    uint64_t lo = (uint64_t)blockIdx.x * NT;                      // level-d node of lds[0]
    uint32_t m = (uint32_t)(c0 - lo < NT ? c0 - lo : NT);
    wg_load_nodes<false>(lds, levels + 8 * (off + lo), m);
    uint32_t d = d0;
    const uint32_t L = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const spread::Lane cst = spread::lane_consts(L);
    uint32_t nst = 0;
    TOP_STAMP(nst++);
    auto run = [&](uint32_t d_end) {
        for (; d < d_end && m > 1; ++d) {
            TOP_STAMP(nst++);
            uint32_t* out = levels + 8 * (off + capd + (lo >> 1));  // level d + 1, this part's first parent
            wg_level<NT, true>(
                lds, m, cst,
                [&](uint32_t j, const uint4& d0, const uint4& d1) {
                    reinterpret_cast<uint4*>(out)[2 * j] = d0;
                    reinterpret_cast<uint4*>(out)[2 * j + 1] = d1;
                },
                [&](uint32_t j, const uint32_t(&h)[4], uint32_t p) { store_node3(out, j, false, p, h); },
                [&](uint32_t j, uint32_t e, uint32_t o, uint32_t L) { spread_store_digest(e, o, L, out + 8 * j); });
            m = (m + 1) / 2;
            lo >>= 1;
            off += capd;
            capd = (capd + 1) / 2;
        }
        if (d < d_end) {
            // one node left: the zero-sibling levels K(node || 0^32) as a
            // chain on wave 0, the node kept in registers as plain (lo, hi)
            // words (no LDS round trip, no barrier, no bit (de)interleave per
            // level; the lo/hi round, 6.29 k cycles a permutation against
            // 6.44 k, profiles/r02d/lat_probe_spread.json)
            const spread::LaneLH ch = spread::lane_consts_lh(L);
            const uint32_t i = ch.i;
            uint32_t lo32 = 0u, hi32 = 0u;
            if (w == 0 && i < 4u) ilv_to_plain(lds[2 * i], lds[2 * i + 1], lo32, hi32);
            for (; d < d_end; ++d) {
                TOP_STAMP(nst++);
                if (w == 0) {
                    if (i >= 4u) lo32 = hi32 = 0u;
                    if (i == 8u) lo32 ^= 1u;
                    if (i == 16u) hi32 ^= 0x80000000u;
                    spread::keccak_f_lh(lo32, hi32, ch);
                    if (L < 4u)
                        reinterpret_cast<uint2*>(levels + 8 * (off + capd + (lo >> 1)))[L] = make_uint2(lo32, hi32);
                }
                lo >>= 1;
                off += capd;
                capd = (capd + 1) / 2;
            }
            if (w == 0 && L < 4u) {
                lds[2 * L] = ilv::to_ilv(lo32, hi32, 0);
                lds[2 * L + 1] = ilv::to_ilv(lo32, hi32, 1);
            }
            __syncthreads();
        }
    };
    run(dtop);
    if (gridDim.x > 1) {
        // publish this part's node (level dtop, node blockIdx.x: already
        // stored above, again write-through) and arrive
        wg_store_node0<true>(lds, levels + 8 * (off + lo));
        TOP_STAMP(nst++);
        uint32_t parts = gridDim.x;  // nodes of level d, one published per workgroup
        uint32_t gslot = slot + 1;   // arrival slots of this stage's groups
        while (kTopGroupLog2 > 0 && parts > kTopGroup) {
            // the last of each kTopGroup workgroups of a stage takes its
            // group's nodes log2(kTopGroup) levels up, so those levels run on
            // many CUs at once, not one after another on a lone workgroup (a
            // missing right sibling is 0^32 here too)
            const uint32_t b = (uint32_t)lo;  // this workgroup's node of level d
            const uint32_t grp = b / kTopGroup, g0 = grp * kTopGroup;
            const uint32_t members = parts - g0 < kTopGroup ? parts - g0 : kTopGroup;
            const uint32_t groups = (parts + kTopGroup - 1) / kTopGroup;
            if (!wg_arrive_last(gslot + grp, members, &flag)) return;
            TOP_STAMP(nst++);
            lo = g0;
            m = members;
            wg_load_nodes<true>(lds, levels + 8 * (off + lo), m);
            run(d + kTopGroupLog2);
            wg_store_node0<true>(lds, levels + 8 * (off + lo));
            TOP_STAMP(nst++);
            gslot += groups;
            parts = groups;
        }
        if (!wg_arrive_last(slot, parts, &flag)) return;
        TOP_STAMP(nst++);
        lo = 0;
        m = parts;
        wg_load_nodes<true>(lds, levels + 8 * off, m);
    }
    run(depth);
    wg_store_node0<false>(lds, root_out);
    TOP_STAMP(nst++);
}
template __global__ void k_trie_top_fused<1024>(uint32_t*, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t*,
                                                uint32_t);

// merkleHash above a complete level of one or two lists' trees, to the list
// roots with the length mix-in (hash.go:194-239), in one launch: list l's
// workgroups [wg0, wg0 + nwg) reduce 2^span_log2 nodes each by span_log2
// levels (a ragged last part keeps the odd rule at count 1: the other parts
// are even at every level below, so its count's parity is the level's),
// publish their node to `sub`, and the last to arrive reduces the nwg nodes
// to the root and mixes in the length.  Two lists (the State's registry and
// balances, hash.go:141-159): each list's last workgroup is one finisher of
// the pair block (wave3_spread_final), the second to complete hashes the
// struct root -- the two trees' latency-bound tops run side by side in one
// launch on one stream, where the "level1" schedule ran four launches on two
// streams with an event between them.
template <uint32_t NT>
__global__ __launch_bounds__(NT) void k_merkle_top_fused(MerkleTopArgs a) {
    __shared__ uint32_t lds[8 * NT];
    __shared__ uint32_t flag;
    const uint32_t li = a.nlists > 1 && blockIdx.x >= a.l[1].wg0 ? 1u : 0u;
    const MerkleTopList t = li ? a.l[1] : a.l[0];  // no dynamic index into the kernarg (scratch)
    const uint32_t b = blockIdx.x - t.wg0;
    const spread::Lane cst = spread::lane_consts(threadIdx.x & 63u);
    const uint64_t lo = (uint64_t)b << t.span_log2;
    const uint64_t span = 1ull << t.span_log2;
    uint32_t m = (uint32_t)(t.c - lo < span ? t.c - lo : span);
    wg_load_nodes<false>(lds, reinterpret_cast<const uint32_t*>(t.nodes) + 8 * lo, m);
    auto none3 = [](uint32_t, const uint4&, const uint4&) {};
    auto none_p = [](uint32_t, const uint32_t(&)[4], uint32_t) {};
    auto none_w = [](uint32_t, uint32_t, uint32_t, uint32_t) {};
    uint32_t nst = 0;
    TOP_STAMP(nst++);
    if (t.nwg > 1) {
        for (uint32_t k = 0; k < t.span_log2; ++k) {
            wg_level<NT, false>(lds, m, cst, none3, none_p, none_w);
            m = (m + 1) / 2;
            TOP_STAMP(nst++);
        }
        wg_store_node0<true>(lds, t.sub + 8 * b);
        // groups of kTopGroup parts first, as in k_trie_top_fused: the last of
        // each group takes the group's nodes log2(kTopGroup) levels up and
        // stores its node over the group's first (node idx of a stage at
        // sub[8 stride idx]).  Every group but a ragged last one is even at
        // each of those levels, so the ragged group's count has the level's
        // parity and a lone node there is the level's unpaired last node,
        // K(l || 0^128), as wg_level hashes it.
        uint32_t parts = t.nwg, stride = 1, idx = b, gslot = t.slot + 1;
        while (kTopGroupLog2 > 0 && parts > kTopGroup) {
            const uint32_t grp = idx / kTopGroup, g0 = grp * kTopGroup;
            const uint32_t members = parts - g0 < kTopGroup ? parts - g0 : kTopGroup;
            const uint32_t groups = (parts + kTopGroup - 1) / kTopGroup;
            if (!wg_arrive_last(gslot + grp, members, &flag)) return;
            m = members;
            wg_load_nodes<true>(lds, t.sub + 8 * stride * g0, m, stride);
            for (uint32_t k = 0; k < kTopGroupLog2; ++k) {
                wg_level<NT, false>(lds, m, cst, none3, none_p, none_w);
                m = (m + 1) / 2;
            }
            stride *= kTopGroup;
            idx = grp;
            wg_store_node0<true>(lds, t.sub + 8 * stride * idx);
            TOP_STAMP(nst++);
            gslot += groups;
            parts = groups;
        }
        if (!wg_arrive_last(t.slot, parts, &flag)) return;
        m = parts;
        wg_load_nodes<true>(lds, t.sub, m, stride);
        TOP_STAMP(nst++);
    }
    while (m > 1) {
        wg_level<NT, false>(lds, m, cst, none3, none_p, none_w);
        m = (m + 1) / 2;
        TOP_STAMP(nst++);
    }
    // the length mix-in K(root || le64(n) || 0^24) on wave 0 (spread form)
    const uint32_t L = threadIdx.x & 63u, i = cst.i;
    uint32_t e = 0u, o = 0u;
    if (threadIdx.x < 64) {
        if (i < 4u) {
            e = lds[2 * i];
            o = lds[2 * i + 1];
        } else if (i == 4u) {
            e = ilv::to_ilv((uint32_t)t.n_items, (uint32_t)(t.n_items >> 32), 0);
            o = ilv::to_ilv((uint32_t)t.n_items, (uint32_t)(t.n_items >> 32), 1);
        } else if (i == 8u) {
            e = 1u;
        }
        if (i == 16u) o ^= 0x80000000u;
        spread::keccak_f(e, o, cst);
    }
    if (a.nlists == 1) {
        if (threadIdx.x < 64) spread_store_digest(e, o, L, t.out);
        TOP_STAMP(nst++);
        return;
    }
    // Two lists: publish this list's root to its slot of the pair block
    // (write-through, drained) and arrive on the pair's counter; the second
    // list to arrive hashes the struct root K(root 0 || root 1) (hash.go:141-
    // 159) into pair[64..96).  Both finishers are in this launch, so an
    // arrival counter does what the epoch-tagged arrival word does between
    // two launches (wave3_spread_final), without its fences.
    __syncthreads();
    if (threadIdx.x < 64 && L < 4u) {
        lds[2 * L] = e;
        lds[2 * L + 1] = o;
    }
    __syncthreads();
    wg_store_node0<true>(lds, t.out);
    if (!wg_arrive_last(a.pair_slot, 2, &flag)) return;
    if (threadIdx.x < 64) {
        e = o = 0u;
        if (i < 8u) {  // lanes of Keccak lanes 0..3: list 0's root, 4..7: list 1's
            const uint64_t v = __hip_atomic_load(reinterpret_cast<const uint64_t*>(a.pair) + i, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            e = ilv::to_ilv((uint32_t)v, (uint32_t)(v >> 32), 0);
            o = ilv::to_ilv((uint32_t)v, (uint32_t)(v >> 32), 1);
        } else if (i == 8u) {
            e = 1u;  // byte 64
        }
        if (i == 16u) o ^= 0x80000000u;
        spread::keccak_f(e, o, cst);
        spread_store_digest(e, o, L, a.pair + 16);
    }
    TOP_STAMP(nst++);
}
template __global__ void k_merkle_top_fused<1024>(MerkleTopArgs);

// Small merkleHash leaf passes in spread form (one state per wave): a
// workgroup of 16 waves owns 16 windows; wave w hashes window w (256 B, the
// ragged last one, or one padded with 0^128: hash.go:205-222), then the
// workgroup folds them through up to 4 levels in LDS (parent w on wave w,
// K(l || r) or K(l || 0^128)), like k_wave3.  The final pass (<= 16
// windows) continues to the root and the length mix-in.  Where a tree's
// first level has few windows every wave runs nearly alone, and a window
// costs 2 x 6.3 k cycles here against 2 x 12.8 k in a lane pair.
// The body (every thread of the workgroup calls it): windows [SPAN blk,
// SPAN blk + SPAN); with STORE the pass's nodes go to a.out, else the
// workgroup's node (a.levels = 1 + log2 SPAN) is left in nodes[0..3].
template <uint32_t SPAN, bool STORE>
__device__ __forceinline__ void spread_leaf_body(const ReduceArgs& a, uint32_t w8, uint64_t blk, uint2 (&nodes)[64]) {
    static_assert(SPAN == 8 || SPAN == 16, "windows per workgroup");
    const uint32_t w = threadIdx.x >> 6, L = threadIdx.x & 63u;
    const spread::LaneLH cst = spread::lane_consts_lh(L);
    const uint32_t i = cst.i;
    const uint64_t lo1 = (a.wg_base + blk) * (uint64_t)SPAN;
    const uint64_t m1 = a.c1 - lo1 < SPAN ? a.c1 - lo1 : SPAN;
    if (w < m1) {  // wave-uniform
        const uint64_t j = lo1 + w;
        const uint64_t lo = j * 2 * a.cb;
        uint64_t la;
        uint32_t lz;
        if (2 * j + 1 < a.nchunks) {
            la = (lo + 2 * a.cb < a.total ? lo + 2 * a.cb : a.total) - lo;
            lz = 0;
        } else {
            la = a.total - lo;
            lz = 128;
        }
        uint32_t hlo, hhi;
        if (w8)
            spread_sponge<true>(a.items + lo, la, cst, hlo, hhi, lz);
        else
            spread_sponge<false>(a.items + lo, la, cst, hlo, hhi, lz);
        if (L < 4u) nodes[4 * w + L] = make_uint2(hlo, hhi);
    }
    __syncthreads();
    uint64_t c = a.c1, m = m1;
    int left = a.finalize ? 64 : (int)a.levels - 1;
    int done = 0;
    while (left > 0 && (c > 1 || a.pad_at_one)) {
        const uint64_t mn = (m + 1) / 2;
        uint32_t slo = 0u, shi = 0u;
        if (w < mn) {
            const bool padded = !(2 * (uint64_t)w + 1 < m);
            if (i < 4u) {
                const uint2 v = nodes[8 * w + i];
                slo = v.x;
                shi = v.y;
            } else if (i < 8u && !padded) {
                const uint2 v = nodes[8 * w + i];  // node 2w+1, word i-4
                slo = v.x;
                shi = v.y;
            }
            if (padded) {  // 160 bytes: two blocks
                spread::keccak_f_lh(slo, shi, cst);
                if (i == 3u) slo ^= 1u;
            } else if (i == 8u) {
                slo ^= 1u;
            }
            if (i == 16u) shi ^= 0x80000000u;
            spread::keccak_f_lh(slo, shi, cst);
        }
        __syncthreads();
        if (w < mn && L < 4u) nodes[4 * w + L] = make_uint2(slo, shi);
        __syncthreads();
        c = (c + 1) / 2;
        m = mn;
        --left;
        ++done;
    }
    uint2* out = reinterpret_cast<uint2*>(a.out);
    if (a.finalize) {
        if (w == 0) {  // K(root || le64(n) || 0^24)
            uint32_t slo = 0u, shi = 0u;
            if (i < 4u) {
                const uint2 v = nodes[i];
                slo = v.x;
                shi = v.y;
            } else if (i == 4u) {
                slo = (uint32_t)a.n_items;
                shi = (uint32_t)(a.n_items >> 32);
            } else if (i == 8u) {
                slo = 1u;
            }
            if (i == 16u) shi ^= 0x80000000u;
            spread::keccak_f_lh(slo, shi, cst);
            if (L < 4u) out[L] = make_uint2(slo, shi);
        }
    } else if (STORE && w < m && L < 4u) {
        out[4 * ((lo1 >> done) + w) + L] = nodes[4 * w + L];
    }
}
template <uint32_t SPAN>
__global__ __launch_bounds__(1024) void k_spread_leaf(ReduceArgs a, uint32_t w8) {
    __shared__ uint2 nodes[16 * 4];
    spread_leaf_body<SPAN, true>(a, w8, blockIdx.x, nodes);
}
template __global__ void k_spread_leaf<16>(ReduceArgs, uint32_t);
template __global__ void k_spread_leaf<8>(ReduceArgs, uint32_t);

// TreeHash of a small list of structs in ONE launch (round 6: C1, 16,384
// ValidatorRecords, hash.go:118-159 -> 194-239): workgroup b hashes records
// [64 b, 64 b + 64) as k_struct_split does (the fields side by side, the
// struct message on a lane pair; roots to `roots`), then their 8 windows
// and 3 levels as k_spread_leaf<8> does (one window per wave), publishes
// its node (write-through, drained) and arrives; groups of kTopGroup
// workgroups and the last one take the nodes to the list root and the
// length mix-in as k_merkle_top_fused does.  Three launches' boundaries
// and the roots' trip through a second kernel go away.  `a` is the window
// pass over `roots` (a.levels = 4); sub: one published node per workgroup.
template <int NB, int NRAW>
__global__ __launch_bounds__(1024) void k_struct_list_fused(const uint8_t* __restrict__ rec, uint64_t n, StructSpec sp,
                                                            uint32_t vec16, uint4* __restrict__ roots, ReduceArgs a,
                                                            uint32_t* __restrict__ sub, uint32_t* __restrict__ out,
                                                            uint32_t slot) {
    __shared__ uint32_t dg[NB * 8][64];
    __shared__ uint2 nodes[16 * 4];
    __shared__ uint32_t lds[8 * 1024];
    __shared__ uint32_t flag;
    constexpr uint32_t NT = 1024;
    const uint32_t b = blockIdx.x, nwg = gridDim.x;
    struct_split_body<NB, NRAW>(rec, n, sp, vec16, roots, b, dg);
    __threadfence_block();  // this workgroup's roots, read back by its own waves below
    __syncthreads();
    spread_leaf_body<8, false>(a, 1u, b, nodes);
    // publish node b: plain (lo, hi) words of lanes 0..3, write-through, drained
    if (threadIdx.x < 4u) {
        const uint2 v = nodes[threadIdx.x];
        __hip_atomic_store(reinterpret_cast<uint64_t*>(sub) + 4 * b + threadIdx.x,
                           (uint64_t)v.x | ((uint64_t)v.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const spread::Lane cst = spread::lane_consts(threadIdx.x & 63u);
    auto none3 = [](uint32_t, const uint4&, const uint4&) {};
    auto none_p = [](uint32_t, const uint32_t(&)[4], uint32_t) {};
    auto none_w = [](uint32_t, uint32_t, uint32_t, uint32_t) {};
    uint32_t m = 1;
    // as k_merkle_top_fused: groups of kTopGroup parts first, each group's
    // last arriver takes its nodes log2(kTopGroup) levels up (a ragged last
    // group's count has the level's parity: a lone node is the level's
    // unpaired last node, K(l || 0^128))
    uint32_t parts = nwg, stride = 1, idx = b, gslot = slot + 1;
    while (kTopGroupLog2 > 0 && parts > kTopGroup) {
        const uint32_t grp = idx / kTopGroup, g0 = grp * kTopGroup;
        const uint32_t members = parts - g0 < kTopGroup ? parts - g0 : kTopGroup;
        const uint32_t groups = (parts + kTopGroup - 1) / kTopGroup;
        if (!wg_arrive_last(gslot + grp, members, &flag)) return;
        m = members;
        wg_load_nodes<true>(lds, sub + 8 * stride * g0, m, stride);
        for (uint32_t k = 0; k < kTopGroupLog2; ++k) {
            wg_level<NT, false>(lds, m, cst, none3, none_p, none_w);
            m = (m + 1) / 2;
        }
        stride *= kTopGroup;
        idx = grp;
        wg_store_node0<true>(lds, sub + 8 * stride * idx);
        gslot += groups;
        parts = groups;
    }
    if (!wg_arrive_last(slot, parts, &flag)) return;
    m = parts;
    wg_load_nodes<true>(lds, sub, m, stride);
    while (m > 1) {
        wg_level<NT, false>(lds, m, cst, none3, none_p, none_w);
        m = (m + 1) / 2;
    }
    // the length mix-in K(root || le64(n) || 0^24) on wave 0 (spread form)
    if (threadIdx.x < 64) {
        const uint32_t L = threadIdx.x, i = cst.i;
        uint32_t e = 0u, o = 0u;
        if (i < 4u) {
            e = lds[2 * i];
            o = lds[2 * i + 1];
        } else if (i == 4u) {
            e = ilv::to_ilv((uint32_t)n, (uint32_t)(n >> 32), 0);
            o = ilv::to_ilv((uint32_t)n, (uint32_t)(n >> 32), 1);
        } else if (i == 8u) {
            e = 1u;
        }
        if (i == 16u) o ^= 0x80000000u;
        spread::keccak_f(e, o, cst);
        spread_store_digest(e, o, L, out);
    }
}
template __global__ void k_struct_list_fused<3, 6>(const uint8_t*, uint64_t, StructSpec, uint32_t, uint4*, ReduceArgs,
                                                   uint32_t*, uint32_t*, uint32_t);
