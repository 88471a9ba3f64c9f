// Struct hashing (hash.go:141-159) of fixed-layout records: k_struct_fields, k_struct_fused,
// k_struct_nested, k_struct_reg, k_struct_lock, k_struct_split and their helpers (kernels_struct_list.hip
// uses k_struct_nested's column helpers).
// A part of the one kernel translation unit: merkle_kernels.hip includes it inside its open `namespace mk`,
// where these lines have always stood, so this file opens no namespace of its own (closing the namespace
// between two parts moves kernels in the code object).  Built as an object of its own it would emit other
// code for the same text ("Kernel files").
#ifndef MK_KERNEL_UNIT
#error "kernels_struct.hip is built through merkle_kernels.hip"
#endif

// ----------------------------------------------------------------------------
// Struct hashing (hash.go:141-159) for flat fixed-layout records: every
// record's message is the concatenation, in declaration order, of
//   MK_FIELD_BYTES: Keccak(le32(len) || bytes)   (hashedEncoding, hash.go:100-107)
//   MK_FIELD_RAW:   the raw little-endian bytes  (getEncoding of bool/uintN)
// k_struct_fields writes those messages; k_keccak_fixed hashes them.

// Keccak(le32(len) || A[0, len)) in one block, dword-granular: dword 0 =
// le32(len), dwords 1.. = bytes (len % 4 == 0, len + 4 < 136, A 4-byte aligned)
__device__ __forceinline__ void bytes_block_digest(const uint8_t* __restrict__ A, uint32_t len, uint4& d0,
                                                   uint4& d1) {
    const uint32_t* A32 = reinterpret_cast<const uint32_t*>(A);
    const uint32_t nd = len / 4 + 1;  // message dwords
    State s;
    zero(s);
#pragma unroll
    for (int q = 0; q < 34; ++q) {
        uint32_t v = q == 0 ? len : ((uint32_t)q < nd ? A32[q - 1] : 0u);
        if ((uint32_t)q == nd) v ^= 1u;  // domain pad byte
        if (q & 1)
            s.hi[q / 2] ^= v;
        else
            s.lo[q / 2] ^= v;
    }
    s.hi[16] ^= 0x80000000u;
    keccak_f_digest(s);
    digest(s, d0, d1);
}

template <bool FAST>
__global__ __launch_bounds__(256) void k_struct_fields(const uint8_t* __restrict__ rec, uint64_t n, StructSpec sp,
                                                       uint8_t* __restrict__ msg) {
    // one thread per (record, field): field-major so neighbouring lanes hash
    // the same field of neighbouring records
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * sp.nfields) return;
    const uint32_t f = (uint32_t)(t / n);
    const uint64_t i = t - (uint64_t)f * n;
    const uint8_t* r = rec + i * sp.rec_len;
    uint8_t* m = msg + i * sp.msg_len;
    const uint32_t off = sp.off[f], len = sp.len[f], out = sp.out_off[f];
    if (sp.kind[f] == 1) {  // MK_FIELD_BYTES
        uint4 d0, d1;
        if constexpr (FAST) {  // host-checked: every bytes field has len % 4 == 0, len + 4 < 136
            bytes_block_digest(r + off, len, d0, d1);
        } else {
            sponge_prefix4(r + off, len, d0, d1);
        }
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        if ((out & 3u) == 0 && (((uintptr_t)m) & 3u) == 0) {
            uint32_t* o = reinterpret_cast<uint32_t*>(m + out);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = dw[k];
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k) m[out + k] = (uint8_t)(dw[k / 4] >> (8 * (k % 4)));
        }
    } else if (len == 8 && ((off | out) & 7u) == 0 && ((((uintptr_t)r) | ((uintptr_t)m)) & 7u) == 0) {
        *reinterpret_cast<uint2*>(m + out) = *reinterpret_cast<const uint2*>(r + off);
    } else {  // MK_FIELD_RAW
        for (uint32_t k = 0; k < len; ++k) m[out + k] = r[off + k];
    }
}

template __global__ void k_struct_fields<true>(const uint8_t*, uint64_t, StructSpec, uint8_t*);
template __global__ void k_struct_fields<false>(const uint8_t*, uint64_t, StructSpec, uint8_t*);

// Fused struct roots: one thread per record hashes every bytes field
// (Keccak(le32(len) || bytes), one block), assembles the struct message in
// LDS (dword-major: dword q of thread t at msg[q * 256 + t], conflict-free)
// and absorbs it -- no message round trip through HBM and one launch instead
// of two.  The next bytes field's loads are issued before the current
// field's permutation, so their latency hides behind it.  Host-checked
// layout: every bytes field dword-granular and at most 64 B, every output
// offset and raw length a multiple of 4, records 4-byte aligned (16-B
// aligned records and field offsets use 16-B loads).
// Dynamic LDS: kStructThreads * msg_len bytes.
namespace {
__device__ __forceinline__ void load_field16(const uint8_t* __restrict__ p, uint32_t len, uint32_t vec16,
                                             uint32_t (&a)[16]) {
    if (vec16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = (4u * k < len / 4) ? *reinterpret_cast<const uint4*>(p + 16 * k) : make_uint4(0, 0, 0, 0);
            a[4 * k] = v.x;
            a[4 * k + 1] = v.y;
            a[4 * k + 2] = v.z;
            a[4 * k + 3] = v.w;
        }
    } else {
        const uint32_t* A32 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = (uint32_t)k < len / 4 ? A32[k] : 0u;
    }
}
}  // namespace

__global__ __launch_bounds__(kStructThreads) void k_struct_fused(const uint8_t* __restrict__ rec, uint64_t n,
                                                                 StructSpec sp, uint32_t vec16,
                                                                 uint4* __restrict__ roots) {
    extern __shared__ uint32_t msg[];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kStructThreads + tid;
    const bool live = i < n;
    const uint8_t* r = rec + (live ? i : 0) * sp.rec_len;
    // first bytes field: loads in flight while the raw scalars are copied
    uint32_t f = 0;
    while (f < sp.nfields && sp.kind[f] != 1) ++f;
    uint32_t nxt[16];
    if (f < sp.nfields) load_field16(r + sp.off[f], sp.len[f], vec16, nxt);
#pragma unroll 1
    for (uint32_t g = 0; g < sp.nfields; ++g) {  // MK_FIELD_RAW, len 4 or 8
        if (sp.kind[g] == 1) continue;
        const uint32_t* A32 = reinterpret_cast<const uint32_t*>(r + sp.off[g]);
        const uint32_t q0 = sp.out_off[g] / 4;
        msg[q0 * kStructThreads + tid] = A32[0];
        if (sp.len[g] == 8) msg[(q0 + 1) * kStructThreads + tid] = A32[1];
    }
#pragma unroll 1
    while (f < sp.nfields) {  // MK_FIELD_BYTES: Keccak(le32(len) || bytes), one block
        const uint32_t len = sp.len[f], q0 = sp.out_off[f] / 4;
        uint32_t a[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = nxt[k];
        ++f;
        while (f < sp.nfields && sp.kind[f] != 1) ++f;
        if (f < sp.nfields) load_field16(r + sp.off[f], sp.len[f], vec16, nxt);
        const uint32_t nd = len / 4 + 1;  // message dwords (<= 17)
        State s;
        zero(s);
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            uint32_t v = q == 0 ? len : ((uint32_t)q < nd ? a[q - 1] : 0u);
            if ((uint32_t)q == nd) v ^= 1u;  // domain pad byte
            if (q & 1)
                s.hi[q / 2] ^= v;
            else
                s.lo[q / 2] ^= v;
        }
        s.hi[16] ^= 0x80000000u;
        keccak_f_digest(s);
        uint4 d0, d1;
        digest(s, d0, d1);
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int w = 0; w < 8; ++w) msg[(q0 + w) * kStructThreads + tid] = dw[w];
    }
    // struct hash over the msg_len-byte message (msg_len % 4 == 0)
    const uint32_t mw = sp.msg_len / 4, nb = sp.msg_len / 136 + 1;
    State s;
    zero(s);
#pragma unroll 1
    for (uint32_t b = 0; b < nb; ++b) {
#pragma unroll
        for (int w = 0; w < 34; ++w) {
            const uint32_t q = 34 * b + w;
            uint32_t v = q < mw ? msg[q * kStructThreads + tid] : 0u;
            if (q == mw) v ^= 1u;
            if (b == nb - 1 && w == 33) v ^= 0x80000000u;
            if (w & 1)
                s.hi[w / 2] ^= v;
            else
                s.lo[w / 2] ^= v;
        }
        if (b + 1 < nb)  // nb is uniform (one struct layout)
            keccak_f(s);
        else
            keccak_f_digest(s);
    }
    if (live) {
        uint4 d0, d1;
        digest(s, d0, d1);
        roots[2 * i] = d0;
        roots[2 * i + 1] = d1;
    }
}

// Nested structs and variable-length byte fields (hash.go:141-178): one
// record per thread, one launch.  The host flattens the layout into a program
// (struct_spec.cpp): the fields in declaration order, a struct's close right
// after its last descendant.  A struct's message is staged in the thread's
// LDS column (dword-major as in k_struct_fused: column dword q of thread t at
// col[q * NT + t], conflict-free) right behind its parent's; its close hashes
// the region and stores the 32-B digest into the parent's message, after which
// the next sibling struct reuses the region.  The column is therefore as long
// as the largest sum of message lengths along one nesting path (ns.peak).
//   MK_FIELD_BYTES:    one block (bytes_block_digest), else sponge_rec4
//   MK_FIELD_VARBYTES: sponge_rec4 straight from the record over the stored
//                      length clamped to the slot (per-lane data)
//   MK_FIELD_RAW:      copied
// Every op is uniform across the workgroup, so the only divergence is that
// block loop of sponge_rec4.  No barrier: a thread only touches its own column.
// Dynamic LDS: NT * ns.peak bytes.
namespace {
// nbytes (1..4) low bytes of v to column bytes [b, b + nbytes)
template <uint32_t NT>
__device__ __forceinline__ void col_put(uint32_t* col, uint32_t b, uint32_t v, uint32_t nbytes) {
    const uint32_t q = b / 4, sh = 8 * (b % 4);
    if (sh == 0 && nbytes == 4) {
        col[q * NT] = v;
        return;
    }
    const uint32_t mask = nbytes == 4 ? 0xFFFFFFFFu : (1u << (8 * nbytes)) - 1u;
    v &= mask;
    col[q * NT] = (col[q * NT] & ~(mask << sh)) | (v << sh);
    if (sh + 8 * nbytes > 32) {
        const uint32_t r = 32 - sh;  // bits that went into dword q
        col[(q + 1) * NT] = (col[(q + 1) * NT] & ~(mask >> r)) | (v >> r);
    }
}

// a 32-B digest to column bytes [b, b + 32): whole dwords when b % 4 == 0,
// else the eight dwords shifted across nine (the first and the last merged
// into what the column holds)
template <uint32_t NT>
__device__ __forceinline__ void col_put_digest(uint32_t* col, uint32_t b, const uint32_t (&dw)[8]) {
    const uint32_t q = b / 4, sh = 8 * (b % 4);
    if (sh == 0) {
#pragma unroll
        for (int w = 0; w < 8; ++w) col[(q + w) * NT] = dw[w];
        return;
    }
    const uint32_t r = 32 - sh, lo = (1u << sh) - 1u;  // lo: the bytes of dword q below the digest
    col[q * NT] = (col[q * NT] & lo) | (dw[0] << sh);
#pragma unroll
    for (int w = 1; w < 8; ++w) col[(q + w) * NT] = (dw[w - 1] >> r) | (dw[w] << sh);
    col[(q + 8) * NT] = (col[(q + 8) * NT] & ~lo) | (dw[7] >> r);
}

// Keccak of column bytes [b, b + mlen), b % 4 == 0
template <uint32_t NT>
__device__ __forceinline__ void col_digest(const uint32_t* col, uint32_t b, uint32_t mlen, uint4& d0,
                                           uint4& d1) {
    const uint32_t q0 = b / 4, mw = mlen / 4, rem = mlen % 4, nb = mlen / 136 + 1;
    State s;
    zero(s);
#pragma unroll 1
    for (uint32_t blk = 0; blk < nb; ++blk) {
#pragma unroll
        for (int w = 0; w < 34; ++w) {
            const uint32_t q = 34 * blk + w;
            uint32_t v = q < mw ? col[(q0 + q) * NT] : 0u;
            if (q == mw) {  // the last, partial dword and the domain pad byte
                if (rem) v = col[(q0 + q) * NT] & ((1u << (8 * rem)) - 1u);
                v ^= 1u << (8 * rem);
            }
            if (blk == nb - 1 && w == 33) v ^= 0x80000000u;
            if (w & 1)
                s.hi[w / 2] ^= v;
            else
                s.lo[w / 2] ^= v;
        }
        if (blk + 1 < nb)  // nb is uniform (one layout)
            keccak_f(s);
        else
            keccak_f_digest(s);
    }
    digest(s, d0, d1);
}
}  // namespace

// Keccak(le32(L) || A[0, L)) absorbed straight from the record, as
// sponge_prefix4 does, for a length that differs between lanes: whole dwords
// while they lie inside [0, L), the last partial dword from byte loads (no
// read past A + L).  The block loop diverges: it runs to the wave's largest
// block count while the lanes that are done sit masked off.
__device__ __forceinline__ void sponge_rec4(const uint8_t* __restrict__ A, uint32_t L, uint4& d0, uint4& d1) {
    const uint32_t* A32 = reinterpret_cast<const uint32_t*>(A);
    const uint32_t len = L + 4, nb = len / 136 + 1;
    uint32_t tail = 0;  // message dword len / 4: the L % 4 last bytes
    for (uint32_t k = 0; k < (L & 3u); ++k) tail |= (uint32_t)A[(L & ~3u) + k] << (8 * k);
    tail |= 1u << (8 * (L & 3u));  // domain pad byte
    const uint32_t mw = len / 4;
    State s;
    zero(s);
#pragma unroll 1
    for (uint32_t b = 0; b < nb; ++b) {
#pragma unroll
        for (int w = 0; w < 34; ++w) {
            const uint32_t q = 34 * b + w;  // message dword
            uint32_t v = 0;
            if (q == 0)
                v = L;
            else if (q < mw)
                v = A32[q - 1];
            else if (q == mw)
                v = tail;
            if (b == nb - 1 && w == 33) v ^= 0x80000000u;
            if (w & 1)
                s.hi[w / 2] ^= v;
            else
                s.lo[w / 2] ^= v;
        }
        keccak_f(s);
    }
    digest(s, d0, d1);
}

template <uint32_t NT>
__global__ __launch_bounds__(NT) void k_struct_nested(const uint8_t* __restrict__ rec, uint64_t n, NestedSpec ns,
                                                      uint4* __restrict__ roots) {
    extern __shared__ uint32_t colbase[];
    const uint32_t tid = threadIdx.x;
    uint32_t* col = colbase + tid;
    const uint64_t i = (uint64_t)blockIdx.x * NT + tid;
    const bool live = i < n;
    const uint8_t* r = rec + (live ? i : 0) * ns.rec_len;  // n >= 1: a spare lane re-hashes record 0
#pragma unroll 1
    for (uint32_t k = 0; k < ns.nops; ++k) {
        const uint32_t kind = ns.op[k].kind, src = ns.op[k].src, len = ns.op[k].len, dst = ns.op[k].dst;
        if (kind == 2) {  // MK_FIELD_RAW, len 1, 2, 4 or 8
            if (((src | dst | len) & 3u) == 0) {
                const uint32_t* A32 = reinterpret_cast<const uint32_t*>(r + src);
                col[(dst / 4) * NT] = A32[0];
                if (len == 8) col[(dst / 4 + 1) * NT] = A32[1];
            } else {
                for (uint32_t j = 0; j < len; ++j) col_put<NT>(col, dst + j, r[src + j], 1);
            }
            continue;
        }
        uint4 d0, d1;
        if (kind == 1 && len % 4 == 0 && len + 4 < 136) {  // MK_FIELD_BYTES in one block
            bytes_block_digest(r + src, len, d0, d1);
        } else if (kind == 1) {  // MK_FIELD_BYTES of any other length
            sponge_rec4(r + src, len, d0, d1);
        } else if (kind == 3) {  // MK_FIELD_VARBYTES: le32(L) at src, then L <= len bytes
            // (its own call: with the two kinds folded into one call -- pointer and length chosen by
            // kind -- fixed bytes fields after the first digest of a record came out wrong on the device)
            const uint32_t L = min(*reinterpret_cast<const uint32_t*>(r + src), len);
            sponge_rec4(r + src + 4, L, d0, d1);
        } else {  // kOpClose
            col_digest<NT>(col, src, len, d0, d1);
            if (k + 1 == ns.nops) {  // the top-level struct: the record's root
                if (live) {
                    roots[2 * i] = d0;
                    roots[2 * i + 1] = d1;
                }
                break;
            }
        }
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        col_put_digest<NT>(col, dst, dw);
    }
}
template __global__ void k_struct_nested<256>(const uint8_t*, uint64_t, NestedSpec, uint4*);
template __global__ void k_struct_nested<128>(const uint8_t*, uint64_t, NestedSpec, uint4*);

// Struct roots for the "bytes fields first, then 8-byte scalars" layout
// (pb.Validator: 3 bytes fields + 6 uint64) with the message
// layout known at compile time: the NB field digests go to this thread's
// LDS column (24 KB per workgroup for NB = 3, against 36 KB for the whole
// message in k_struct_fused), the NRAW scalars are re-read from the record
// at absorb time, and the absorb loop is unrolled over compile-time message
// dwords.  No barrier: a thread only touches its own LDS column.
#define MK_STRUCT_REG_WAVES 6
template <int NB, int NRAW>
__global__ __launch_bounds__(kStructThreads, MK_STRUCT_REG_WAVES) void k_struct_reg(const uint8_t* __restrict__ rec,
                                                                                  uint64_t n, StructSpec sp,
                                                                                  uint32_t vec16,
                                                                                  uint4* __restrict__ roots) {
    __shared__ uint32_t dg[NB * 8 * kStructThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kStructThreads + tid;
    if (i >= n) return;
    const uint8_t* r = rec + i * sp.rec_len;
    uint32_t nxt[16];
    load_field16(r + sp.off[0], sp.len[0], vec16, nxt);
#pragma unroll 1
    for (uint32_t f = 0; f < (uint32_t)NB; ++f) {  // Keccak(le32(len) || bytes), one block
        const uint32_t len = sp.len[f];
        uint32_t a[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = nxt[k];
        if (f + 1 < (uint32_t)NB) load_field16(r + sp.off[f + 1], sp.len[f + 1], vec16, nxt);
        const uint32_t nd = len / 4 + 1;
        State s;
        zero(s);
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            uint32_t v = q == 0 ? len : ((uint32_t)q < nd ? a[q - 1] : 0u);
            if ((uint32_t)q == nd) v ^= 1u;
            if (q & 1)
                s.hi[q / 2] ^= v;
            else
                s.lo[q / 2] ^= v;
        }
        s.hi[16] ^= 0x80000000u;
        keccak_f_digest(s);
        uint4 d0, d1;
        digest(s, d0, d1);
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int w = 0; w < 8; ++w) dg[(8 * f + w) * kStructThreads + tid] = dw[w];
    }
    uint32_t raw[2 * NRAW > 0 ? 2 * NRAW : 1];
#pragma unroll
    for (int k = 0; k < NRAW; ++k) {
        const uint32_t* A32 = reinterpret_cast<const uint32_t*>(r + sp.off[NB + k]);
        raw[2 * k] = A32[0];
        raw[2 * k + 1] = A32[1];
    }
    constexpr int MW = 8 * NB + 2 * NRAW;  // message dwords
    constexpr int NBLK = 4 * MW / 136 + 1;
    State s;
    zero(s);
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
#pragma unroll
        for (int w = 0; w < 34; ++w) {
            const int q = 34 * b + w;
            uint32_t v = q < 8 * NB ? dg[q * kStructThreads + tid] : (q < MW ? raw[q - 8 * NB] : 0u);
            if (q == MW) v ^= 1u;
            if (b == NBLK - 1 && w == 33) v ^= 0x80000000u;
            if (w & 1)
                s.hi[w / 2] ^= v;
            else
                s.lo[w / 2] ^= v;
        }
        if (b + 1 < NBLK)
            keccak_f(s);
        else
            keccak_f_digest(s);
    }
    uint4 d0, d1;
    digest(s, d0, d1);
    roots[2 * i] = d0;
    roots[2 * i + 1] = d1;
}
template __global__ void k_struct_reg<3, 6>(const uint8_t*, uint64_t, StructSpec, uint32_t, uint4*);

// Phase-locked struct roots for the validator layout of
// SURVEY §8d (ValidatorRecord: Pubkey 48 B @0, WithdrawalCredentialsHash32
// 32 B @48, RandaoCommitmentHash32 32 B @80, six uint64 @112..152; 160-B
// records, 16-B aligned; the host checks the StructSpec against
// kValOff/kValLen) for n = 1024 * ngroups records, the rest by k_struct_reg.
// 1024-thread workgroups, one per CU, persistent; lane m of wave w hashes
// record g * 1024 + 64 w + m with 3 + 2 phase-locked permutations
// (hash.go:141-159 over the field hashes of :100-107).  The wave's 64
// records (10 KB, contiguous) are copied into its LDS by coalesced DMA (64 x
// 16 B per instruction, consecutive lanes on consecutive units; 160 KB for
// the workgroup), each field digest overwrites that field's own bytes once
// they are absorbed, and the struct message is read back from the record's
// slot; the next group's copy goes out once it is (before the two
// struct-message permutations).
// Level-1 window w of merkleHash over `total` bytes of items whose length
// divides 128 (chunks of 128 B, windows of 256 B) at a 16-B aligned `base`
// (total % 8 == 0): a full window streams its 256 B; the ragged last one
// hashes its r bytes, plus 0^128 when they fill one chunk only (hash.go:225-228).
__device__ __forceinline__ void window256_or_ragged(const uint8_t* __restrict__ base, uint64_t total, uint64_t w,
                                                    uint4& d0, uint4& d1) {
    if (256 * w + 256 <= total) {
        hash_window256(reinterpret_cast<const uint4*>(base) + 16 * w, d0, d1);
        return;
    }
    const uint32_t r = (uint32_t)(total - 256 * w);                // 8..248 bytes
    const uint32_t nwd = r / 8, len = r + (r <= 128 ? 128u : 0u);  // 136..256 B: two blocks
    const uint2* p = reinterpret_cast<const uint2*>(base + 256 * w);
    State s;
    zero(s);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int k = 0; k < 17; ++k) {
            const uint32_t q = 17 * b + k;
            uint2 v = q < nwd ? p[q] : make_uint2(0, 0);
            if (q == len / 8) v.x ^= 1u;  // domain pad (len % 8 == 0)
            s.lo[k] ^= v.x;
            s.hi[k] ^= v.y;
        }
        if (b == 0) {
            keccak_f(s);
        } else {
            s.hi[16] ^= 0x80000000u;
            keccak_f_digest(s);
        }
    }
    digest(s, d0, d1);
}

__device__ constexpr uint32_t kValOff[9] = {0, 48, 80, 112, 120, 128, 136, 144, 152};
__device__ constexpr uint32_t kValLen[9] = {48, 32, 32, 8, 8, 8, 8, 8, 8};
//
// gpw > 0 (the list root, mk_dev_ssz_struct_list_root): workgroup b takes the
// CONTIGUOUS groups [gpw b, gpw b + gpw) instead of striding over the grid,
// and after its last group hashes the level-1 windows of the registry's
// merkleHash (hash.go:194-239 over the 32-B roots: 8 roots = 2 chunks per
// window) from the roots it has just written -- one window per lane on waves
// 0..(gpw*2 - 1), free-running (the other waves have left), into `wins`.  That
// replaces the merkleHash leaf pass, a latency-bound pass over the whole
// roots array.
//
// PREV (gpw == 4, a stream of states, registry.StatePipeline): the launch
// also builds levels 2..10 of the PREVIOUS state's registry tree from that
// state's level-1 windows (its own launch wrote them): workgroup b < nfull
// takes the subtree over windows [512 b, 512 b + 512) -- 256 + 128 + ... + 1
// node permutations -- and writes its level-10 node, so what is left of that
// tree is a 245-node top.  Each wave does ONE of them as an extra lock-step
// permutation (level 2 on waves 0-3, 3 on 4-5, then levels 4..10 on waves
// 6..12, one node per lane), so every wave runs 21 permutations and the
// same barriers; waves 13-15 take levels 2, 3, 4 of the previous state's
// second list (the balances: 128 windows per workgroup, 64 + 32 + 16 node
// permutations), leaving 16 nodes per workgroup.  Level k sits before the field
// permutation at position 2 (k - 2) of the 16 (4 groups x f0, f1, f2, s1);
// level 10 after the group loop: the writer waits for its store at round 12
// of the field permutation that follows its slot, and counted in barriers
// (waves line up by barrier count, not by position) every reader loads at
// least half a permutation after that wait (through L2: this CU never read
// those lines, and its L1 was invalidated at dispatch).
template <bool PREV>
__global__ __launch_bounds__(kLockThreads, 1) void k_struct_lock(const uint8_t* __restrict__ rec, uint64_t n,
                                                                 uint4* __restrict__ roots, uint32_t gpw,
                                                                 uint4* __restrict__ wins,
                                                                 const uint8_t* __restrict__ vals, uint64_t vbytes,
                                                                 uint4* __restrict__ vwins, StructPrev prev) {
    constexpr uint32_t kRecLen = 160, kRw = kRecLen / 4, kNinstr = kRecLen / 16;
    __shared__ uint32_t buf[kLockThreads / 64][64 * kRw];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* Bw = buf[wave];
    const uint32_t wv = __builtin_amdgcn_readfirstlane(wave);
    // this wave's slot: the registry's level my_k (waves 0-12: 2 on 0-3, 3 on
    // 4-5, 4..10 on 6..12) or the second list's (waves 13-15: levels 2, 3,
    // 4), at position my_pos (2 (k - 2); the registry's level 10 at 16, after
    // the group loop)
    const bool my_val = wv >= 13;
    const uint32_t my_k = my_val ? wv - 11u : wv < 4 ? 2u : wv < 6 ? 3u : wv - 2u;
    const uint32_t my_pos = my_k == 10 ? 16u : 2u * (my_k - 2u);
    auto prev_slot = [&] {
        const uint32_t k = my_k;
        const uint32_t sub = my_val ? 128u : 512u;                           // level-1 nodes per subtree
        const uint32_t w0 = my_val ? wv : k == 2 ? 0u : k == 3 ? 4u : k + 2u;  // first wave of level k
        const uint32_t per = sub >> (k - 1);                                 // level-k nodes per subtree
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));  // computed here, not hoisted and kept live across the loop
        const uint32_t j = 64u * (wv - w0) + ln;
        const bool act = prev.live && blockIdx.x < (my_val ? prev.nvfull : prev.nfull) && j < per;
        const uint4* src = k == 2 ? (my_val ? prev.v1 : prev.l1) + 2 * (sub * blockIdx.x)
                                  : (my_val ? prev.vlv[k - 3] : prev.lv[k - 3]) + 4 * (per * blockIdx.x);
        asm volatile("" ::: "memory");
        State s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = act ? src[4 * j + q] : make_uint4(0, 0, 0, 0);
            s.lo[2 * q] = v.x;
            s.hi[2 * q] = v.y;
            s.lo[2 * q + 1] = v.z;
            s.hi[2 * q + 1] = v.w;
        }
#pragma unroll
        for (int w = 8; w < 25; ++w) s.lo[w] = s.hi[w] = 0;
        s.lo[8] = 1u;  // byte 64
        s.hi[16] = 0x80000000u;
        keccak_f_digest_lock(s);
        if (act) {
            uint4 d0, d1;
            digest(s, d0, d1);
            uint4* dst = (my_val ? prev.vlv[k - 2] : prev.lv[k - 2]) + 2 * (per * blockIdx.x + j);
            dst[0] = d0;
            dst[1] = d1;
        }
        asm volatile("" ::: "memory");
    };
    // the last group may be partial: its lanes past n copy the last record
    // (every wave still runs the same permutations and barriers) and store nothing
    const uint64_t ngroups = (n + kLockThreads - 1) / kLockThreads;
    const uint64_t last_unit = n * (kRecLen / 16) - 1;
    // instructions [i0, i1) of the kNinstr (issued in parts).  Record m of
    // the wave sits in 16-B slots [10 m, 10 m + 10) rotated by one unit when
    // bits 2 and 3 of m differ (unit u in slot 10 m + (u + rot) mod 10).  On
    // gfx950 a ds_read_b128 is conflict-free when the slots of each 16
    // consecutive lanes differ mod 16, a ds_write_b128 when those of each 8
    // differ mod 8 (tools/lds_bank_probe.hip, profiles/r06/lds_bank_probe.txt);
    // the plain 160-B stride fails both (lanes l, l + 8 and l, l + 4 collide:
    // 1.63 M SQ_LDS_BANK_CONFLICT per launch, profiles/r05/pmc/), this
    // rotation passes both.  The copy stays one contiguous 1-KB LDS write per
    // instruction, each lane fetching the unit its slot holds
    auto dma = [&](uint64_t g, uint32_t i0 = 0, uint32_t i1 = kNinstr) {
        const uint64_t u0 = (g * kLockThreads + 64 * wave) * (kRecLen / 16);
        const uint4* src = reinterpret_cast<const uint4*>(rec);
#pragma unroll
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t sl = 64 * i + lane, m = sl / 10u, v = sl - 10u * m;
            const uint32_t rot = ((m >> 2) ^ (m >> 3)) & 1u;
            const uint64_t u = u0 + 10u * m + (v >= rot ? v - rot : v + 10u - rot);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + (u < last_unit ? u : last_unit)),
                                             (__attribute__((address_space(3))) void*)(Bw + 256 * i), 16, 0,
                                             kSideAux);
        }
    };
    const uint64_t g_begin = gpw ? (uint64_t)blockIdx.x * gpw : blockIdx.x;
    const uint64_t g_end = gpw ? (g_begin + gpw < ngroups ? g_begin + gpw : ngroups) : ngroups;
    const uint64_t g_step = gpw ? 1 : gridDim.x;
    uint64_t g = g_begin;
    if (g < g_end) dma(g);
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;  // the previous group's root, stored after the next wait
    uint64_t qi = 0;
    bool pend = false;
    // the previous state's slots run in workgroups of exactly gpw == 4 groups
    // (uniform over the workgroup: all its waves run the same permutations)
    const bool slots = PREV && gpw == 4 && g_end - g_begin == 4;
    // this lane's record: units 0..8 at R (rotated), unit 9 at R9
    const uint32_t rot = ((lane >> 2) ^ (lane >> 3)) & 1u;
    uint32_t* const R = Bw + lane * kRw + 4u * rot;
    const uint32_t* const R9 = Bw + lane * kRw + (rot ? 0u : 36u);
#pragma unroll 1
    for (; g < g_end; g += g_step) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the wave's records have landed
        if (pend && qi < n) {
            roots[2 * qi] = q0;
            roots[2 * qi + 1] = q1;
        }
        const uint32_t pos0 = 4u * (uint32_t)(g - g_begin);  // slot position of field 0 of this group
#pragma unroll
        for (int f = 0; f < 3; ++f) {  // Keccak(le32(len) || bytes), one block
            // this wave's slot of the previous state's tree (f = 0, 2 only: positions 2 (k - 2))
            const bool slot_here = slots && (f == 0 || f == 2) && my_pos == pos0 + f;
            if (slot_here) prev_slot();
            const uint32_t len = kValLen[f], off = kValOff[f] / 4, nd = len / 4 + 1;
            State s;
#pragma unroll
            for (uint32_t q = 0; q < 18; ++q) {
                uint32_t v = q == 0 ? len : (q < nd ? R[off + q - 1] : 0u);
                if (q == nd) v ^= 1u;
                if (q & 1)
                    s.hi[q / 2] = v;
                else
                    s.lo[q / 2] = v;
            }
#pragma unroll
            for (int k = 9; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
            s.hi[16] = 0x80000000u;
            if constexpr (PREV) {
                // the slot's node store completes mid-permutation, before the
                // next level's reader (two positions on) can pass a barrier
                keccak_f_digest_lock<12>(s, [&] {
                    if (slot_here) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                });
            } else {
                keccak_f_digest_lock(s);
            }
            // the digest replaces the field's own bytes (absorbed above)
            R[off + 0] = s.lo[0]; R[off + 1] = s.hi[0]; R[off + 2] = s.lo[1]; R[off + 3] = s.hi[1];
            R[off + 4] = s.lo[2]; R[off + 5] = s.hi[2]; R[off + 6] = s.lo[3]; R[off + 7] = s.hi[3];
        }
        // struct message (hash.go:141-159): the digests of fields 0..2, then
        // the six uint64 raw: 36 dwords = block 1 (34) + 2 dwords of block 2
        State s;
#pragma unroll
        for (int q = 0; q < 34; ++q) {
            // the six uint64 are dwords 28..39: units 7, 8 and (dwords 36..39) 9
            const uint32_t v = q < 24 ? R[kValOff[q / 8] / 4 + q % 8]
                                      : (q < 32 ? R[kValOff[3] / 4 + (q - 24)] : R9[q - 32]);
            if (q & 1)
                s.hi[q / 2] = v;
            else
                s.lo[q / 2] = v;
        }
#pragma unroll
        for (int k = 17; k < 25; ++k) s.lo[k] = s.hi[k] = 0;
        const uint32_t t0 = R9[2], t1 = R9[3];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // record read: the next group's copy may land
        // the next group's copy in three parts over the first struct
        // permutation, not one burst of 16 waves' DMA (the
        // 10^6 list root 0.600 -> 0.593 ms, profiles/r05/side_dma_split/)
        const bool more = g + g_step < g_end;
        keccak_f_lock_mid3<2, 8, 14>(s, [&] { if (more) dma(g + g_step, 0, 4); },
                                     [&] { if (more) dma(g + g_step, 4, 7); },
                                     [&] { if (more) dma(g + g_step, 7, 10); });
        s.lo[0] ^= t0;
        s.hi[0] ^= t1;
        s.lo[1] ^= 1u;  // domain pad at message byte 144 = block 2 byte 8
        s.hi[16] ^= 0x80000000u;
        keccak_f_digest_lock(s);
        digest(s, q0, q1);
        qi = g * kLockThreads + threadIdx.x;
        pend = true;
    }
    // the registry's level 10 (wave 12) after the loop.  Waves line up by
    // barrier count: the level-9 writer (wave 11) stores at the end of its
    // slot permutation (its 18th of 21) and waits for the store at round 12 of
    // the next (group 3's f2); wave 12 runs f2 as its 18th, the two struct
    // permutations as its 19th-20th and loads level 9 at the start of its
    // 21st, 1.5 permutations after that wait (before the loop's end it would
    // load at the writer's store).  Nothing in this launch reads it.
    if (slots && my_pos == 16u) prev_slot();
    if (pend && qi < n) {
        roots[2 * qi] = q0;
        roots[2 * qi + 1] = q1;
    }
    if (!wins || g_begin >= g_end) return;
    // the workgroup's roots are in L2 (written above; this CU never read those
    // lines, and its L1 was invalidated at dispatch): every wave's stores
    // complete, then one window per lane -- the registry's windows over the
    // roots just written, then this workgroup's share of the optional second
    // list's windows (`vals`, vbytes bytes of items dividing 128; the State's
    // balances) on the lanes left over
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint64_t r0 = g_begin * kLockThreads, r1 = g_end * kLockThreads < n ? g_end * kLockThreads : n;
    const uint64_t w0 = r0 / 8, nw = (r1 - r0 + 7) / 8;
    // PREV: 128 windows per workgroup (the subtrees the next launch's slots
    // take; 128 >= ceil(vw_total / grid) for the State's 8-B balances)
    const uint64_t vw_total = (vbytes + 255) / 256;
    const uint64_t vpw = PREV && gpw == 4 ? 128u : (vw_total + gridDim.x - 1) / gridDim.x;
    const uint64_t v0 = (uint64_t)blockIdx.x * vpw;
    const uint64_t nv = vals && v0 < vw_total ? (vw_total - v0 < vpw ? vw_total - v0 : vpw) : 0;
#pragma unroll 1
    for (uint64_t t = threadIdx.x; t < nw + nv; t += kLockThreads) {
        const bool reg = t < nw;
        const uint64_t w = reg ? w0 + t : v0 + (t - nw);
        const uint8_t* base = reg ? reinterpret_cast<const uint8_t*>(roots) : vals;
        const uint64_t total = reg ? 32 * n : vbytes;
        uint4 d0, d1;
        window256_or_ragged(base, total, w, d0, d1);
        uint4* o = reg ? wins : vwins;
        o[2 * w] = d0;
        o[2 * w + 1] = d1;
    }
}

template __global__ void k_struct_lock<false>(const uint8_t*, uint64_t, uint4*, uint32_t, uint4*, const uint8_t*,
                                              uint64_t, uint4*, StructPrev);
template __global__ void k_struct_lock<true>(const uint8_t*, uint64_t, uint4*, uint32_t, uint4*, const uint8_t*,
                                             uint64_t, uint4*, StructPrev);
template __global__ void k_struct_reg<2, 0>(const uint8_t*, uint64_t, StructSpec, uint32_t, uint4*);

// The same layouts for SMALL registries (the 16,384-validator C1 shape),
// where every wave runs alone on its SIMD and the cost is the chain of
// permutation latencies, not throughput: four lanes per record.  Lanes
// 0..NB-1 of a record hash its NB bytes fields side by side (one
// permutation of latency instead of NB), the digests meet in LDS, and lanes
// 0 and 1 hash the struct message (2 blocks) as a lo/hi lane pair (round 6:
// C1's struct roots 29.6 -> see DESIGN §4.5): 3 serial permutations per
// record instead of 5, the last two at lane-pair latency.  The host takes this form while 4 lanes per record still fit
// the chip once (n <= kStructSplitMaxN).
// The body, for the first 256 threads of the calling workgroup (every
// thread of it must call: the digests meet in LDS behind a barrier):
// records [64 blk, 64 blk + 64), roots to roots[].
template <int NB, int NRAW>
__device__ __forceinline__ void struct_split_body(const uint8_t* __restrict__ rec, uint64_t n, const StructSpec& sp,
                                                  uint32_t vec16, uint4* __restrict__ roots, uint64_t blk,
                                                  uint32_t (&dg)[NB * 8][64]) {
    static_assert(NB <= 4, "one lane per bytes field");
    constexpr uint32_t kV = 256 / 4;  // records per workgroup
    const uint32_t tid = threadIdx.x, v = (tid >> 2) & (kV - 1), role = tid & 3u;
    const uint64_t i = blk * kV + v;
    const bool live = tid < 256u && i < n;
    const uint8_t* r = rec + (live ? i : 0) * sp.rec_len;
    if (live && role < (uint32_t)NB) {  // Keccak(le32(len) || bytes), one block
        const uint32_t off = role == 0 ? sp.off[0] : role == 1 ? sp.off[1 % NB] : sp.off[2 % NB];
        const uint32_t len = role == 0 ? sp.len[0] : role == 1 ? sp.len[1 % NB] : sp.len[2 % NB];
        uint32_t a[16];
        load_field16(r + off, len, vec16, a);
        const uint32_t nd = len / 4 + 1;
        State s;
        zero(s);
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            uint32_t x = q == 0 ? len : ((uint32_t)q < nd ? a[q - 1] : 0u);
            if ((uint32_t)q == nd) x ^= 1u;
            if (q & 1)
                s.hi[q / 2] ^= x;
            else
                s.lo[q / 2] ^= x;
        }
        s.hi[16] ^= 0x80000000u;
        keccak_f_digest(s);
        uint4 d0, d1;
        digest(s, d0, d1);
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int w = 0; w < 8; ++w) dg[8 * role + w][v] = dw[w];
    }
    __syncthreads();
    // the struct message (the digests, then the raw scalars) on lanes 0 and 1
    // of the record as a lo/hi lane pair (mk::pair: lane p holds half p of
    // every Keccak lane, so message dword 2k + p is its word k and no
    // conversion is needed): 2 x ~12.8 k cycles of latency for the two
    // blocks against 2 x ~21 k on one lane
    if (!live || role > 1u) return;
    const uint32_t p = role;
    uint32_t raw[NRAW > 0 ? NRAW : 1];
#pragma unroll
    for (int k = 0; k < NRAW; ++k) raw[k] = reinterpret_cast<const uint32_t*>(r + sp.off[NB + k])[p];
    constexpr int MW = 8 * NB + 2 * NRAW;  // message dwords
    constexpr int NBLK = 4 * MW / 136 + 1;
    pair::Half s;
    pair::zero(s);
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
#pragma unroll
        for (int k = 0; k < 17; ++k) {
            const int q0 = 34 * b + 2 * k;  // this Keccak lane's lo dword (MW and 8 NB are even)
            uint32_t x = q0 < 8 * NB ? dg[q0 + p][v] : (q0 < MW ? raw[(q0 - 8 * NB) / 2] : 0u);
            if (q0 == MW && p == 0u) x ^= 1u;
            if (b == NBLK - 1 && k == 16 && p == 1u) x ^= 0x80000000u;
            s.v[k] ^= x;
        }
        pair::keccak_f(s, p != 0u);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(roots) + 8 * i;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[2 * k + p] = s.v[k];
}

template <int NB, int NRAW>
__global__ __launch_bounds__(256) void k_struct_split(const uint8_t* __restrict__ rec, uint64_t n, StructSpec sp,
                                                      uint32_t vec16, uint4* __restrict__ roots) {
    __shared__ uint32_t dg[NB * 8][64];
    struct_split_body<NB, NRAW>(rec, n, sp, vec16, roots, blockIdx.x, dg);
}
template __global__ void k_struct_split<3, 6>(const uint8_t*, uint64_t, StructSpec, uint32_t, uint4*);
template __global__ void k_struct_split<2, 0>(const uint8_t*, uint64_t, StructSpec, uint32_t, uint4*);
