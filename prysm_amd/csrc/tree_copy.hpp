// The piece map of a resident tree's copy: the live part of a
// tree of n values laid out for cap_src values, moved into the layout of
// cap_dst values, as a list of segments cut into 16-byte pieces.  Segment 0 is
// the values (n * item_len bytes), segment 1 level 0 of a struct / bytes tree
// (32 n bytes, empty for a list tree), segment 1 + d the ceil(nchunks / 2^d)
// nodes of level d = 1 .. D, segment D + 2 the 32-byte root.  A level starts at
// node sum_{1<=i<d} ceil(cap_chunks / 2^i) of its level array
// (include/prysm_merkle.h, the resident list tree), so its source and its
// destination offsets differ when the capacities do; everything else starts
// its buffer.  Levels above D and nodes beyond a level's count belong to no
// segment: they are not read and not written (§5k).  Shared by k_trees_copy
// (kernels_tree.hip), the host side (tree_copy_api.cpp) and the host fuzz
// (tests/c_abi/tree_copy_fuzz.cpp); no HIP in it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MK_COPY_HD __host__ __device__
#else
#define MK_COPY_HD
#endif

namespace mk {

constexpr uint32_t kCopyPiece = 16;
constexpr uint32_t kCopyLevelsMax = 64;                // D <= 64 for any 64-bit chunk count
constexpr uint32_t kCopySegsMax = kCopyLevelsMax + 3;  // values, level 0, the levels, the root
// the buffer a segment lies in: one pointer pair of the tree's descriptor each
enum CopyBuf : uint32_t { kCopyItems = 0, kCopyLevel0 = 1, kCopyLevels = 2, kCopyRoot = 3 };

struct CopyShape {
    uint32_t item_len;  // 1 .. 2^30
    uint32_t level0;    // a 32-B entry per value under the levels (struct roots, element digests)
    uint32_t D;         // stored levels: the smallest d with ceil(nchunks / 2^d) == 1
    uint64_t n;
    uint64_t nchunks;                         // ceil(n / p), p leaves per chunk
    uint64_t cap_src_chunks, cap_dst_chunks;  // the same of the two capacities: where a level starts
};

// one 16-byte piece: its segment and buffer, where it lies in the source and in the destination buffer
struct CopyPiece {
    uint32_t seg, buf;
    uint32_t valid;  // bytes of the piece inside the segment: 16, less for the last piece of the values
    uint64_t src_off, dst_off;
};

// n <= cap_src, n <= cap_dst, item_len in 1 .. 2^30, capacity * max(item_len, 32) < 2^64 (the caller's checks)
MK_COPY_HD inline CopyShape copy_shape(uint64_t n, uint64_t cap_src, uint64_t cap_dst, uint32_t item_len,
                                       bool level0) {
    CopyShape c{};
    c.item_len = item_len;
    c.level0 = level0 ? 1u : 0u;
    c.n = n;
    const uint32_t leaf = level0 ? 32u : item_len;  // a leaf of the tree: the value, or its root / digest
    const uint64_t p = leaf < 128u ? 128u / leaf : 1u;
    c.nchunks = n / p + (n % p != 0);
    c.cap_src_chunks = cap_src / p + (cap_src % p != 0);
    c.cap_dst_chunks = cap_dst / p + (cap_dst % p != 0);
    c.D = c.nchunks > 1 ? 64u - (uint32_t)__builtin_clzll(c.nchunks - 1) : 0u;  // ceil(log2(nchunks))
    return c;
}

// nodes of level d >= 1 of the current list: ceil(nchunks / 2^d)
MK_COPY_HD inline uint64_t copy_level_count(const CopyShape& c, uint32_t d) {
    if (d >= 64) return c.nchunks != 0;
    const uint64_t m = (1ull << d) - 1;
    return (c.nchunks >> d) + ((c.nchunks & m) != 0);
}

// First node of level d (1 <= d <= 65) in a level array laid out for
// cap_chunks chunks: sum over 1 <= i < d of ceil(cap_chunks / 2^i), without the
// loop.  With m = cap_chunks - 1 and k = d - 1, ceil(cap_chunks / 2^i) =
// (m >> i) + 1, and sum_{i>=1} (x >> i) = x - popcount(x) for x = m and, for the
// terms above k, x = m >> k.
MK_COPY_HD inline uint64_t copy_level_off(uint64_t cap_chunks, uint32_t d) {
    if (cap_chunks == 0 || d <= 1) return 0;
    const uint32_t k = d - 1;
    const uint64_t m = cap_chunks - 1, top = k < 64 ? m >> k : 0;
    return k + (m - (uint64_t)__builtin_popcountll(m)) - (top - (uint64_t)__builtin_popcountll(top));
}

MK_COPY_HD inline uint32_t copy_segs(const CopyShape& c) { return c.D + 3; }

MK_COPY_HD inline uint32_t copy_seg_buf(const CopyShape& c, uint32_t seg) {
    return seg == 0 ? kCopyItems : seg == 1 ? kCopyLevel0 : seg == c.D + 2 ? kCopyRoot : kCopyLevels;
}

// bytes of segment seg < copy_segs(c)
MK_COPY_HD inline uint64_t copy_seg_bytes(const CopyShape& c, uint32_t seg) {
    if (seg == 0) return c.n * c.item_len;
    if (seg == 1) return c.level0 ? 32 * c.n : 0;
    if (seg == c.D + 2) return 32;
    return 32 * copy_level_count(c, seg - 1);
}

MK_COPY_HD inline uint64_t copy_seg_pieces(const CopyShape& c, uint32_t seg) {
    const uint64_t b = copy_seg_bytes(c, seg);
    return b / kCopyPiece + (b % kCopyPiece != 0);
}

// where segment seg starts in its source and in its destination buffer (bytes)
MK_COPY_HD inline void copy_seg_offs(const CopyShape& c, uint32_t seg, uint64_t* src_off, uint64_t* dst_off) {
    const bool level = seg >= 2 && seg < c.D + 2;
    *src_off = level ? 32 * copy_level_off(c.cap_src_chunks, seg - 1) : 0;
    *dst_off = level ? 32 * copy_level_off(c.cap_dst_chunks, seg - 1) : 0;
}

// the tree's first piece of segment seg <= copy_segs(c) (the segments in order; seg == copy_segs(c): the
// tree's piece total).  A level's nodes are two pieces each, and the levels' counts add up as a level
// array's offsets do for nchunks chunks.
MK_COPY_HD inline uint64_t copy_seg_first(const CopyShape& c, uint32_t seg) {
    if (seg == 0) return 0;
    const uint64_t items = copy_seg_pieces(c, 0);
    if (seg == 1) return items;
    const uint64_t lv = items + (c.level0 ? 2 * c.n : 0);
    if (seg <= c.D + 2) return lv + 2 * copy_level_off(c.nchunks, seg - 1);
    return lv + 2 * copy_level_off(c.nchunks, c.D + 1) + 2;
}

MK_COPY_HD inline uint64_t copy_pieces(const CopyShape& c) { return copy_seg_first(c, copy_segs(c)); }

// piece q of segment seg, whose segment starts at seg_src / seg_dst of its buffers (copy_seg_offs)
MK_COPY_HD inline CopyPiece copy_piece_in(const CopyShape& c, uint32_t seg, uint64_t q, uint64_t seg_src,
                                          uint64_t seg_dst) {
    CopyPiece p{};
    p.seg = seg;
    p.buf = copy_seg_buf(c, seg);
    const uint64_t at = q * kCopyPiece, rest = copy_seg_bytes(c, seg) - at;
    p.valid = rest < kCopyPiece ? (uint32_t)rest : kCopyPiece;
    p.src_off = seg_src + at;
    p.dst_off = seg_dst + at;
    return p;
}

// piece g < copy_pieces(c) of the tree, the segments in order
MK_COPY_HD inline CopyPiece copy_piece(const CopyShape& c, uint64_t g) {
    uint32_t s = 0;
    while (copy_seg_first(c, s + 1) <= g) ++s;  // an empty segment is stepped over
    uint64_t so, dof;
    copy_seg_offs(c, s, &so, &dof);
    return copy_piece_in(c, s, g - copy_seg_first(c, s), so, dof);
}

}  // namespace mk
