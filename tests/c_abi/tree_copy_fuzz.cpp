// Stand-alone host fuzz of the piece map of a resident tree's copy
// (prysm_amd/csrc/tree_copy.hpp, shared with k_trees_copy and the host side of
// mk_dev_ssz_trees_copy): built with -fsanitize=address,undefined and run as a
// child process by tests/test_tree_copy_fuzz.py.
//
//   tree_copy_fuzz SEED RANDOM_CASES
//
// Every case: a tree shape (item_len 1..300, n 0..5000, cap_src and cap_dst >=
// n drawn independently, with or without a level 0) and a naive model of the
// layout rule of include/prysm_merkle.h -- the chunk count, every level's live
// count by repeated halving, every level's first node in the two level arrays
// by the loop mk_ssz_list_tree_levels_bytes sums with.  The model keeps every
// live extent (the values, level 0, each level's live nodes, the root) in a
// heap buffer of exactly its size, source and destination, so a piece that
// reaches outside one is ASan's to report as well as this program's.  The
// source is filled with a position code; every piece of the header's map is
// replayed; then every live destination byte must have arrived exactly once
// with the code of its own position.  D, the level offsets (also for random
// 64-bit chunk counts, where the header's closed form has no buffers to
// check it) and the piece total are compared with the model's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tree_copy.hpp"

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t g_cases, g_pieces, g_offsets;

struct Case {
    uint64_t n, cap_src, cap_dst;
    uint32_t item_len;
    bool level0;
};

[[noreturn]] static void die(const Case& c, const char* what, uint64_t a = 0, uint64_t b = 0) {
    std::fprintf(stderr, "%s (%llu, %llu): n %llu, cap_src %llu, cap_dst %llu, item_len %u, level0 %d\n", what,
                 (unsigned long long)a, (unsigned long long)b, (unsigned long long)c.n, (unsigned long long)c.cap_src,
                 (unsigned long long)c.cap_dst, c.item_len, (int)c.level0);
    std::exit(1);
}

// ---- the model: the layout rule, naively ----------------------------------------------------------
static uint64_t chunks_of(uint64_t n, uint32_t leaf) {
    const uint64_t p = leaf < 128 ? 128 / leaf : 1;
    return (n + p - 1) / p;
}

// first node of level d >= 1 of a level array for cap_chunks chunks: the levels below it, each ceil(half) of the last
static uint64_t naive_level_off(uint64_t cap_chunks, uint32_t d) {
    uint64_t off = 0, c = cap_chunks;
    for (uint32_t i = 1; i < d; ++i) {
        c = c / 2 + (c & 1);
        off += c;
    }
    return off;
}

// nodes of the whole level array: what mk_ssz_list_tree_levels_bytes / 32 is
static uint64_t naive_levels_nodes(uint64_t cap_chunks) {
    uint64_t sum = 0;
    for (uint64_t c = cap_chunks; c > 1;) {
        c = (c + 1) / 2;
        sum += c;
    }
    return sum;
}

static uint8_t code(uint32_t extent, uint64_t off) {  // a position code: the extent and the byte's place in it
    uint64_t z = (uint64_t)extent * 0x9E3779B97F4A7C15ull + off * 0xBF58476D1CE4E5B9ull;
    return (uint8_t)((z >> 29) ^ (z >> 7) ^ 0x5a);
}

// one live extent: exactly its bytes, source and destination, and how often each destination byte was written
struct ExtentBufs {
    uint64_t bytes = 0, src_at = 0, dst_at = 0;  // where the extent starts in its source / destination buffer
    uint8_t *src = nullptr, *dst = nullptr, *hits = nullptr;
    void make(uint32_t id, uint64_t b, uint64_t s_at, uint64_t d_at) {
        bytes = b, src_at = s_at, dst_at = d_at;
        src = (uint8_t*)std::malloc(b ? b : 1);  // malloc(0) may be null: the extent is then never touched
        dst = (uint8_t*)std::malloc(b ? b : 1);
        hits = (uint8_t*)std::calloc(b ? b : 1, 1);
        if (!src || !dst || !hits) std::abort();
        for (uint64_t i = 0; i < b; ++i) src[i] = code(id, i), dst[i] = (uint8_t)~code(id, i);
    }
    void drop() {
        std::free(src), std::free(dst), std::free(hits);
    }
};

static void check(const Case& k) {
    const uint32_t leaf = k.level0 ? 32 : k.item_len;
    const uint64_t nch = chunks_of(k.n, leaf), caps = chunks_of(k.cap_src, leaf), capd = chunks_of(k.cap_dst, leaf);
    std::vector<uint64_t> count;  // count[d - 1]: live nodes of level d
    for (uint64_t c = nch; c > 1;) {
        c = (c + 1) / 2;
        count.push_back(c);
    }
    const uint32_t D = (uint32_t)count.size();

    const mk::CopyShape sh = mk::copy_shape(k.n, k.cap_src, k.cap_dst, k.item_len, k.level0);
    if (sh.D != D) die(k, "D", sh.D, D);
    if (sh.nchunks != nch || sh.cap_src_chunks != caps || sh.cap_dst_chunks != capd) die(k, "chunk counts");
    if (mk::copy_segs(sh) != D + 3) die(k, "segments");
    for (uint32_t d = 1; d <= D + 1; ++d) {
        if (mk::copy_level_off(caps, d) != naive_level_off(caps, d)) die(k, "source level offset", d);
        if (mk::copy_level_off(capd, d) != naive_level_off(capd, d)) die(k, "destination level offset", d);
        if (d <= D && mk::copy_level_count(sh, d) != count[d - 1]) die(k, "level count", d);
        g_offsets += 2;
    }
    // every stored level ends inside the level array of its capacity
    if (D && naive_level_off(caps, D) + count[D - 1] > naive_levels_nodes(caps)) die(k, "source levels overrun");
    if (D && naive_level_off(capd, D) + count[D - 1] > naive_levels_nodes(capd)) die(k, "destination levels overrun");

    // the live extents, in the header's segment order: values, level 0, level 1 .. D, root
    std::vector<ExtentBufs> ext(D + 3);
    ext[0].make(0, k.n * k.item_len, 0, 0);
    ext[1].make(1, k.level0 ? 32 * k.n : 0, 0, 0);
    for (uint32_t d = 1; d <= D; ++d)
        ext[1 + d].make(1 + d, 32 * count[d - 1], 32 * naive_level_off(caps, d), 32 * naive_level_off(capd, d));
    ext[D + 2].make(D + 2, 32, 0, 0);
    uint64_t want_pieces = 0;
    for (const ExtentBufs& e : ext) want_pieces += (e.bytes + 15) / 16;

    const uint64_t total = mk::copy_pieces(sh);
    if (total != want_pieces) die(k, "piece total", total, want_pieces);
    for (uint64_t g = 0; g < total; ++g) {
        const mk::CopyPiece p = mk::copy_piece(sh, g);
        if (p.seg >= D + 3) die(k, "segment of a piece", g, p.seg);
        ExtentBufs& e = ext[p.seg];
        const uint32_t buf = p.seg == 0 ? mk::kCopyItems : p.seg == 1 ? mk::kCopyLevel0 : p.seg == D + 2 ? mk::kCopyRoot : mk::kCopyLevels;
        if (p.buf != buf) die(k, "buffer of a piece", g, p.buf);
        if (p.valid == 0 || p.valid > 16) die(k, "valid bytes", g, p.valid);
        if (p.valid != 16 && p.seg != 0) die(k, "a short piece outside the values", g, p.seg);
        // inside the live extent, on both sides, at the same place of it
        if (p.src_off < e.src_at || p.src_off - e.src_at + p.valid > e.bytes) die(k, "source outside its live extent", g, p.src_off);
        if (p.dst_off < e.dst_at || p.dst_off - e.dst_at + p.valid > e.bytes) die(k, "destination outside its live extent", g, p.dst_off);
        if (p.src_off - e.src_at != p.dst_off - e.dst_at) die(k, "a piece changes its place in the extent", g);
        if (p.seg != 0 && ((p.src_off | p.dst_off) & 15)) die(k, "a misaligned piece outside the values", g);
        const uint64_t at = p.src_off - e.src_at;
        std::memcpy(e.dst + at, e.src + at, p.valid);  // exact-size buffers: an overrun is ASan's
        for (uint32_t i = 0; i < p.valid; ++i)
            if (++e.hits[at + i] != 1) die(k, "a byte written twice", g, at + i);
        // the kernel's form: the segment's first piece and offsets looked up once, then copy_piece_in
        uint64_t so, dof;
        mk::copy_seg_offs(sh, p.seg, &so, &dof);
        const mk::CopyPiece q = mk::copy_piece_in(sh, p.seg, g - mk::copy_seg_first(sh, p.seg), so, dof);
        if (q.src_off != p.src_off || q.dst_off != p.dst_off || q.valid != p.valid || q.buf != p.buf) die(k, "copy_piece_in", g);
        ++g_pieces;
    }
    for (uint32_t s = 0; s < D + 3; ++s) {
        const ExtentBufs& e = ext[s];
        for (uint64_t i = 0; i < e.bytes; ++i) {
            if (e.hits[i] != 1) die(k, "a live byte never arrived", s, i);
            if (e.dst[i] != code(s, i)) die(k, "a byte arrived at the wrong place", s, i);
        }
    }
    for (ExtentBufs& e : ext) e.drop();
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s SEED RANDOM_CASES\n", argv[0]);
        return 2;
    }
    g_state = std::strtoull(argv[1], nullptr, 0);
    const uint64_t ncases = std::strtoull(argv[2], nullptr, 0);
    // the corners first: every small n at every kind of item length, equal and unequal capacities
    for (uint32_t L : {1u, 5u, 8u, 32u, 33u, 48u, 100u, 127u, 128u, 129u, 200u, 300u})
        for (uint64_t n = 0; n <= 40; ++n)
            for (int l0 = 0; l0 < 2; ++l0) {
                check({n, n, n, L, l0 != 0});
                check({n, n, n + 1, L, l0 != 0});
                check({n, n + 1, 2 * n + 3, L, l0 != 0});
                check({n, 2 * n + 3, n, L, l0 != 0});
            }
    for (uint64_t i = 0; i < ncases; ++i) {
        Case k;
        k.item_len = 1 + (uint32_t)(rnd() % 300);
        k.n = rnd() % 5001;
        if (rnd() % 4 == 0) k.n = rnd() % 70;  // the small trees, where D changes fastest
        k.cap_src = k.n + (rnd() % 3 == 0 ? 0 : rnd() % 6000);
        k.cap_dst = k.n + (rnd() % 3 == 0 ? 0 : rnd() % 6000);
        k.level0 = rnd() % 2;
        check(k);
    }
    // the closed form of a level's first node against the loop, for chunk counts no buffer could hold
    const Case none{0, 0, 0, 1, false};
    for (uint64_t i = 0; i < 20 * ncases + 1000; ++i) {
        const uint64_t c = rnd() >> (rnd() % 64);
        for (uint32_t d : {1u, 2u, 3u, (uint32_t)(1 + rnd() % 65), 64u, 65u}) {
            if (mk::copy_level_off(c, d) != naive_level_off(c, d)) die(none, "level offset of a large array", c, d);
            ++g_offsets;
        }
        uint32_t D = 0;
        for (uint64_t x = c; x > 1; x = x / 2 + (x & 1)) ++D;
        const mk::CopyShape real = mk::copy_shape(c, c, c, 128, false);  // one item per chunk: nchunks == n
        if (real.D != D || real.nchunks != c) die(none, "D of a large list", c, real.D);
        uint64_t x = c;
        for (uint32_t d = 1; d <= D; ++d) {
            x = x / 2 + (x & 1);
            if (mk::copy_level_count(real, d) != x) die(none, "level count of a large list", c, d);
        }
    }
    std::fprintf(stderr, "%llu cases clean, %llu pieces replayed, %llu level offsets compared\n",
                 (unsigned long long)g_cases, (unsigned long long)g_pieces, (unsigned long long)g_offsets);
    return 0;
}
