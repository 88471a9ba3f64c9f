// Stand-alone host fuzz of the rule of two resident trees' diff
// (prysm_amd/csrc/tree_diff.hpp, shared with k_trees_diff and the host side of
// mk_dev_ssz_trees_diff): built with -fsanitize=address,undefined and run as a
// child process by tests/test_tree_diff_fuzz.py.
//
//   tree_diff_fuzz SEED RANDOM_CASES
//
// Every case: a kind (a list tree of item_len 1..128, or 32-byte level-0
// entries), n_a, cap_a, n_b, cap_b drawn independently (often equal, often one
// apart, often a chunk or a work item's end), a subtree height h in 1..10 and a
// change set over the values below min(n_a, n_b).  A naive model builds both
// trees over the real message layout -- level 1 over the list bytes of two
// chunks, 0^128 behind an odd last chunk, level d over two children or a child
// and 0^128 -- with a 32-byte mixing function in place of Keccak, so the
// zero-pad collision of the real tree hash exists here too (half of the longer
// trees continue the shorter one with zero values).  The leaves and every
// level's live nodes lie in heap buffers of exactly their size, so a read at or
// beyond a count is ASan's to report as well as this program's; where a node
// lies in a level array laid out for its capacity is compared with the loop
// mk_ssz_list_tree_levels_bytes sums with.  The header's descent is replayed
// for every work item: the result must be the leaf-wise answer, every node
// read must be comparable, visited and inside both trees' counts, and the work
// items must be the visited nodes of level h0, each once.  For random 64-bit
// counts the shape and the predicates are compared with 128-bit arithmetic.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "tree_diff.hpp"

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t g_cases, g_reads, g_items, g_wide, g_collisions;

struct Case {
    uint64_t n_a, cap_a, n_b, cap_b;
    uint32_t len0, h;
};

[[noreturn]] static void die(const Case& c, const char* what, uint64_t a = 0, uint64_t b = 0) {
    std::fprintf(stderr, "%s (%llu, %llu): n_a %llu, cap_a %llu, n_b %llu, cap_b %llu, len0 %u, h %u\n", what,
                 (unsigned long long)a, (unsigned long long)b, (unsigned long long)c.n_a, (unsigned long long)c.cap_a,
                 (unsigned long long)c.n_b, (unsigned long long)c.cap_b, c.len0, c.h);
    std::exit(1);
}

// ---- the model: the layout rule and the tree, naively -----------------------------------------------
static uint64_t per_of(uint32_t len0) { return len0 < 128 ? 128 / len0 : 1; }
static uint64_t chunks_of(uint64_t n, uint32_t len0) { return n / per_of(len0) + (n % per_of(len0) != 0); }

static uint64_t naive_level_off(uint64_t cap_chunks, uint32_t d) {
    uint64_t off = 0, c = cap_chunks;
    for (uint32_t i = 1; i < d; ++i) {
        c = c / 2 + (c & 1);
        off += c;
    }
    return off;
}

struct Node {
    uint8_t b[32];
};

// any 32-byte mixing function of a message: four chained 64-bit lanes
static Node mix(const std::vector<uint8_t>& msg) {
    uint64_t l[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
    for (size_t i = 0; i < msg.size(); ++i) {
        l[i & 3] = (l[i & 3] ^ msg[i]) * 0x100000001B3ull;
        l[(i + 1) & 3] += l[i & 3] >> 29;
    }
    l[0] ^= msg.size();
    for (int r = 0; r < 8; ++r) l[r & 3] = (l[r & 3] ^ (l[(r + 1) & 3] >> 31)) * 0xBF58476D1CE4E5B9ull + r;
    Node n;
    std::memcpy(n.b, l, 32);
    return n;
}

struct Tree {
    uint64_t n = 0, cap = 0, nchunks = 0;
    uint32_t len0 = 0, D = 0;
    std::unique_ptr<uint8_t[]> leaves;                // exactly n * len0 bytes
    std::vector<std::unique_ptr<Node[]>> level;       // [d - 1]: exactly count(d) nodes
    std::vector<uint64_t> count;                      // [d - 1]
};

static Tree build(const std::vector<uint8_t>& bytes, uint64_t n, uint64_t cap, uint32_t len0) {
    Tree t;
    t.n = n, t.cap = cap, t.len0 = len0;
    t.nchunks = chunks_of(n, len0);
    t.leaves.reset(new uint8_t[n * len0]);
    std::memcpy(t.leaves.get(), bytes.data(), n * len0);
    const uint64_t cb = per_of(len0) * len0, total = n * len0;
    uint64_t c = t.nchunks;
    const Node* below = nullptr;
    while (c > 1) {
        const uint64_t up = c / 2 + (c & 1);
        std::unique_ptr<Node[]> nodes(new Node[up]);
        for (uint64_t j = 0; j < up; ++j) {
            std::vector<uint8_t> msg;
            if (!below) {
                const uint64_t lo = 2 * j * cb, hi = std::min(total, (2 * j + 2) * cb);
                msg.assign(bytes.begin() + lo, bytes.begin() + hi);
            } else {
                msg.insert(msg.end(), below[2 * j].b, below[2 * j].b + 32);
                if (2 * j + 1 < c) msg.insert(msg.end(), below[2 * j + 1].b, below[2 * j + 1].b + 32);
            }
            if (2 * j + 1 >= c) msg.insert(msg.end(), 128, 0);  // the odd pad
            nodes[j] = mix(msg);
        }
        below = nodes.get();
        t.level.push_back(std::move(nodes));
        t.count.push_back(up);
        c = up;
    }
    t.D = (uint32_t)t.level.size();
    return t;
}

// ---- one case -----------------------------------------------------------------------------------
static void run_case(const Case& c, bool zero_tail, int force_mode = -1) {
    const uint32_t L = c.len0;
    const uint64_t p = per_of(L), m = std::min(c.n_a, c.n_b), top = std::max(c.n_a, c.n_b);
    std::vector<uint8_t> xa(top * L + 1), xb;
    for (auto& v : xa) v = (uint8_t)rnd();
    if (zero_tail) std::fill(xa.begin() + m * L, xa.end(), 0);  // the longer tree continues with zero values
    xb = xa;
    const uint64_t mode = force_mode >= 0 ? (uint64_t)force_mode : rnd() % 5;  // none, one, a few, one per chunk, dense
    std::vector<uint64_t> want;
    for (uint64_t i = 0; i < m; ++i) {
        const bool hit = mode == 1   ? i == (c.n_a * 7 + 3) % m
                         : mode == 2 ? rnd() % 97 == 0
                         : mode == 3 ? i % p == p - 1
                         : mode == 4 ? rnd() % 3 != 0
                                     : false;
        if (!hit) continue;
        xb[i * L + rnd() % L] ^= (uint8_t)(1u << (rnd() % 8));
        want.push_back(i);
    }
    const Tree a = build(xa, c.n_a, c.cap_a, L), b = build(xb, c.n_b, c.cap_b, L);
    const mk::DiffShape s = mk::diff_shape(c.n_a, c.cap_a, c.n_b, c.cap_b, L, c.h);
    if (s.Da != a.D || s.Db != b.D) die(c, "D differs from the model's", s.Da, s.Db);
    if (s.h0 != std::min(c.h, std::min(a.D, b.D)) || s.m != m || s.p != p) die(c, "h0, m or p", s.h0, s.m);
    if (s.mch != chunks_of(m, L) || s.mfull != m / p) die(c, "chunk counts of m", s.mch, s.mfull);
    // the work items: the visited nodes of level h0, each once
    uint64_t roots = 0;
    while (m && (s.h0 ? (roots << s.h0) * p < m : roots < 1)) ++roots;
    if (mk::diff_items(s) != roots) die(c, "work items", mk::diff_items(s), roots);
    std::vector<uint64_t> got;
    std::vector<uint8_t> seen_root(roots, 0);
    for (uint64_t q = 0; q < roots; ++q) {
        auto node_ne = [&](uint32_t d, uint64_t j) {
            ++g_reads;
            if (d > s.h0 || (j >> (s.h0 - d)) != q) die(c, "a node outside the work item's subtree", d, j);
            if (d < 1 || d > std::min(a.D, b.D)) die(c, "a level above min(D_a, D_b)", d, j);
            if (j >= a.count[d - 1] || j >= b.count[d - 1]) die(c, "a node at or beyond a level's count", d, j);
            if (!((j << d) * p < m)) die(c, "a node that is not visited", d, j);
            if (!(c.n_a == c.n_b || ((j + 1) << d) * p <= m)) die(c, "a node that is not comparable was read", d, j);
            if (mk::diff_node_a(s, d, j) != naive_level_off(chunks_of(c.cap_a, L), d) + j ||
                mk::diff_node_b(s, d, j) != naive_level_off(chunks_of(c.cap_b, L), d) + j)
                die(c, "where a node lies in its level array", d, j);
            return std::memcmp(a.level[d - 1][j].b, b.level[d - 1][j].b, 32) != 0;
        };
        auto leaf_ne = [&](uint64_t i) {
            if (i >= m) die(c, "a leaf at or beyond m", i, m);
            return std::memcmp(a.leaves.get() + i * L, b.leaves.get() + i * L, L) != 0;
        };
        if (seen_root[q]++) die(c, "a work item twice", q);
        mk::diff_walk(s, q, node_ne, leaf_ne, [&](uint64_t i) { got.push_back(i); });
        ++g_items;
    }
    std::sort(got.begin(), got.end());
    if (got != want) die(c, "the result is not the leaf-wise answer", got.size(), want.size());
    // the collision is in the model: a straddling level-1 node over a last odd chunk is byte-equal to the longer
    // tree's when zero values follow, and the result above did not depend on it
    if (zero_tail && L * p == 128 && c.n_a != c.n_b && want.empty() && m % p == 0 && (m / p) % 2 == 1 &&
        std::min(a.D, b.D) >= 1 && top >= m + p) {
        const uint64_t j = (m / p) / 2;
        if (std::memcmp(a.level[0][j].b, b.level[0][j].b, 32) != 0) die(c, "the zero-pad collision is missing", j);
        ++g_collisions;
    }
    ++g_cases;
}

static uint64_t pick_n(uint32_t len0, uint32_t h) {
    const uint64_t p = per_of(len0), H = (p << h);
    switch (rnd() % 8) {
        case 0: return rnd() % 3;
        case 1: return p * (rnd() % 40);
        case 2: return p * (rnd() % 40) + 1;
        case 3: return H * (1 + rnd() % 2) + (rnd() % 3) - 1;
        case 4: return p * (2 * (rnd() % 20) + 1);  // an odd chunk count: the pad
        default: return rnd() % 3000;
    }
}

// 64-bit counts: the shape and the predicates against 128-bit arithmetic, the offsets against the loop
static void wide_case() {
    typedef unsigned __int128 u128;
    const uint32_t len0 = 1 + (uint32_t)(rnd() % 128);
    const uint64_t p = per_of(len0), lim = UINT64_MAX / len0;
    const uint64_t n_a = rnd() % lim >> (rnd() % 50), n_b = rnd() % 4 ? rnd() % lim >> (rnd() % 50) : n_a;
    const uint64_t cap_a = n_a + (lim > n_a ? rnd() % (lim - n_a) : 0), cap_b = n_b + (lim > n_b ? rnd() % (lim - n_b) : 0);
    const uint32_t h = 1 + (uint32_t)(rnd() % 10);
    const mk::DiffShape s = mk::diff_shape(n_a, cap_a, n_b, cap_b, len0, h);
    const Case c{n_a, cap_a, n_b, cap_b, len0, h};
    const uint64_t m = std::min(n_a, n_b);
    auto depth = [&](uint64_t n) {
        uint32_t d = 0;
        for (uint64_t k = chunks_of(n, len0); k > 1; k = k / 2 + (k & 1)) ++d;
        return d;
    };
    if (s.Da != depth(n_a) || s.Db != depth(n_b)) die(c, "wide: D", s.Da, s.Db);
    const u128 span = ((u128)p) << s.h0;
    const uint64_t items = (uint64_t)(((u128)m + span - 1) / span);
    if (mk::diff_items(s) != items) die(c, "wide: work items", mk::diff_items(s), items);
    for (int k = 0; k < 24; ++k) {
        const uint32_t d = 1 + (uint32_t)(rnd() % std::max(1u, std::min(s.Da, s.Db)));
        if (d > std::min(s.Da, s.Db)) break;
        const uint64_t cnt = (uint64_t)(((u128)s.mch + (((u128)1) << d) - 1) >> d);
        const uint64_t j = k < 4 ? cnt - 1 - (k & 1 ? 0 : std::min<uint64_t>(cnt - 1, 1)) : rnd() % cnt;
        const bool vis = ((u128)j << d) * p < m, cmp = n_a == n_b || (((u128)j + 1) << d) * p <= m;
        if (mk::diff_visited(s, d, j) != vis || mk::diff_comparable(s, d, j) != cmp) die(c, "wide: a predicate", d, j);
        if (mk::diff_visited(s, d, cnt)) die(c, "wide: a node at the level's count is visited", d, cnt);
        if (mk::diff_node_a(s, d, j) != naive_level_off(chunks_of(cap_a, len0), d) + j ||
            mk::diff_node_b(s, d, j) != naive_level_off(chunks_of(cap_b, len0), d) + j)
            die(c, "wide: where a node lies", d, j);
        ++g_wide;
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: tree_diff_fuzz SEED RANDOM_CASES\n");
        return 2;
    }
    g_state = std::strtoull(argv[1], nullptr, 0);
    const uint64_t random_cases = std::strtoull(argv[2], nullptr, 0);
    // the two collision shapes by hand: 12 against 16 items of 32 bytes, 20 against 24
    for (uint64_t k : {12, 20}) run_case(Case{k, k + 3, k + 4, 2 * k + 9, 32, 10}, true, 0);
    if (g_collisions != 2) return 1;
    for (uint64_t k = 0; k < random_cases; ++k) {
        Case c{};
        c.len0 = rnd() % 3 == 0 ? 32 : 1 + (uint32_t)(rnd() % 128);
        c.h = 1 + (uint32_t)(rnd() % 10);
        c.n_a = pick_n(c.len0, c.h);
        const uint64_t rel = rnd() % 6;
        c.n_b = rel == 0 ? c.n_a : rel == 1 ? c.n_a + 1 : rel == 2 ? c.n_a + per_of(c.len0) : pick_n(c.len0, c.h);
        if (c.n_a > 40000 || c.n_b > 40000) c.n_a %= 40000, c.n_b %= 40000;
        if (rnd() & 1) std::swap(c.n_a, c.n_b);
        c.cap_a = c.n_a + (rnd() % 3 ? rnd() % (c.n_a + 5) : 0);
        c.cap_b = c.n_b + (rnd() % 3 ? rnd() % (2 * c.n_b + 9) : 0);
        run_case(c, (rnd() & 1) != 0);
        for (int w = 0; w < 8; ++w) wide_case();
    }
    std::fprintf(stderr, "%llu cases clean, %llu nodes read, %llu work items, %llu wide checks, %llu collisions met\n",
                 (unsigned long long)g_cases, (unsigned long long)g_reads, (unsigned long long)g_items,
                 (unsigned long long)g_wide, (unsigned long long)g_collisions);
    return 0;
}
