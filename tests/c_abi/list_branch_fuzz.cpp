// Stand-alone host fuzz of the list-tree proof arithmetic
// (prysm_amd/csrc/list_branch.hpp, shared by k_list_tree_branches,
// k_verify_list_branches and the host side): built with
// -fsanitize=address,undefined and run as a child process by
// tests/test_list_branch_fuzz.py.
//
//   list_branch_fuzz SEED RANDOM_CASES
//
// Every case: (n, capacity >= n, s in 1..128, i < n) against a naive model
// that materialises every level's count and capacity.  Asserted: the shape
// (p, cb, nchunks, D, the record stride), every level's offset, that every
// node index the header yields is below its level's count, that every window
// byte range ends at or before total and holds item i where the header says,
// and the presence rule of a sibling.  For lists small enough to allocate, the
// gather is replayed piece by piece out of heap buffers of exactly total and
// exactly the level array's bytes: a read outside them is ASan's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "list_branch.hpp"

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t g_cases, g_nodes, g_replayed;

#define CHECK(cond, what)                                                                                        \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::fprintf(stderr, "%s (%s): n %llu, capacity %llu, s %u, i %llu\n", what, #cond,                  \
                         (unsigned long long)n, (unsigned long long)cap, s, (unsigned long long)i);              \
            std::exit(1);                                                                                        \
        }                                                                                                        \
    } while (0)

static void check(uint64_t n, uint64_t cap, uint32_t s, uint64_t i, bool replay) {
    ++g_cases;
    // the naive model
    const uint64_t p = 128 / s, cb = p * s, total = n * s;
    const uint64_t nchunks = (n + p - 1) / p, cap_chunks = (cap + p - 1) / p;
    std::vector<uint64_t> count{nchunks}, capd{cap_chunks}, off{0, 0};  // index d; off[d]: first node of level d >= 1
    while (count.back() > 1) count.push_back((count.back() + 1) / 2);
    while (capd.back() > 1) capd.push_back((capd.back() + 1) / 2);
    const uint32_t D = (uint32_t)count.size() - 1;
    for (size_t d = 1; d + 1 < capd.size(); ++d) off.push_back(off[d] + capd[d]);
    uint64_t level_nodes = 0;
    for (size_t d = 1; d < capd.size(); ++d) level_nodes += capd[d];

    const mk::BranchShape b = mk::branch_shape(n, cap, s);
    CHECK(b.p == p && b.cb == cb && b.total == total && b.nchunks == nchunks && b.cap_chunks == cap_chunks, "shape");
    CHECK(b.D == D, "depth");
    CHECK(mk::branch_record_bytes(b) == 256 + 32ull * (D > 1 ? D - 1 : 0), "record stride");
    for (uint32_t d = 1; d <= D; ++d) {
        CHECK(mk::branch_level_count(b, d) == count[d], "level count");
        CHECK(mk::branch_level_off(b, d) == off[d], "level offset");
        CHECK(count[d] <= capd[d], "a level outgrew its capacity");
    }
    if (n == 0) return;

    const uint64_t j = mk::branch_window_index(b, i);
    CHECK(j == (nchunks >= 2 ? (i / p) / 2 : 0), "window index");
    CHECK(nchunks < 2 || j < count[1], "window beyond level 1");
    uint64_t lo;
    uint32_t len;
    mk::branch_window(b, j, &lo, &len);
    CHECK(len <= 256 && lo + len <= total, "window leaves the list");
    CHECK(len > 0, "empty window");
    const uint64_t want_lo = nchunks >= 2 ? 2 * j * cb : 0;
    const uint64_t want_hi = nchunks >= 2 ? (total < (2 * j + 2) * cb ? total : (2 * j + 2) * cb) : total;
    CHECK(lo == want_lo && lo + len == want_hi, "window range");
    const uint32_t pos = mk::branch_item_pos(b, i);
    CHECK(lo + pos == i * s && pos + s <= len, "item outside its window");
    CHECK(mk::branch_window_padded(b, j) == (nchunks >= 2 && 2 * j + 1 == nchunks), "window pad");

    std::vector<uint64_t> want_nodes;  // level-array node per slot, UINT64_MAX: a zero slot
    for (uint32_t d = 1; d < D; ++d) {
        uint64_t node = 0;
        const bool have = mk::branch_sibling(b, j, d, &node);
        const uint64_t q = j >> (d - 1), sib = q ^ 1;
        CHECK(q < count[d], "ancestor beyond its level");
        CHECK(have == (sib < count[d]), "sibling presence");
        if (have) {
            ++g_nodes;
            CHECK(node == sib && node < count[d], "node index at or beyond the level's count");
            CHECK(off[d] + node < level_nodes, "node outside the level array");
        } else {
            CHECK((q & 1) == 0 && q + 1 == count[d], "a missing sibling that is not the right edge's");
        }
        want_nodes.push_back(have ? off[d] + node : UINT64_MAX);
    }
    if (!replay) return;

    // the gather of k_list_tree_branches out of exact-size heap buffers
    ++g_replayed;
    std::vector<uint8_t> level0(total);
    for (uint64_t x = 0; x < total; ++x) level0[x] = (uint8_t)(x * 131 + 7);
    std::vector<uint8_t> levels(32 * level_nodes);
    for (uint64_t x = 0; x < levels.size(); ++x) levels[x] = (uint8_t)(x / 32 * 29 + x % 32 + 1);
    const uint32_t pieces = (uint32_t)(mk::branch_record_bytes(b) / 16);
    std::vector<uint8_t> rec(16 * pieces, 0xEE);
    const uint8_t* wsrc = level0.data() + lo;
    for (uint32_t q = 0; q < pieces; ++q) {
        uint8_t v[16] = {};
        if (q < 16) {
            const uint32_t a = 16 * q;
            if (a + 16 <= len)
                std::memcpy(v, wsrc + a, 16);
            else if (a < len)
                for (uint32_t e = 0; e < 16 && a + e < len; ++e) v[e] = wsrc[a + e];
        } else {
            const uint32_t d = 1 + ((q - 16) >> 1), h = (q - 16) & 1;
            uint64_t node;
            if (mk::branch_sibling(b, j, d, &node))
                std::memcpy(v, levels.data() + 32 * (mk::branch_level_off(b, d) + node) + 16 * h, 16);
        }
        std::memcpy(rec.data() + 16 * q, v, 16);
    }
    for (uint32_t x = 0; x < 256; ++x)
        CHECK(rec[x] == (x < len ? level0[lo + x] : 0), "window bytes");
    for (uint32_t d = 1; d < D; ++d)
        for (uint32_t x = 0; x < 32; ++x) {
            const uint64_t w = want_nodes[d - 1];
            CHECK(rec[256 + 32 * (d - 1) + x] == (w == UINT64_MAX ? 0 : levels[32 * w + x]), "sibling bytes");
        }
}

int main(int argc, char** argv) {
    g_state = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
    const uint64_t random_cases = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 2000;
    // every small shape, every index
    for (uint32_t s : {1u, 2u, 3u, 8u, 31u, 32u, 33u, 48u, 64u, 65u, 100u, 127u, 128u})
        for (uint64_t n = 0; n <= 41 * (128 / s) && n <= 700; n += (n < 70 ? 1 : 1 + rnd() % 9))
            for (uint64_t cap : {n, n + 1, 2 * n + 3, n + 1000}) {
                if (n == 0) check(0, cap, s, 0, false);
                for (uint64_t i = 0; i < n; i += (n < 70 ? 1 : 1 + rnd() % 5)) check(n, cap, s, i, true);
                if (n) check(n, cap, s, n - 1, true);
            }
    // random shapes small enough to replay
    for (uint64_t c = 0; c < random_cases; ++c) {
        const uint32_t s = 1 + (uint32_t)(rnd() % 128);
        const uint64_t n = 1 + rnd() % (1ull << (1 + rnd() % 16));
        const uint64_t cap = n + (rnd() % 3 ? rnd() % (n + 2) : 0);
        for (int t = 0; t < 4; ++t) check(n, cap, s, t == 0 ? n - 1 : rnd() % n, true);
    }
    // huge shapes: arithmetic only
    for (uint64_t c = 0; c < random_cases; ++c) {
        const uint32_t s = 1 + (uint32_t)(rnd() % 128);
        const uint64_t n = 1 + rnd() % (1ull << (17 + rnd() % 40));  // n * s < 2^64
        const uint64_t room = (UINT64_MAX / s) - n;
        const uint64_t cap = n + (rnd() % 2 ? rnd() % (room < (1ull << 40) ? room + 1 : (1ull << 40)) : 0);
        for (int t = 0; t < 4; ++t) check(n, cap, s, t == 0 ? n - 1 : rnd() % n, false);
    }
    std::fprintf(stderr, "%llu cases clean, %llu node indices, %llu gathers replayed\n", (unsigned long long)g_cases,
                 (unsigned long long)g_nodes, (unsigned long long)g_replayed);
    return 0;
}
