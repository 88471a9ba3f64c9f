// Stand-alone host fuzz of the undo journal's slot map
// (prysm_amd/csrc/tree_journal.hpp, shared with k_trees_journal /
// k_trees_restore and the host side of mk_dev_ssz_trees_journal): built with
// -fsanitize=address,undefined and run as a child process by
// tests/test_tree_journal_fuzz.py.
//
//   tree_journal_fuzz SEED RANDOM_CASES
//
// Every case: (item_len, level 0 or not, capacity, n_old, n_new, an index
// list, ascending or not, with indices at and beyond n_old in it).  Checked:
//   every piece's journal bytes lie inside journal_tree_bytes, no two distinct
//   pieces share a byte, and together they are exactly the index list, the
//   root and per work item the value, the level-0 entry and D nodes;
//   every piece's tree-side bytes lie inside what the OLD counts specify (the
//   values below n_old, level 0 below n_old, a node below its level's old
//   count, at the offset of a naive sum over the capacity's levels);
//   every ancestor of every dirty or appended chunk that exists in the old
//   tree -- a naive walk over the old counts -- is saved by some work item.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "tree_journal.hpp"

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t g_cases, g_pieces, g_ancestors;

struct Case {
    uint32_t item_len;
    bool level0;
    uint64_t cap, n_old, n_new;
    std::vector<uint64_t> idx;
};

static void die(const Case& c, const char* what, uint64_t a = 0, uint64_t b = 0) {
    std::fprintf(stderr, "%s (%llu, %llu): item_len %u, level0 %d, capacity %llu, n_old %llu, n_new %llu, k %zu\n", what,
                 (unsigned long long)a, (unsigned long long)b, c.item_len, (int)c.level0, (unsigned long long)c.cap,
                 (unsigned long long)c.n_old, (unsigned long long)c.n_new, c.idx.size());
    std::exit(1);
}

static uint64_t cdiv(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

static void check(const Case& c) {
    const mk::JournalShape s = mk::journal_shape(c.n_old, c.n_new, c.cap, c.idx.size(), c.item_len, c.level0);
    const uint32_t leaf = c.level0 ? 32 : c.item_len;
    const uint64_t p = leaf < 128 ? 128 / leaf : 1;
    const uint64_t nch = cdiv(c.n_old, p), capch = cdiv(c.cap, p);
    // the old tree, naively: counts of level 1 .. D, and where a level starts in the capacity's layout
    std::vector<uint64_t> cnt{nch}, off{0}, capcnt{capch};
    while (cnt.back() > 1) {
        off.push_back(cnt.size() == 1 ? 0 : off.back() + capcnt.back());
        capcnt.push_back(cdiv(capcnt.back(), 2));
        cnt.push_back(cdiv(cnt.back(), 2));
    }
    const uint32_t D = (uint32_t)cnt.size() - 1;
    if (s.D != D || s.nchunks != nch || s.p != p) die(c, "shape", s.D, D);
    const uint64_t want_W = c.n_old ? c.idx.size() + (c.n_new > c.n_old) : 0;
    if (s.W != want_W) die(c, "work items", s.W, want_W);
    uint64_t levels_nodes = 0;  // nodes of the capacity's level array
    for (uint64_t m = capch; m > 1;) levels_nodes += (m = cdiv(m, 2));

    const uint64_t bytes = mk::journal_tree_bytes(s);
    if (bytes % 16 || mk::journal_root_off(s) % 16 || mk::journal_rec_bytes(s) % 16) die(c, "a part off 16 bytes");
    std::vector<uint64_t> heap_idx(c.idx);  // exactly k entries: a read outside is ASan's to report
    std::set<std::pair<uint64_t, uint64_t>> saved;  // (level, node)
    for (uint32_t unit : {1u, 8u, 16u}) {
        if (c.item_len % unit) continue;
        std::vector<uint8_t> used(bytes, 0);
        const uint64_t total = mk::journal_pieces(s, unit);
        uint64_t covered = 0;
        for (uint64_t g = 0; g < total + 3; ++g) {
            const mk::JournalPiece pc = mk::journal_piece(s, unit, g);
            if (g >= total) {
                if (pc.kind != mk::kJournalNone) die(c, "a piece beyond the total", g, pc.kind);
                continue;
            }
            if (pc.kind == mk::kJournalNone) die(c, "no piece below the total", g, total);
            if (pc.jr_off + pc.len > bytes) die(c, "a slot beyond the reported size", pc.jr_off + pc.len, bytes);
            for (uint32_t b = 0; b < pc.len; ++b)
                if (used[pc.jr_off + b]++) die(c, "two pieces share a journal byte", g, pc.jr_off + b);
            covered += pc.len;
            ++g_pieces;
            if (pc.kind == mk::kJournalRoot) {
                if (pc.at + pc.len > 32) die(c, "root piece", pc.at);
                continue;
            }
            if (pc.w >= s.W) die(c, "work item", pc.w, s.W);
            const uint64_t x = mk::journal_value(s, pc.w, pc.w < heap_idx.size() ? heap_idx[pc.w] : 0);
            if (x >= c.n_old) die(c, "a value at or beyond n_old", x);
            if (pc.w < c.idx.size() && c.idx[pc.w] < c.n_old && x != c.idx[pc.w]) die(c, "a listed index moved", x);
            if (pc.kind == mk::kJournalItem) {
                if (pc.len != unit || x * c.item_len + pc.at + pc.len > c.n_old * c.item_len) die(c, "value piece", x);
            } else if (pc.kind == mk::kJournalLevel0) {
                if (!c.level0 || pc.at + pc.len > 32) die(c, "level-0 piece", x);
            } else if (pc.kind == mk::kJournalNode) {
                const uint32_t d = pc.level;
                if (d < 1 || d > D || pc.at + pc.len > 32) die(c, "node piece", d, D);
                if (!mk::journal_node_exists(s, x, d)) die(c, "a slot for a node the old tree has not", d, x);
                const uint64_t node = (x / p) >> d;
                if (node >= cnt[d]) die(c, "a node beyond its level's old count", d, node);
                const uint64_t want = 32 * (off[d] + node);
                if (mk::journal_node_off(s, x, d) != want) die(c, "node offset", mk::journal_node_off(s, x, d), want);
                if (want + 32 > 32 * levels_nodes) die(c, "a node outside the level array", want, levels_nodes);
                saved.insert({d, node});
            } else if (pc.kind != mk::kJournalIndex || pc.len != 8) {
                die(c, "piece kind", pc.kind);
            }
        }
        const uint64_t want = 8 * s.W + 32 + s.W * (c.item_len + 32ull * c.level0 + 32ull * D);
        if (covered != want) die(c, "bytes covered", covered, want);
    }
    // the naive walk: what the update stores of what the old counts specify
    std::vector<uint64_t> dirty;
    for (uint64_t i : c.idx)
        if (i < c.n_old) dirty.push_back(i / p);
    for (uint64_t i = c.n_old; i < c.n_new; ++i) dirty.push_back(i / p);
    for (uint64_t ch : dirty)
        for (uint32_t d = 1; d <= D; ++d) {
            if ((ch >> d) >= cnt[d]) continue;  // not in the old tree
            ++g_ancestors;
            if (!saved.count({d, ch >> d})) die(c, "an ancestor the old tree has is not saved", d, ch >> d);
        }
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_state = std::strtoull(argv[1], nullptr, 0) * 0x9E3779B97F4A7C15ull + 5150;
    const uint64_t rounds = std::strtoull(argv[2], nullptr, 0);
    const uint32_t lens[] = {1, 3, 8, 16, 32, 48, 64, 100, 127, 128, 129, 160, 200};
    for (uint64_t r = 0; r < rounds; ++r) {
        Case c;
        c.item_len = lens[rnd() % (sizeof lens / sizeof *lens)];
        c.level0 = rnd() % 3 == 0;
        const uint32_t leaf = c.level0 ? 32 : c.item_len;
        const uint64_t p = leaf < 128 ? 128 / leaf : 1;
        const uint64_t shapes[] = {0, 1, p, p + 1, 2 * p, 2 * p + 1, 8 * p, 8 * p + 1, 33 * p - 1, rnd() % 700};
        c.n_old = shapes[rnd() % 10];
        const uint64_t apps[] = {0, 0, 1, p, 3 * p + 1, c.n_old, 3 * c.n_old + 5};
        c.n_new = c.n_old + apps[rnd() % 7];
        c.cap = c.n_new + (rnd() % 2 ? rnd() % 300 : 0);
        if (c.cap == 0) c.cap = 1;
        const uint64_t k = rnd() % 4 == 0 ? 0 : 1 + rnd() % 12;
        for (uint64_t i = 0; i < k; ++i) c.idx.push_back(rnd() % (c.n_old + 3));
        if (rnd() % 4) {  // ascending, as the update wants them; else any order, repeats included
            std::set<uint64_t> u(c.idx.begin(), c.idx.end());
            c.idx.assign(u.begin(), u.end());
        }
        check(c);
    }
    std::fprintf(stderr, "%llu cases clean, %llu pieces, %llu ancestors\n", (unsigned long long)g_cases,
                 (unsigned long long)g_pieces, (unsigned long long)g_ancestors);
    return 0;
}
