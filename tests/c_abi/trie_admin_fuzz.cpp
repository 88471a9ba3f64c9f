// Host fuzz of the deposit trie's roll back, fork point, audit and copy rules
// (prysm_amd/csrc/trie_admin.hpp): random sequences of append /
// roll back / fork point / audit / copy on two tries, each an exact-size heap
// array in the capacity layout, against a naive model (the leaf list, every
// level rebuilt from it).  Every load goes through a checked accessor: a node at
// or beyond its level's live count aborts the run; dead nodes hold poison, so a
// read that slipped through would also show in the values.  Built stand-alone
// with -fsanitize=address,undefined by tests/test_trie_admin_fuzz.py; the hash
// is a cheap stand-in for Keccak (the rules never look inside a node).
//   usage: trie_admin_fuzz SEED STEPS
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <utility>
#include <vector>

#include "trie_admin.hpp"

using mk::TrieNode;

namespace {

uint64_t g_rng = 1, g_reads = 0, g_hashes = 0;
uint64_t rnd() {
    g_rng += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

[[noreturn]] void die(const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) {
    fprintf(stderr, "FAIL: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
    abort();
}

bool same(const TrieNode& x, const TrieNode& y) { return memcmp(x.b, y.b, 32) == 0; }

TrieNode hash2(const TrieNode& l, const TrieNode& r) {
    ++g_hashes;
    uint64_t h[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
    for (int k = 0; k < 64; ++k) {
        const uint8_t v = k < 32 ? l.b[k] : r.b[k - 32];
        h[k & 3] = (h[k & 3] ^ v) * 0x100000001B3ull;
        h[(k + 1) & 3] ^= h[k & 3] >> 29;
    }
    TrieNode o;
    memcpy(o.b, h, 32);
    return o;
}

TrieNode leaf_of(uint64_t tag) {
    TrieNode a{}, b{};
    memcpy(a.b, &tag, 8);
    return hash2(a, b);
}

const TrieNode kPoison = [] {
    TrieNode p;
    memset(p.b, 0xFF, 32);
    return p;
}();

struct Trie {
    uint32_t depth;
    uint64_t cap, count = 0;
    TrieNode* lv;  // exactly ta_level_off(cap, depth + 1) nodes
    TrieNode root{};
    std::vector<TrieNode> leaves;  // the model

    Trie(uint32_t d, uint64_t c) : depth(d), cap(c), lv(alloc(c, d)) {}
    ~Trie() { delete[] lv; }
    Trie(const Trie&) = delete;
    Trie& operator=(const Trie&) = delete;

    static TrieNode* alloc(uint64_t cap, uint32_t depth) {
        const uint64_t n = mk::ta_level_off(cap, depth + 1);
        TrieNode* p = new TrieNode[n];
        for (uint64_t i = 0; i < n; ++i) p[i] = kPoison;
        return p;
    }
    // a load as of `as` deposits: the node must be live then
    TrieNode load(uint32_t d, uint64_t j, uint64_t as) const {
        ++g_reads;
        if (d > depth || j >= mk::ta_count(as, d)) die("dead node read", d, j, as);
        return lv[mk::ta_level_off(cap, d) + j];
    }
    void store(uint32_t d, uint64_t j, const TrieNode& v) {
        if (d > depth || j >= mk::ta_count(cap, d)) die("store outside the layout", d, j, cap);
        lv[mk::ta_level_off(cap, d) + j] = v;
    }
    void poison_dead() {
        for (uint32_t d = 0; d <= depth; ++d)
            for (uint64_t j = mk::ta_count(count, d); j < mk::ta_count(cap, d); ++j) store(d, j, kPoison);
    }
};

// the model: every level of `leaves` from scratch
std::vector<std::vector<TrieNode>> build(const std::vector<TrieNode>& leaves, uint32_t depth) {
    std::vector<std::vector<TrieNode>> L(depth + 1);
    L[0] = leaves;
    const TrieNode zero{};
    for (uint32_t d = 1; d <= depth; ++d)
        for (uint64_t j = 0; j < mk::ta_count(leaves.size(), d); ++j)
            L[d].push_back(hash2(L[d - 1][2 * j], 2 * j + 1 < L[d - 1].size() ? L[d - 1][2 * j + 1] : zero));
    return L;
}

void check_against_model(const Trie& t, const char* what) {
    if (t.count != t.leaves.size()) die("count", t.count, t.leaves.size());
    const auto L = build(t.leaves, t.depth);
    for (uint32_t d = 0; d <= t.depth; ++d)
        for (uint64_t j = 0; j < L[d].size(); ++j)
            if (!same(t.load(d, j, t.count), L[d][j])) die(what, d, j, t.count);
    const TrieNode zero{};
    if (!same(t.root, t.count ? L[t.depth][0] : zero)) die("root", t.count);
}

// the copy rule, piece by piece as k_trie_copy takes them
void copy_levels(const Trie& s, TrieNode* dst, uint64_t cap_dst) {
    const uint64_t pieces = mk::ta_copy_first(s.count, s.depth + 1);
    for (uint64_t q = 0; q < pieces; ++q) {
        uint32_t d = 0;
        while (d < s.depth && mk::ta_copy_first(s.count, d + 1) <= q) ++d;
        const uint64_t r = q - mk::ta_copy_first(s.count, d), j = r / 2;
        const TrieNode v = s.load(d, j, s.count);
        if (j >= mk::ta_count(cap_dst, d)) die("copy outside the destination", d, j, cap_dst);
        memcpy(dst[mk::ta_level_off(cap_dst, d) + j].b + 16 * (r & 1), v.b + 16 * (r & 1), 16);
    }
}

void regrow(Trie& t, uint64_t cap) {
    TrieNode* nl = Trie::alloc(cap, t.depth);
    copy_levels(t, nl, cap);
    delete[] t.lv;
    t.lv = nl;
    t.cap = cap;
    for (uint32_t d = 0; d <= t.depth; ++d)  // the copy left every dead node of the new array alone
        for (uint64_t j = mk::ta_count(t.count, d); j < mk::ta_count(cap, d); ++j)
            if (!same(t.lv[mk::ta_level_off(cap, d) + j], kPoison)) die("copy wrote a dead node", d, j);
}

void append(Trie& t, uint64_t k) {
    const uint64_t full = 1ull << t.depth;
    if (t.count + k > full) k = full - t.count;
    if (t.count + k > t.cap) regrow(t, t.count + k + below(5));
    const TrieNode zero{};
    for (uint64_t a = 0; a < k; ++a) {
        const uint64_t i = t.count;
        const TrieNode leaf = leaf_of(rnd());
        t.leaves.push_back(leaf);
        t.count = i + 1;
        t.store(0, i, leaf);
        for (uint32_t d = 0; d < t.depth; ++d) {  // the right edge, reading live nodes only
            const uint64_t q = i >> d;
            const TrieNode v = (q & 1) ? hash2(t.load(d, q - 1, t.count), t.load(d, q, t.count))
                                       : hash2(t.load(d, q, t.count), zero);
            t.store(d + 1, q >> 1, v);
        }
        t.root = t.load(t.depth, 0, t.count);
    }
}

void rollback(Trie& t, uint64_t c) {
    const uint64_t nodes = mk::ta_level_off(t.cap, t.depth + 1);
    std::vector<TrieNode> before(t.lv, t.lv + nodes);
    std::set<std::pair<uint32_t, uint64_t>> wrote;
    const uint64_t count = t.count;
    t.root = mk::ta_truncate(
        count, c, t.depth, [&](uint32_t d, uint64_t j) { return t.load(d, j, c ? c : 1); },
        [&](uint32_t d, uint64_t j, const TrieNode& v) {
            wrote.insert({d, j});
            t.store(d, j, v);
        },
        hash2);
    for (const auto& w : wrote) {
        const bool straddler = w.first >= 1 && mk::ta_chain_first(count, c, t.depth) && count > c &&
                               (c & ((1ull << w.first) - 1)) != 0 && w.second == mk::ta_path_node(c, w.first);
        if (!straddler && !(c == 0 && w.first == t.depth && w.second == 0)) die("roll back wrote", w.first, w.second, c);
    }
    for (uint32_t d = 0; d <= t.depth; ++d)
        for (uint64_t j = 0; j < mk::ta_count(t.cap, d); ++j) {
            const uint64_t at = mk::ta_level_off(t.cap, d) + j;
            if (!wrote.count({d, j}) && !same(before[at], t.lv[at])) die("roll back changed", d, j, c);
        }
    t.count = c;
    t.leaves.resize(c);
    check_against_model(t, "roll back");
    t.poison_dead();
}

void fork(const Trie& a, const Trie& b) {
    const uint64_t m = a.count < b.count ? a.count : b.count;
    uint64_t want = m;
    for (uint64_t i = 0; i < m; ++i)
        if (!same(a.leaves[i], b.leaves[i])) {
            want = i;
            break;
        }
    const uint64_t got = mk::ta_fork_point(a.count, b.count, a.depth, [&](uint32_t d, uint64_t j) {
        if (((j + 1) << d) > m) die("a node that is not comparable was compared", d, j, m);
        return !same(a.load(d, j, m), b.load(d, j, m));
    });
    if (got != want) die("fork point", got, want, m);
}

void audit(Trie& t) {
    std::vector<std::pair<uint32_t, uint64_t>> bad;
    auto run = [&](const TrieNode& root) {
        bad.clear();
        return mk::ta_audit(
            t.count, t.depth, root, 64u, [&](uint32_t d, uint64_t j) { return t.load(d, j, t.count ? t.count : 1); },
            hash2, [&](uint32_t d, uint64_t j) { bad.push_back({d, j}); });
    };
    if (t.count == 0) {
        if (run(TrieNode{}) != 0) die("audit of an empty trie");
        if (run(kPoison) != 1 || bad[0].first != 64u) die("audit of an empty trie's root");
        return;
    }
    if (run(t.root) != 0) die("audit of a sound trie", bad[0].first, bad[0].second);
    const uint32_t d = (uint32_t)below(t.depth + 1);
    const uint64_t j = below(mk::ta_count(t.count, d));
    TrieNode& n = t.lv[mk::ta_level_off(t.cap, d) + j];
    n.b[below(32)] ^= (uint8_t)(1u << below(8));
    const uint64_t k = run(t.root);
    std::vector<std::pair<uint32_t, uint64_t>> want;
    if (d >= 1) want.push_back({d, j});
    want.push_back(d == t.depth ? std::make_pair(64u, (uint64_t)0) : std::make_pair(d + 1, j >> 1));
    if (k != want.size() || bad != want) die("audit after a flip", d, j, k);
    t.lv[mk::ta_level_off(t.cap, d) + j] = build(t.leaves, t.depth)[d][j];
    // a dead node and the items' numbering
    if (mk::ta_count(t.count, 1) < mk::ta_count(t.cap, 1)) {
        t.lv[mk::ta_level_off(t.cap, 1) + mk::ta_count(t.count, 1)].b[3] ^= 1;
        if (run(t.root) != 0) die("audit read a dead node");
        t.poison_dead();
    }
    uint64_t items = 1;
    for (uint32_t e = 1; e <= t.depth; ++e) {
        if (mk::ta_audit_first(t.count, t.depth, e - 1) != items - 1) die("audit numbering", e);
        items += mk::ta_count(t.count, e);
    }
    if (mk::ta_audit_items(t.count, t.depth) != items) die("audit items", items);
}

void copy_to(const Trie& s, Trie& dst) {
    if (s.count > dst.cap) {
        delete[] dst.lv;
        dst.lv = Trie::alloc(s.cap, s.depth);
        dst.cap = s.cap;
    }
    copy_levels(s, dst.lv, dst.cap);
    dst.count = s.count;
    dst.root = s.root;
    dst.leaves = s.leaves;
    dst.poison_dead();
    check_against_model(dst, "copy");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_rng = strtoull(argv[1], nullptr, 10);
    const uint64_t steps = strtoull(argv[2], nullptr, 10);
    uint64_t cases = 0, rollbacks = 0;
    for (uint32_t round = 0; round < 4; ++round) {
        const uint32_t depth = round == 0 ? 1 : round == 1 ? 6 : round == 2 ? 10 : 32;
        const uint64_t lim = depth < 10 ? (1ull << depth) : 700;
        Trie a(depth, 1 + below(8)), b(depth, 1 + below(8));
        Trie* t[2] = {&a, &b};
        for (uint64_t s = 0; s < steps / 4; ++s, ++cases) {
            Trie& x = *t[below(2)];
            switch (below(8)) {
                case 0:
                case 1: {
                    uint64_t k = 1 + below(below(4) ? 4 : 40);
                    if (x.count + k > lim) k = lim - x.count;
                    append(x, k);
                    check_against_model(x, "append");
                    break;
                }
                case 2:
                case 3: {
                    const uint64_t pick = below(6);
                    uint64_t c = pick == 0 ? 0 : pick == 1 ? x.count : pick == 2 && x.count ? x.count - 1 : below(x.count + 1);
                    if (pick == 3 && x.count > 1) c = 1ull << below(64 - __builtin_clzll(x.count - 1));
                    rollback(x, c);
                    ++rollbacks;
                    break;
                }
                case 4:
                case 5:
                    fork(a, b);
                    fork(x, x);
                    break;
                case 6:
                    audit(x);
                    break;
                default:
                    copy_to(x, &x == &a ? b : a);
                    fork(a, b);
                    break;
            }
        }
    }
    fprintf(stderr, "%llu cases clean, %llu roll backs, %llu nodes read, %llu hashes\n", (unsigned long long)cases,
            (unsigned long long)rollbacks, (unsigned long long)g_reads, (unsigned long long)g_hashes);
    return 0;
}
