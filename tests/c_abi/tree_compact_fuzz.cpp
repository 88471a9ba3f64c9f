// Stand-alone host fuzz of the stable-erase index map
// (prysm_amd/csrc/tree_compact.hpp, shared with k_tree_compact): built with
// -fsanitize=address,undefined and run as a child process by
// tests/test_tree_compact_fuzz.py.
//
//   tree_compact_fuzz SEED RANDOM_CASES
//
// Every case: a list 0 .. n_old - 1, a strictly ascending removal list, and
// the naive filtered copy.  Checked against it: compact_src of every
// destination (and that positions below r_0 do not move), and the kernel's
// form -- a block of B consecutive destination pieces searches for its first
// and last destination and every piece bisects between the two
// (compact_skip_in) -- for several B and pieces per value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tree_compact.hpp"

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t g_cases, g_dests;

static void fail(const char* what, uint64_t n, const std::vector<uint64_t>& rm, uint64_t q, uint64_t got,
                 uint64_t want) {
    std::fprintf(stderr, "%s: n_old %llu, k %zu, destination %llu: source %llu, want %llu\n", what,
                 (unsigned long long)n, rm.size(), (unsigned long long)q, (unsigned long long)got,
                 (unsigned long long)want);
    std::exit(1);
}

static void check(uint64_t n, const std::vector<uint64_t>& rm, bool full = true) {
    const uint64_t k = rm.size();
    std::vector<uint64_t> want;  // the reference's append-into-a-new-slice loop
    {
        uint64_t i = 0;
        for (uint64_t s = 0; s < n; ++s) {
            if (i < k && rm[i] == s) {
                ++i;
                continue;
            }
            want.push_back(s);
        }
    }
    if (want.size() != n - k) fail("removal list not ascending below n_old", n, rm, 0, want.size(), n - k);
    // a heap copy of exactly k entries: a read outside it is ASan's to report
    std::vector<uint64_t> r(rm);
    const uint64_t* p = r.data();
    for (uint64_t q = 0; q < n - k; ++q) {
        const uint64_t s = mk::compact_src(p, k, q);
        if (s != want[q]) fail("compact_src", n, rm, q, s, want[q]);
        if (k && q < rm[0] && s != q) fail("a position below r_0 moved", n, rm, q, s, q);
    }
    // the kernel's form over destinations [first, n - k), first <= r_0
    const uint64_t first = k ? (rnd() % 2 ? rm[0] : rnd() % (rm[0] + 1)) : 0;
    const uint64_t moved = k && n - k > first ? n - k - first : 0;
    for (uint32_t per : {1u, 3u, 8u}) {
        for (uint32_t B : {1u, 4u, 64u, 256u}) {
            if (!full && (per != 1 || (B != 4 && B != 256))) continue;  // the exhaustive part: two block sizes
            const uint64_t pieces = moved * per;
            for (uint64_t g0 = 0; g0 < pieces; g0 += B) {
                const uint64_t last = g0 + B - 1 < pieces ? g0 + B - 1 : pieces - 1;
                const uint64_t jlo = mk::compact_skip(p, k, first + g0 / per);
                const uint64_t jhi = mk::compact_skip(p, k, first + last / per);
                if (jlo > jhi || jhi > k) fail("block bounds", n, rm, first + g0 / per, jlo, jhi);
                for (uint64_t g = g0; g <= last; ++g) {
                    const uint64_t q = first + g / per;
                    const uint64_t s = q + mk::compact_skip_in(p, jlo, jhi, q);
                    if (s != want[q]) fail("compact_skip_in", n, rm, q, s, want[q]);
                    ++g_dests;
                }
            }
        }
    }
    ++g_cases;
}

// any contents: the search stays inside rm and j <= k (so q + j < n_old)
static void check_garbage(uint64_t n, uint64_t k) {
    std::vector<uint64_t> r(k);
    for (auto& x : r) x = rnd() % 4 == 0 ? rnd() : rnd() % (n + 1);
    for (uint64_t q = 0; q < n - k; ++q) {
        const uint64_t j = mk::compact_skip(r.data(), k, q);
        if (j > k) fail("unbounded j", n, r, q, j, k);
    }
}

int main(int argc, char** argv) {
    g_state = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
    const uint64_t random_cases = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 200;
    // exhaustive: every n_old 0..300 with every removal list of k <= 1; every pair up to n_old = 96
    // and, above, every pair whose first index is at an end or in the middle; every triple up to 40
    for (uint64_t n = 0; n <= 300; ++n) {
        check(n, {});
        for (uint64_t a = 0; a < n; ++a) {
            check(n, {a});
            if (n <= 96 || a < 2 || a + 3 >= n || a == n / 2)
                for (uint64_t b = a + 1; b < n; ++b) check(n, {a, b}, false);
        }
        if (n <= 40)
            for (uint64_t a = 0; a < n; ++a)
                for (uint64_t b = a + 1; b < n; ++b)
                    for (uint64_t c = b + 1; c < n; ++c) check(n, {a, b, c}, false);
    }
    // the named cases at every n_old 1..300
    for (uint64_t n = 1; n <= 300; ++n) {
        std::vector<uint64_t> all, prefix, suffix, odd, even, ends{0};
        for (uint64_t i = 0; i < n; ++i) {
            all.push_back(i);
            if (i < n / 3 + 1) prefix.push_back(i);
            if (i >= n - n / 3 - 1) suffix.push_back(i);
            (i % 2 ? odd : even).push_back(i);
        }
        if (n > 1) ends.push_back(n - 1);
        check(n, {});          // nothing removed
        check(n, all);         // everything removed
        check(n, prefix);      // a prefix
        check(n, suffix);      // a suffix
        check(n, even);        // every other value, from the first
        check(n, odd);         // ... from the second
        check(n, ends);        // one index at each end
        all.erase(all.begin() + (long)(n / 2));
        check(n, all);         // all but one
    }
    // random: any k, runs and scattered
    for (uint64_t c = 0; c < random_cases; ++c) {
        const uint64_t n = rnd() % 301;
        std::vector<uint64_t> rm;
        const uint64_t dens = rnd() % 100, run = rnd() % 2;
        bool in = false;
        for (uint64_t i = 0; i < n; ++i) {
            if (run) {
                if (rnd() % 8 == 0) in = !in;
            } else {
                in = rnd() % 100 < dens;
            }
            if (in) rm.push_back(i);
        }
        check(n, rm);
        if (n) check_garbage(n, rnd() % (n + 1));
    }
    std::fprintf(stderr, "%llu cases clean, %llu block destinations\n", (unsigned long long)g_cases,
                 (unsigned long long)g_dests);
    return 0;
}
