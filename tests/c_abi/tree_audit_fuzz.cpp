// Stand-alone host fuzz of the work-item map of a resident tree's audit
// (prysm_amd/csrc/tree_audit.hpp, shared with k_trees_audit and the host side
// of mk_dev_ssz_trees_audit): built with -fsanitize=address,undefined and run as
// a child process by tests/test_tree_audit_fuzz.py.
//
//   tree_audit_fuzz SEED RANDOM_CASES
//
// Every case: a tree shape (len0 1..128, n 0..5000, capacity >= n) and a naive
// model of the layout rule of include/prysm_merkle.h -- the chunk count, every
// level's live count by repeated halving, every level's first node in the level
// array by the loop mk_ssz_list_tree_levels_bytes sums with.  The model keeps
// every live extent (level 0's n * len0 bytes, each level's live nodes, the
// root) in a heap buffer of exactly its size, so a work item that reads outside
// one is ASan's to report as well as this program's.  Every work item of the
// header's map is replayed: its message must be the rule's (which bytes, how
// many, the 0^128, the mix-in) and lie inside the live extent of the level
// below, its stored node inside the live extent of its own level.  Afterwards
// every live node has been checked exactly once and every live byte below the
// root has been read exactly once.  D, the item total and the level offsets
// (also for random 64-bit chunk counts, where no buffer could check them) are
// compared with the model's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tree_audit.hpp"

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t g_cases, g_items, g_offsets;

struct Case {
    uint64_t n, cap;
    uint32_t len0;
};

[[noreturn]] static void die(const Case& c, const char* what, uint64_t a = 0, uint64_t b = 0) {
    std::fprintf(stderr, "%s (%llu, %llu): n %llu, capacity %llu, len0 %u\n", what, (unsigned long long)a,
                 (unsigned long long)b, (unsigned long long)c.n, (unsigned long long)c.cap, c.len0);
    std::exit(1);
}

// ---- the model: the layout rule, naively ----------------------------------------------------------
static uint64_t chunks_of(uint64_t n, uint32_t leaf) {
    const uint64_t p = leaf < 128 ? 128 / leaf : 1;
    return n / p + (n % p != 0);
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
        c = c / 2 + (c & 1);
        sum += c;
    }
    return sum;
}

// one live extent: exactly its bytes, where it starts in its buffer, how often each byte was read as part of a
// message and how often each 32-byte node was compared
struct Extent {
    uint64_t bytes = 0, at = 0;
    uint8_t *mem = nullptr, *reads = nullptr, *checks = nullptr;
    void make(uint64_t b, uint64_t start) {
        bytes = b, at = start;
        mem = (uint8_t*)std::malloc(b ? b : 1);  // malloc(0) may be null: the extent is then never touched
        reads = (uint8_t*)std::calloc(b ? b : 1, 1);
        checks = (uint8_t*)std::calloc(b / 32 + 1, 1);
        if (!mem || !reads || !checks) std::abort();
        std::memset(mem, 0x5a, b);
    }
    void drop() { std::free(mem), std::free(reads), std::free(checks); }
};

static void check(const Case& k) {
    const uint64_t p = k.len0 < 128 ? 128 / k.len0 : 1, cb = p * k.len0, total = k.n * k.len0;
    const uint64_t nch = chunks_of(k.n, k.len0), capc = chunks_of(k.cap, k.len0);
    std::vector<uint64_t> count;  // count[d - 1]: live nodes of level d
    for (uint64_t c = nch; c > 1;) {
        c = c / 2 + (c & 1);
        count.push_back(c);
    }
    const uint32_t D = (uint32_t)count.size();

    const mk::AuditShape sh = mk::audit_shape(k.n, k.cap, k.len0);
    if (sh.D != D) die(k, "D", sh.D, D);
    if (sh.nchunks != nch || sh.cap_chunks != capc || sh.total != total || sh.cb != cb) die(k, "shape");
    if (mk::audit_slots(sh) != D + 1) die(k, "slots");
    uint64_t want_items = 1;
    for (uint64_t c : count) want_items += c;
    if (mk::audit_items(sh) != want_items) die(k, "item total", mk::audit_items(sh), want_items);
    // every stored level ends inside the level array of the capacity
    if (D && naive_level_off(capc, D) + count[D - 1] > naive_levels_nodes(capc)) die(k, "levels overrun");

    // the live extents: [0] level 0, [d] level d = 1 .. D, [D + 1] the root
    std::vector<Extent> ext(D + 2);
    ext[0].make(total, 0);
    for (uint32_t d = 1; d <= D; ++d) ext[d].make(32 * count[d - 1], 32 * naive_level_off(capc, d));
    ext[D + 1].make(32, 0);

    uint64_t first = 0;
    for (uint32_t s = 0; s <= D; ++s) {  // where every slot starts: its items, its messages, its nodes
        if (mk::audit_slot_first(sh, s) != first) die(k, "first item of a slot", s, first);
        first += s < D ? count[s] : 1;
        uint32_t cbuf, nbuf;
        uint64_t coff, noff;
        mk::audit_slot_child(sh, s, &cbuf, &coff);
        mk::audit_slot_node(sh, s, &nbuf, &noff);
        const bool below0 = s == 0 || D == 0;
        if (cbuf != (below0 ? mk::kAuditLevel0 : mk::kAuditLevels)) die(k, "buffer of a slot's messages", s);
        if (coff != (below0 ? 0 : ext[s].at)) die(k, "offset of a slot's messages", s, coff);
        if (nbuf != (s == D ? mk::kAuditRootBuf : mk::kAuditLevels)) die(k, "buffer of a slot's nodes", s);
        if (noff != (s == D ? 0 : ext[s + 1].at)) die(k, "offset of a slot's nodes", s, noff);
        g_offsets += 2;
    }
    if (mk::audit_slot_first(sh, D + 1) != want_items) die(k, "the slot behind the last");

    uint8_t sink[256];
    for (uint64_t q = 0; q < want_items; ++q) {
        uint32_t s = 0;
        const mk::AuditItem it = mk::audit_item(sh, q, &s);
        if (s > D) die(k, "slot of an item", q, s);
        const uint64_t j = q - mk::audit_slot_first(sh, s);
        if (it.index != j) die(k, "index of an item", q, it.index);
        const uint32_t level = s == D ? mk::kAuditRoot : s + 1;
        if (it.level != level) die(k, "level of an item", q, it.level);
        if (it.mixin != (s == D)) die(k, "mix-in", q);
        // the rule's message
        Extent& below = ext[(s == D && D > 0) ? D : s];  // level 0 under the windows and a short list's root
        uint64_t want_off, want_len, want_zeros;
        if (s == D && D == 0) {
            want_off = 0, want_len = total, want_zeros = k.n == 0 ? 128 : 0;
        } else if (s == D) {
            want_off = 0, want_len = 32, want_zeros = 0;
        } else if (s == 0) {
            want_off = 2 * j * cb;
            const uint64_t end = (2 * j + 2) * cb < total ? (2 * j + 2) * cb : total;
            want_len = end - want_off;
            want_zeros = 2 * j + 1 == nch ? 128 : 0;
        } else {
            want_off = 64 * j;
            const bool pad = 2 * j + 1 >= count[s - 1];
            want_len = pad ? 32 : 64, want_zeros = pad ? 128 : 0;
        }
        if (it.child_off != want_off || it.msg_len != want_len || it.zeros != want_zeros)
            die(k, "message of an item", q, it.child_off);
        if (it.msg_len > 256) die(k, "message length", q, it.msg_len);
        if (it.child_off + it.msg_len > below.bytes) die(k, "a message outside the live extent below", q, it.child_off);
        std::memcpy(sink, below.mem + it.child_off, it.msg_len);  // exact-size buffers: an overrun is ASan's
        for (uint32_t i = 0; i < it.msg_len; ++i)
            if (++below.reads[it.child_off + i] != 1) die(k, "a byte hashed twice", q, it.child_off + i);
        // its stored node
        Extent& own = ext[s + 1];
        if (it.node_off != 32 * j || it.node_off + 32 > own.bytes) die(k, "a node outside its live extent", q, it.node_off);
        std::memcpy(sink, own.mem + it.node_off, 32);
        if (++own.checks[j] != 1) die(k, "a node checked twice", q, j);
        // the kernel's form: the slot looked up once, then audit_item_in
        const mk::AuditItem in = mk::audit_item_in(sh, s, j);
        if (std::memcmp(&in, &it, sizeof in)) die(k, "audit_item_in", q);
        ++g_items;
    }
    for (uint32_t e = 0; e <= D + 1; ++e) {
        for (uint64_t i = 0; e <= D && i < ext[e].bytes; ++i)
            if (ext[e].reads[i] != 1) die(k, "a live byte never hashed", e, i);
        for (uint64_t i = 0; e >= 1 && i < ext[e].bytes / 32; ++i)
            if (ext[e].checks[i] != 1) die(k, "a live node never checked", e, i);
    }
    for (Extent& e : ext) e.drop();
    ++g_cases;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s SEED RANDOM_CASES\n", argv[0]);
        return 2;
    }
    g_state = std::strtoull(argv[1], nullptr, 0);
    const uint64_t ncases = std::strtoull(argv[2], nullptr, 0);
    // the corners first: every small n at every kind of leaf length, a tight and a loose capacity
    for (uint32_t L : {1u, 5u, 8u, 32u, 33u, 48u, 64u, 65u, 100u, 127u, 128u})
        for (uint64_t n = 0; n <= 70; ++n) {
            check({n, n, L});
            check({n, n + 1, L});
            check({n, 2 * n + 3, L});
        }
    for (uint64_t i = 0; i < ncases; ++i) {
        Case k;
        k.len0 = 1 + (uint32_t)(rnd() % 128);
        if (rnd() % 3 == 0) k.len0 = 32;  // the struct / bytes trees
        k.n = rnd() % 5001;
        if (rnd() % 4 == 0) k.n = rnd() % 70;  // the small trees, where D changes fastest
        k.cap = k.n + (rnd() % 3 == 0 ? 0 : rnd() % 6000);
        check(k);
    }
    // the offsets against the loops for chunk counts no buffer could hold (one item per chunk: nchunks == n)
    const Case none{0, 0, 128};
    for (uint64_t i = 0; i < 20 * ncases + 1000; ++i) {
        const uint64_t cap = rnd() >> (6 + rnd() % 58);  // 32 * nodes stays below 2^64
        const uint64_t n = cap ? rnd() % (cap + 1) : 0;
        const mk::AuditShape sh = mk::audit_shape(n, cap, 128);
        uint32_t D = 0;
        uint64_t items = 1;
        for (uint64_t x = n; x > 1;) {
            x = x / 2 + (x & 1);
            items += x;
            ++D;
        }
        if (sh.D != D || sh.nchunks != n || sh.cap_chunks != cap) die(none, "shape of a large list", n, cap);
        if (mk::audit_items(sh) != items) die(none, "item total of a large list", n, items);
        uint64_t first = 0, x = n;
        for (uint32_t s = 0; s <= D; ++s) {
            if (mk::audit_slot_first(sh, s) != first) die(none, "first item of a slot of a large list", n, s);
            x = x / 2 + (x & 1);
            first += x;
            uint32_t buf;
            uint64_t off;
            mk::audit_slot_node(sh, s, &buf, &off);
            if (s < D && off != 32 * naive_level_off(cap, s + 1)) die(none, "node offset of a large array", cap, s);
            mk::audit_slot_child(sh, s, &buf, &off);
            if (s >= 1 && off != 32 * naive_level_off(cap, s)) die(none, "message offset of a large array", cap, s);
            g_offsets += 2;
        }
        if (D) {  // an item of every slot maps back to it
            const uint32_t s = (uint32_t)(rnd() % (D + 1));
            uint32_t got = 0;
            const mk::AuditItem it = mk::audit_item(sh, mk::audit_slot_first(sh, s), &got);
            if (got != s || it.index != 0) die(none, "slot of a large list's item", n, s);
        }
    }
    std::fprintf(stderr, "%llu cases clean, %llu items replayed, %llu level offsets compared\n",
                 (unsigned long long)g_cases, (unsigned long long)g_items, (unsigned long long)g_offsets);
    return 0;
}
