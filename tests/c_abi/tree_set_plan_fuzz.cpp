// Fuzz of the tree set's host side (prysm_amd/csrc/tree_set_plan.cpp, plain
// C++), built host-only with -fsanitize=address,undefined by
// tests/test_tree_set_plan_fuzz.py:  tree_set_plan_fuzz <seed> <steps>
// Seeded random sequences of update / append / assign / flush over a handful
// of trees, every plan held against a naive model kept here: the list content
// the staged indices and values produce, strictly ascending indices < n_old,
// aligned, ordered, non-overlapping staging ranges, and the climb / rebuild /
// grow decision; then the decision at exactly count / rebuild_div <= dirty and
// at capacity + 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "tree_set_plan.hpp"

using namespace mk::setplan;

namespace {

uint64_t g_state;
uint64_t rnd() {  // SplitMix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, "\n");                   \
            std::exit(1);                                 \
        }                                                 \
    } while (0)

using Row = std::vector<uint8_t>;

// the naive model of one tree
struct Model {
    uint32_t L;
    uint64_t div;
    std::vector<Row> list;      // what the caller sees
    std::vector<Row> resident;  // what the device holds
    uint64_t cap;
    std::set<uint64_t> touched;  // resident indices changed since the last flush
};

Row row(uint32_t L) {
    Row r(L);
    for (auto& b : r) b = (uint8_t)rnd();
    return r;
}

struct Set {
    std::vector<Pending> pend;
    std::vector<Model> model;
    uint64_t head;
    uint64_t nclimb = 0, nrebuild = 0, ngrow = 0;

    void add(uint32_t L, uint64_t div, uint64_t cap) {
        Pending p;
        p.item_len = L;
        p.rebuild_div = div;
        p.cap = cap;
        pend.push_back(p);
        model.push_back(Model{L, div, {}, {}, cap, {}});
    }

    void assign(size_t i, uint64_t n) {
        Model& m = model[i];
        m.list.clear();
        for (uint64_t j = 0; j < n; ++j) m.list.push_back(row(m.L));
        m.resident = m.list;
        m.cap = std::max(m.cap, n);
        m.touched.clear();
        record_assign(pend[i], n, m.cap);
    }

    void update(size_t i, const std::vector<uint64_t>& idx) {
        Model& m = model[i];
        std::vector<uint8_t> vals;
        std::vector<Row> rows;
        for (size_t j = 0; j < idx.size(); ++j) {
            rows.push_back(row(m.L));
            vals.insert(vals.end(), rows.back().begin(), rows.back().end());
        }
        bool ok = true;
        for (uint64_t x : idx) ok = ok && x < m.list.size();
        const Pending before = pend[i];
        const bool got = record_update(pend[i], idx.data(), vals.data(), idx.size());
        CHECK(got == ok, "tree %zu: update accepted %d, model %d", i, (int)got, (int)ok);
        if (!ok) {  // nothing changed
            CHECK(before.idx == pend[i].idx && before.vals == pend[i].vals && before.app == pend[i].app,
                  "tree %zu: a refused update changed the pending state", i);
            return;
        }
        for (size_t j = 0; j < idx.size(); ++j) {
            m.list[idx[j]] = rows[j];
            if (idx[j] < m.resident.size()) m.touched.insert(idx[j]);
        }
    }

    void append(size_t i, uint64_t k) {
        Model& m = model[i];
        std::vector<uint8_t> vals;
        for (uint64_t j = 0; j < k; ++j) {
            m.list.push_back(row(m.L));
            vals.insert(vals.end(), m.list.back().begin(), m.list.back().end());
        }
        record_append(pend[i], vals.data(), k);
        CHECK(pend[i].count() == m.list.size(), "tree %zu: count %llu, model %zu", i,
              (unsigned long long)pend[i].count(), m.list.size());
    }

    // plan, pack, check everything, apply to the model's device, commit; the action of tree `watch`
    Action flush(size_t watch = 0) {
        const uint32_t nt = (uint32_t)pend.size();
        SetPlan P;
        make_plan(pend.data(), nt, head, P);
        CHECK(P.tree.size() == nt && P.head == head, "plan shape");
        CHECK(P.bytes % 16 == 0 && P.bytes >= head, "plan of %llu bytes", (unsigned long long)P.bytes);
        // exact-size staging with canaries: ASan sees any write beyond it
        std::vector<uint8_t> staging(P.bytes, 0xEE);
        for (uint64_t b = 0; b < head; ++b) staging[b] = 0xC3;
        pack(pend.data(), nt, P, staging.data());
        for (uint64_t b = 0; b < head; ++b) CHECK(staging[b] == 0xC3, "pack wrote into the head at %llu", (unsigned long long)b);
        uint64_t pos = head;
        Action seen = kClimb;
        for (uint32_t i = 0; i < nt; ++i) {
            Model& m = model[i];
            const TreePlan& t = P.tree[i];
            const uint64_t n_old = m.resident.size(), n_new = m.list.size(), n_app = n_new - n_old;
            CHECK(t.n_old == n_old && t.n_new == n_new, "tree %u: n_old / n_new", i);
            CHECK(t.k_idx == m.touched.size() && t.sidx.size() == t.k_idx && t.src.size() == t.k_idx,
                  "tree %u: %llu indices, model %zu", i, (unsigned long long)t.k_idx, m.touched.size());
            for (uint64_t j = 0; j < t.k_idx; ++j) {
                CHECK(t.sidx[j] < n_old, "tree %u: index %llu >= n_old", i, (unsigned long long)t.sidx[j]);
                CHECK(j == 0 || t.sidx[j - 1] < t.sidx[j], "tree %u: indices not strictly ascending", i);
            }
            // ranges: aligned, in order, disjoint, inside the buffer
            CHECK(t.idx_off % 8 == 0 && t.val_off % 16 == 0, "tree %u: misaligned ranges", i);
            CHECK(t.idx_off >= pos, "tree %u: indices overlap what precedes them", i);
            CHECK(t.val_off >= t.idx_off + 8 * t.k_idx, "tree %u: values overlap the indices", i);
            pos = t.val_off + (t.k_idx + n_app) * m.L;
            CHECK(pos <= P.bytes, "tree %u: values leave the staging buffer", i);
            // the decision
            const uint64_t dirty = m.touched.size() + n_app;
            Action want = kClimb;
            uint64_t want_cap = m.cap;
            if (n_new > m.cap) {
                want = kGrow;
                want_cap = std::max(2 * m.cap, n_new);
            } else if (dirty && n_new / m.div <= dirty) {
                want = kRebuild;
            }
            CHECK(t.action == want, "tree %u: action %u, model %u (n_new %llu, dirty %llu, cap %llu)", i,
                  (unsigned)t.action, (unsigned)want, (unsigned long long)n_new, (unsigned long long)dirty,
                  (unsigned long long)m.cap);
            CHECK(t.new_cap == want_cap, "tree %u: new capacity", i);
            (want == kClimb ? nclimb : want == kRebuild ? nrebuild : ngrow)++;
            if (i == watch) seen = t.action;
            // the staged bytes applied the way the device applies them
            uint64_t idx_j;
            for (uint64_t j = 0; j < t.k_idx; ++j) {
                std::memcpy(&idx_j, staging.data() + t.idx_off + 8 * j, 8);
                CHECK(idx_j == t.sidx[j], "tree %u: staged index %llu", i, (unsigned long long)j);
                std::memcpy(m.resident[idx_j].data(), staging.data() + t.val_off + j * m.L, m.L);
            }
            for (uint64_t j = 0; j < n_app; ++j) {
                const uint8_t* v = staging.data() + t.val_off + (t.k_idx + j) * m.L;
                m.resident.push_back(Row(v, v + m.L));
            }
            CHECK(m.resident == m.list, "tree %u: the staged changes do not produce the list", i);
            m.cap = want_cap;
            m.touched.clear();
            commit(pend[i], t);
            CHECK(pend[i].n == n_new && pend[i].cap == want_cap && pend[i].idx.empty() && pend[i].vals.empty() &&
                      pend[i].app.empty(),
                  "tree %u: commit", i);
        }
        return seen;
    }
};

// count / div <= dirty, one below and exactly at it; capacity and capacity + 1
void thresholds() {
    const uint64_t divs[3] = {512, 32, 256};
    for (uint64_t div : divs) {
        for (uint64_t n : {uint64_t(64), uint64_t(2048), 4 * div, 4 * div + 3}) {
            const uint64_t at = n / div;  // the smallest dirty count that rebuilds (0: any change does)
            for (int mode = 0; mode < 2; ++mode) {  // distinct updates; appends (count includes them)
                for (uint64_t dirty : {at ? at - 1 : 0, at, at + 1}) {
                    if (dirty == 0) continue;
                    Set s;
                    s.head = 0;
                    s.add(8, div, 2 * n + 8);
                    s.assign(0, n);
                    if (mode == 0) {
                        std::vector<uint64_t> idx;
                        for (uint64_t j = 0; j < dirty; ++j) idx.push_back(n - 1 - j);
                        idx.push_back(n - 1);  // a repeat is not another dirty item
                        s.update(0, idx);
                        CHECK(s.flush() == (n / div <= dirty ? kRebuild : kClimb), "div %llu n %llu dirty %llu",
                              (unsigned long long)div, (unsigned long long)n, (unsigned long long)dirty);
                    } else {
                        s.append(0, dirty);
                        CHECK(s.flush() == ((n + dirty) / div <= dirty ? kRebuild : kClimb),
                              "div %llu n %llu appended %llu", (unsigned long long)div, (unsigned long long)n,
                              (unsigned long long)dirty);
                    }
                }
            }
        }
    }
    for (uint64_t cap : {uint64_t(1), uint64_t(4), uint64_t(100)}) {
        Set s;
        s.head = 24;
        s.add(5, 1ull << 40, cap);  // a share no list reaches: only the capacity decides
        s.assign(0, cap - 1);
        s.append(0, 1);  // capacity - 1 -> capacity
        CHECK(s.flush() != kGrow, "grew at the capacity %llu", (unsigned long long)cap);
        s.append(0, 1);  // -> capacity + 1
        CHECK(s.flush() == kGrow, "did not grow at capacity %llu + 1", (unsigned long long)cap);
        CHECK(s.pend[0].cap == std::max(2 * cap, cap + 1), "new capacity");
        s.append(0, 3 * cap + 5);  // more than double
        CHECK(s.flush() == kGrow && s.pend[0].cap == s.pend[0].n, "grow beyond the double");
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 1;
    const int steps = argc > 2 ? std::atoi(argv[2]) : 400;
    g_state = seed * 0x2545F4914F6CDD1Dull + 99;
    thresholds();
    uint64_t nclimb = 0, nrebuild = 0, ngrow = 0, nflush = 0;
    for (int round = 0; round < 8; ++round) {
        Set s;
        s.head = (rnd() % 3) * 40 + (rnd() % 2) * 536;
        const uint32_t lens[6] = {8, 5, 32, 33, 40, 144};
        const uint64_t divs[3] = {512, 32, 256};
        const size_t nt = 1 + rnd() % 6;
        for (size_t i = 0; i < nt; ++i) s.add(lens[rnd() % 6], divs[rnd() % 3], 1 + rnd() % 64);
        for (int step = 0; step < steps; ++step) {
            const size_t i = rnd() % nt;
            const uint64_t count = s.model[i].list.size();
            switch (rnd() % 8) {
                case 0:
                case 1:
                case 2: {  // update: any order, repeats, now and then an index beyond the list
                    std::vector<uint64_t> idx;
                    const uint64_t k = rnd() % 6;
                    const bool bad = rnd() % 16 == 0;
                    for (uint64_t j = 0; j < k && count; ++j) idx.push_back(rnd() % 4 == 0 && j ? idx[j - 1] : rnd() % count);
                    if (bad) idx.push_back(count + rnd() % 3);
                    s.update(i, idx);
                    break;
                }
                case 3:
                case 4:
                    s.append(i, rnd() % 4);
                    break;
                case 5:
                    if (rnd() % 4 == 0) s.assign(i, rnd() % 300);  // a shorter list too, changes pending
                    break;
                default:
                    s.flush();
                    ++nflush;
            }
        }
        s.flush();
        nclimb += s.nclimb;
        nrebuild += s.nrebuild;
        ngrow += s.ngrow;
    }
    std::fprintf(stderr, "%llu flushes, %llu climbs, %llu rebuilds, %llu grows: cases clean\n",
                 (unsigned long long)nflush, (unsigned long long)nclimb, (unsigned long long)nrebuild,
                 (unsigned long long)ngrow);
    return 0;
}
