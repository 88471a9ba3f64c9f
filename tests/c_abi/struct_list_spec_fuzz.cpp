// Host-only fuzz of the struct layout parser's list path (prysm_amd/csrc/struct_spec.cpp, MK_FIELD_LIST), built
// with g++ -fsanitize=address,undefined by tests/test_struct_list_spec_fuzz.py.  Random mk_field arrays with list
// entries -- well-formed ones and ones with a broken entry -- in a heap buffer of exactly nfields entries.  The
// parser must refuse an array or produce a program that, replayed here step by step as k_struct_list runs it,
//   - reads no record byte outside [0, rec_len),
//   - writes no column byte outside [0, peak),
//   - keeps every list's node stack inside the levels its end op declares,
// and whose closes read only bytes that were written (abort on violation).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "planner.hpp"
#include "struct_spec.hpp"

using namespace mk;

#define REQUIRE(c)                                                                   \
    do {                                                                             \
        if (!(c)) {                                                                  \
            std::fprintf(stderr, "invariant failed at line %d: %s\n", __LINE__, #c); \
            std::abort();                                                            \
        }                                                                            \
    } while (0)

static std::mt19937_64 rng;
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

static void gen_body(std::vector<mk_field>& out, uint32_t count, uint32_t depth, uint32_t& off, bool item);

// a list entry, its descriptor and (for struct items) the item's fields; returns the entries used
static uint32_t gen_list(std::vector<mk_field>& out, uint32_t budget, uint32_t depth, uint32_t& off) {
    off = (off + 3) & ~3u;
    const uint32_t k = rnd(3);
    uint32_t cap = rnd(8) ? 1 + rnd(40) : 1 + rnd(40000), stride, used = 2;
    const size_t at = out.size();
    out.push_back(mk_field{MK_FIELD_LIST, off, cap});
    if (k == 0) {
        stride = 1u << rnd(4);
        out.push_back(mk_field{MK_FIELD_RAW, stride, stride});
    } else if (k == 1 || budget < 3) {
        const uint32_t len = 4 * rnd(50);
        stride = len + 4 * rnd(3);
        out.push_back(mk_field{MK_FIELD_BYTES, stride, len});
    } else {
        const uint32_t sub = 1 + rnd(std::min(budget - 2, 5u));
        out.push_back(mk_field{MK_FIELD_STRUCT, 0, sub});
        uint32_t ioff = 0;
        gen_body(out, sub, depth + 1, ioff, true);
        stride = ((ioff + 3) & ~3u) + 4 * rnd(2);
        out[at + 1].offset = stride;
        used += sub;
    }
    off += 4 + cap * stride;
    return used;
}

static void gen_body(std::vector<mk_field>& out, uint32_t count, uint32_t depth, uint32_t& off, bool item) {
    while (count) {
        const uint32_t k = rnd(10);
        if (k == 0 && count >= 2 && depth < kMaxStructDepth + 1) {
            const uint32_t sub = 1 + rnd(count - 1);
            out.push_back(mk_field{MK_FIELD_STRUCT, 0, sub});
            gen_body(out, sub, depth + 1, off, item);
            count -= 1 + sub;
        } else if (k <= 2 && count >= 2 && (!item || rnd(8) == 0)) {  // sometimes a list in a list item
            count -= std::min(count, gen_list(out, count, depth, off));
        } else if (k <= 4) {
            const uint32_t len = rnd(60);
            off = (off + 3) & ~3u;
            out.push_back(mk_field{MK_FIELD_VARBYTES, off, len});
            off += 4 + len;
            --count;
        } else if (k <= 6) {
            const uint32_t len = 4 * rnd(40) + (rnd(4) ? 0 : rnd(4));
            off = (off + 3) & ~3u;
            out.push_back(mk_field{MK_FIELD_BYTES, off, len});
            off += len;
            --count;
        } else {
            const uint32_t len = 1u << rnd(4);
            out.push_back(mk_field{MK_FIELD_RAW, off, len});
            off += len;
            --count;
        }
    }
}

// ---- the replay ----------------------------------------------------------------------------
struct Replay {
    const ListSpec* ls;
    std::vector<uint8_t> written;  // per column byte
    uint64_t reads = 0;
    void rd(uint64_t lo, uint64_t len) {  // record bytes [lo, lo + len)
        if (ls->rec_len) REQUIRE(lo + len <= ls->rec_len);
        ++reads;
    }
    void wr(uint64_t lo, uint64_t len) {
        REQUIRE(lo + len <= ls->peak);
        for (uint64_t b = lo; b < lo + len; ++b) written[b] = 1;
    }
    void need(uint64_t lo, uint64_t len) {  // a hash over column bytes [lo, lo + len)
        REQUIRE(lo % 4 == 0 && lo + len <= ls->peak);
        for (uint64_t b = lo; b < lo + len; ++b) REQUIRE(written[b]);
    }
};

// the end op of k_struct_list for a lane whose list holds `count` items, at item j (the caller loops j)
static void end_step(Replay& R, uint32_t count, uint32_t j, uint32_t olen, uint32_t work, uint32_t levels, uint32_t fdst,
                     bool& done) {
    const uint32_t ipc = 128 / olen, ipc2 = 2 * ipc, stk = work + kListPairBytes;
    const bool act = j < count, fin = j + 1 >= count, full = act && (j + 1) % ipc2 == 0 && !fin;
    if (!full && !fin) return;
    const uint32_t p = (fin ? (count ? count - 1 : 0) : j) / ipc2, items = fin ? (count ? (count - 1) % ipc2 + 1 : 0) : ipc2;
    uint32_t bytes = items * olen, mlen, lvl = 1, nl = p + 1;
    bool last = false;
    if (fin && count <= ipc) {
        if (count == 0) R.wr(work, 128), bytes = 128;
        R.wr(work + bytes, 32 + (bytes % 4 ? 4 - bytes % 4 : 0));  // the dword the shifted store finishes
        mlen = bytes + 32, last = true;
    } else if (items <= ipc) {
        R.wr(work + bytes, ((bytes + 3) & ~3u) - bytes + 128);
        mlen = bytes + 128;
    } else {
        mlen = bytes;
    }
    REQUIRE(mlen <= kListPairBytes);
    for (;;) {
        R.need(work, mlen);
        if (last) {
            R.wr(fdst, 32);
            break;
        } else if ((p >> (lvl - 1)) & 1u) {
            REQUIRE(lvl <= levels);
            R.need(stk + 32 * (lvl - 1), 32);
            R.wr(work, 64);
            mlen = 64, ++lvl, nl = (nl + 1) / 2;
        } else if (!fin) {
            REQUIRE(lvl <= levels);  // the stack depth fits the declared budget
            R.wr(stk + 32 * (lvl - 1), 32);
            break;
        } else if (nl == 1) {
            R.wr(work, 64);
            mlen = 64, last = true;
        } else {
            R.wr(work, 160);
            mlen = 160, ++lvl, nl = (nl + 1) / 2;
        }
    }
    if (fin) done = true;
}

static void field_op(Replay& R, const NestedOp& op, uint64_t base, uint32_t pos) {
    const uint32_t kind = op.kind & 0xFF, dst = op.dst + ((op.kind & kOpItemOut) ? pos : 0);
    if (kind == kOpClose) {
        R.need(op.src, op.len);
        R.wr(dst, 32);
    } else if (kind == MK_FIELD_RAW) {
        R.rd(base + op.src, op.len);
        R.wr(dst, op.len);
    } else if (kind == MK_FIELD_BYTES) {
        REQUIRE((base + op.src) % 4 == 0);
        R.rd(base + op.src, op.len);
        R.wr(dst, 32);
    } else {
        REQUIRE(kind == MK_FIELD_VARBYTES && (base + op.src) % 4 == 0);
        R.rd(base + op.src, 4 + (uint64_t)op.len);  // the clamped length reaches at most the slot's end
        R.wr(dst, 32);
    }
}

// one lane whose every list holds min(cap, want) items
static void replay(const HostSpec& hs, uint32_t want) {
    const ListSpec& ls = hs.lprog;
    Replay R{&ls, std::vector<uint8_t>(ls.peak, 0)};
    REQUIRE(ls.nops >= 4 && ls.nops <= kMaxListOps && ls.op[ls.nops - 1].kind == kOpClose);
    for (uint32_t k = 0; k < ls.nops;) {
        const NestedOp& op = ls.op[k];
        if (op.kind == kOpList) {
            REQUIRE(k + 3 < ls.nops && ls.op[k + 1].kind == kOpItem);
            const uint32_t cap = op.len, stride = ls.op[k + 1].src, olen = ls.op[k + 1].len, work = ls.op[k + 1].dst;
            uint32_t e = k + 2;
            while (e < ls.nops && ls.op[e].kind != kOpListEnd) {
                REQUIRE((ls.op[e].kind & 0xFF) != kOpList);  // lists do not nest
                ++e;
            }
            REQUIRE(e < ls.nops && e > k + 2 && ls.op[e].src == k && (ls.op[e - 1].kind & kOpItemOut));
            const uint32_t levels = ls.op[e].len;
            REQUIRE(cap >= 1 && (olen == 1 || olen == 2 || olen == 4 || olen == 8 || olen == 32) && work % 4 == 0);
            REQUIRE(levels <= kListMaxStack && levels == list_stack_levels((cap + 128 / olen - 1) / (128 / olen)));
            REQUIRE((uint64_t)work + kListPairBytes + 32 * levels <= ls.peak);
            REQUIRE(op.src % 4 == 0);
            R.rd(op.src, 4);
            const uint32_t count = std::min(cap, want), ipc2 = 2 * (128 / olen);
            bool done = false;
            uint32_t j = 0;
            do {
                if (j < count)
                    for (uint32_t b = k + 2; b < e; ++b)
                        field_op(R, ls.op[b], (uint64_t)op.src + 4 + (uint64_t)j * stride, (j % ipc2) * olen);
                end_step(R, count, j, olen, work, levels, op.dst, done);
                ++j;
            } while (j < count);
            REQUIRE(done);
            // the last cell the device may touch (count clamped to cap) lies in the record
            R.rd((uint64_t)op.src + 4 + (uint64_t)(cap - 1) * stride, olen == 32 ? stride : olen);
            k = e + 1;
            continue;
        }
        REQUIRE(op.kind != kOpItem && op.kind != kOpListEnd && !(op.kind & kOpItemOut));
        if (k + 1 == ls.nops) {
            REQUIRE(op.src == 0 && op.len == hs.top_len);
            R.need(0, op.len);
        } else {
            field_op(R, op, 0, 0);
        }
        ++k;
    }
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? std::atoi(argv[2]) : 1000;
    rng.seed(seed);
    int accepted = 0, refused = 0, counts_bad = 0;
    for (int c = 0; c < cases; ++c) {
        std::vector<mk_field> v;
        uint32_t off = 0;
        gen_body(v, 2 + rnd(rnd(4) ? 10 : 34), 1, off, false);
        if (rnd(3) == 0 || v.size() < 2) {  // make sure there is a list
            uint32_t o2 = off;
            gen_list(v, 6, 1, o2);
            off = o2;
        }
        uint32_t record_len = (off + 3) & ~3u;
        if (rnd(4) == 0 && !v.empty()) {  // break one entry
            mk_field& f = v[rnd((uint32_t)v.size())];
            switch (rnd(7)) {
                case 0: f.len = rnd(2) ? 0xFFFFFFFFu : rnd(64); break;
                case 1: f.offset = rnd(2) ? 0xFFFFFFFCu : f.offset + 1 + rnd(3); break;
                case 2: f.kind = rnd(9); break;
                case 3: f.kind = MK_FIELD_LIST; break;
                case 4: f.kind = MK_FIELD_LIST, f.len = rnd(2) ? 0 : 0x10000 + rnd(1 << 20); break;
                case 5: v.pop_back(); break;
                default: record_len = rnd(record_len + 1) & ~3u; break;
            }
        }
        if (rnd(16) == 0) record_len = 0;  // a size query
        const uint32_t nf = (uint32_t)v.size();
        mk_field* arr = (mk_field*)std::malloc(sizeof(mk_field) * (nf ? nf : 1));
        if (nf) std::memcpy(arr, v.data(), sizeof(mk_field) * nf);
        HostSpec* hs = new HostSpec;
        const int rc = parse_struct_layout(arr, nf, record_len, *hs);
        bool has_list = false;
        for (uint32_t f = 0; f < nf; ++f) has_list |= arr[f].kind == MK_FIELD_LIST;
        std::free(arr);
        if (rc != MK_OK) {
            REQUIRE(rc == MK_EINVAL && last_error()[0] != 0);
            ++refused;
            delete hs;
            continue;
        }
        REQUIRE((hs->lists != 0) == has_list);
        if (!hs->lists) {
            delete hs;
            continue;
        }
        ++accepted;
        const ListSpec& ls = hs->lprog;
        REQUIRE(hs->nested && hs->nfields == nf && hs->rec_len == record_len && ls.rec_len == record_len);
        REQUIRE(ls.peak % 4 == 0 && ls.peak <= kListMaxPeak);
        REQUIRE(ls.threads == 128 || ls.threads == 64);
        REQUIRE((uint64_t)ls.threads * ls.peak <= kNestedLdsBytes);
        REQUIRE(ls.threads == 128 || (uint64_t)2 * ls.threads * ls.peak > kNestedLdsBytes);
        REQUIRE(hs->ext % 4 == 0 && (!record_len || hs->ext <= record_len));
        uint32_t maxcap = 1;
        for (uint32_t k = 0; k < ls.nops; ++k)
            if (ls.op[k].kind == kOpList) maxcap = std::max(maxcap, ls.op[k].len);
        replay(*hs, 0);
        replay(*hs, maxcap);
        for (int t = 0; t < 6; ++t) replay(*hs, rnd(4) ? rnd(maxcap + 1) : rnd(std::min(maxcap, 70u) + 1));
        // the host check of stored counts and lengths reads only inside the records
        if (record_len && record_len <= 65536) {
            const uint64_t n = 1 + rnd(2);
            uint8_t* recs = (uint8_t*)std::malloc(n * record_len);
            for (uint64_t b = 0; b < n * record_len; ++b) recs[b] = rnd(6) ? 0 : (uint8_t)rnd(256);
            if (check_var_lengths(*hs, recs, n) != MK_OK) ++counts_bad;
            std::free(recs);
        }
        delete hs;
    }
    std::fprintf(stderr, "%d cases clean: %d accepted with a list, %d refused, %d with a stored count or length refused\n",
                 cases, accepted, refused, counts_bad);
    return 0;
}
