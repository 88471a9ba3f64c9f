// Host-only fuzz of the struct layout parser (prysm_amd/csrc/struct_spec.cpp),
// built with g++ -fsanitize=address,undefined by tests/test_struct_spec_fuzz.py.
// Random mk_field arrays -- well-formed nests, hostile child counts, depths,
// offsets and lengths -- in a heap buffer of exactly nfields entries, so a
// read past the array is an ASan report.  The parser must either refuse an
// array or produce a program whose every access stays inside the record, the
// LDS column and the message bounds it reports (abort on violation).
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

// a well-formed struct body of `count` entries at nesting depth `depth`
static void gen_body(std::vector<mk_field>& out, uint32_t count, uint32_t depth, uint32_t& off) {
    while (count) {
        const uint32_t k = rnd(8);
        if (k == 0 && count >= 2 && depth < kMaxStructDepth + 1) {  // sometimes one level too deep
            const uint32_t sub = 1 + rnd(count - 1);
            out.push_back(mk_field{MK_FIELD_STRUCT, 0, sub});
            gen_body(out, sub, depth + 1, off);
            count -= 1 + sub;
        } else if (k <= 2) {
            const uint32_t len = rnd(200);
            out.push_back(mk_field{MK_FIELD_VARBYTES, off, len});
            off += (4 + len + 3) & ~3u;
            --count;
        } else if (k <= 5) {
            const uint32_t len = 4 * rnd(50) + (rnd(4) ? 0 : rnd(4));
            out.push_back(mk_field{MK_FIELD_BYTES, off, len});
            off += (len + 3) & ~3u;
            --count;
        } else {
            const uint32_t len = 1u << rnd(4);
            out.push_back(mk_field{MK_FIELD_RAW, off, len});
            off += rnd(2) ? len : ((len + 3) & ~3u);
            off = rnd(3) ? ((off + 3) & ~3u) : off;
            --count;
        }
    }
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? std::atoi(argv[2]) : 1000;
    rng.seed(seed);
    int accepted = 0, nested = 0, refused = 0, lens_bad = 0;
    for (int c = 0; c < cases; ++c) {
        std::vector<mk_field> v;
        uint32_t off = 0;
        gen_body(v, 1 + rnd(rnd(4) ? 12 : 40), 1, off);
        uint32_t record_len = (off + 3) & ~3u;
        const uint32_t hostile = rnd(4);
        if (hostile == 0 && !v.empty()) {  // break one entry
            mk_field& f = v[rnd((uint32_t)v.size())];
            switch (rnd(6)) {
                case 0: f.len = rnd(2) ? 0xFFFFFFFFu : rnd(64); break;
                case 1: f.offset = rnd(2) ? 0xFFFFFFFCu : f.offset + 1 + rnd(3); break;
                case 2: f.kind = rnd(8); break;
                case 3: f.kind = MK_FIELD_STRUCT; break;
                case 4: f.kind = MK_FIELD_STRUCT, f.offset = 0, f.len = rnd(40); break;
                default: record_len = rnd(record_len + 1) & ~3u; break;
            }
        } else if (hostile == 1) {  // a pure chain of structs
            v.clear();
            const uint32_t d = 1 + rnd(7);
            for (uint32_t i = 0; i < d; ++i) v.push_back(mk_field{MK_FIELD_STRUCT, 0, d - i + rnd(2) * rnd(3)});
            v.push_back(mk_field{MK_FIELD_RAW, 0, 8});
            record_len = 8;
        }
        if (rnd(16) == 0) record_len = 0;  // a size query
        // exactly nfields entries on the heap
        const uint32_t nf = (uint32_t)v.size();
        mk_field* arr = (mk_field*)std::malloc(sizeof(mk_field) * (nf ? nf : 1));
        if (nf) std::memcpy(arr, v.data(), sizeof(mk_field) * nf);
        HostSpec hs;
        const int rc = parse_struct_spec(arr, nf, record_len, hs);
        std::free(arr);
        if (rc != MK_OK) {
            REQUIRE(rc == MK_EINVAL && last_error()[0] != 0);
            ++refused;
            continue;
        }
        ++accepted;
        REQUIRE(hs.nfields == nf && hs.rec_len == record_len && record_len % 4 == 0);
        REQUIRE(hs.top_len <= 32 * kMaxStructFields && hs.msg_len >= hs.top_len);
        uint32_t depth_seen = 0;
        (void)depth_seen;
        if (!hs.nested) {
            REQUIRE(hs.msg_len == hs.top_len);
            for (uint32_t f = 0; f < nf; ++f) {
                REQUIRE(hs.kind[f] == MK_FIELD_BYTES || hs.kind[f] == MK_FIELD_RAW);
                REQUIRE(hs.out_off[f] + (hs.kind[f] == MK_FIELD_BYTES ? 32 : hs.len[f]) <= hs.msg_len);
                if (record_len) REQUIRE((uint64_t)hs.off[f] + hs.len[f] <= record_len);
            }
            continue;
        }
        ++nested;
        const NestedSpec& ns = hs.prog;
        REQUIRE(ns.nops == nf + 1 && ns.nops <= kMaxStructFields + 1);
        REQUIRE(ns.peak % 4 == 0 && ns.peak <= kNestedMaxPeak && ns.rec_len == record_len);
        REQUIRE(ns.threads == kNestedThreadsMax || ns.threads == kNestedThreadsMin);
        REQUIRE((uint64_t)ns.threads * ns.peak <= kNestedLdsBytes);
        REQUIRE(ns.threads == kNestedThreadsMax || (uint64_t)2 * ns.threads * ns.peak > kNestedLdsBytes);
        // replay the program over a column of `peak` bytes: what is written, what a close reads
        std::vector<uint8_t> written(ns.peak, 0);
        uint64_t closed = 0;
        for (uint32_t k = 0; k < ns.nops; ++k) {
            const NestedOp& op = ns.op[k];
            uint32_t outb = 32;
            if (op.kind == kOpClose) {
                REQUIRE(op.src % 4 == 0 && (uint64_t)op.src + op.len <= ns.peak);
                for (uint32_t b = 0; b < op.len; ++b) REQUIRE(written[op.src + b]);  // a complete message
                for (uint32_t b = 0; b < op.len; ++b) written[op.src + b] = 0;       // the region is free again
                closed += op.len;
                if (k + 1 == ns.nops) {
                    REQUIRE(op.src == 0 && op.len == hs.top_len);
                    break;
                }
                REQUIRE(op.dst + 32 <= op.src);  // into an ancestor's message, below the region
            } else if (op.kind == MK_FIELD_RAW) {
                outb = op.len;
                if (record_len) REQUIRE((uint64_t)op.src + op.len <= record_len);
            } else if (op.kind == MK_FIELD_BYTES) {
                REQUIRE(op.src % 4 == 0);
                if (record_len) REQUIRE((uint64_t)op.src + op.len <= record_len);
            } else {
                REQUIRE(op.kind == MK_FIELD_VARBYTES && op.src % 4 == 0);
                if (record_len) REQUIRE((uint64_t)op.src + 4 + op.len <= record_len);
            }
            REQUIRE((uint64_t)op.dst + outb <= ns.peak);
            for (uint32_t b = 0; b < outb; ++b) {
                REQUIRE(!written[op.dst + b]);  // no field output overlaps a live one
                written[op.dst + b] = 1;
            }
        }
        REQUIRE(ns.op[ns.nops - 1].kind == kOpClose);
        bool has_struct = false;
        for (uint32_t f = 0; f < nf; ++f) has_struct |= hs.kind[f] == MK_FIELD_STRUCT;
        REQUIRE(hs.msg_len == (has_struct ? closed : hs.top_len));
        // the host check of stored lengths reads only inside the records
        if (record_len && record_len <= 4096) {
            const uint64_t n = 1 + rnd(3);
            uint8_t* recs = (uint8_t*)std::malloc(n * record_len);
            for (uint64_t b = 0; b < n * record_len; ++b) recs[b] = rnd(8) ? 0 : (uint8_t)rnd(256);
            if (check_var_lengths(hs, recs, n) != MK_OK) ++lens_bad;
            std::free(recs);
        }
    }
    std::fprintf(stderr, "%d cases clean: %d accepted (%d nested), %d refused, %d with a stored length refused\n", cases,
                 accepted, nested, refused, lens_bad);
    return 0;
}
