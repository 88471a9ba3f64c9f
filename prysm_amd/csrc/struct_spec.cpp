// Parsing and validation of mk_field layouts (struct_spec.hpp).  Plain C++:
// every check here runs before a device is looked up.
#include "struct_spec.hpp"

#include <cstring>

#include "planner.hpp"

namespace mk {

namespace {
inline uint32_t align4(uint32_t x) { return (x + 3) & ~3u; }

// a struct being walked: its entries are [.., end), its message grows by `out`
struct Frame {
    uint32_t entry;  // the MK_FIELD_STRUCT entry (UINT32_MAX: the top-level struct)
    uint32_t end;    // one past its last descendant
    uint32_t out;    // message bytes so far
    uint32_t base;   // column byte offset of its message (second walk)
    uint32_t dst;    // column byte offset of its digest in the parent's message (second walk)
};
}  // namespace

int parse_struct_spec(const mk_field* fields, uint32_t nfields, uint32_t record_len, HostSpec& hs) {
    if (!fields || nfields == 0 || nfields > kMaxStructFields)
        return fail(MK_EINVAL, "nfields %u out of range (1..%u)", nfields, kMaxStructFields);
    std::memset(&hs, 0, sizeof hs);
    // first walk: every check, the offsets inside the messages, each struct's message length
    uint32_t mlen[kMaxStructFields] = {};  // of the struct at entry f
    Frame stack[kMaxStructDepth];
    uint32_t depth = 1, sum = 0;
    bool has_struct = false, has_var = false;
    stack[0] = Frame{UINT32_MAX, nfields, 0, 0, 0};
    for (uint32_t f = 0; f < nfields; ++f) {
        while (depth > 1 && stack[depth - 1].end == f) {  // the struct's last descendant is behind us
            mlen[stack[depth - 1].entry] = stack[depth - 1].out;
            sum += stack[depth - 1].out;
            --depth;
        }
        const mk_field& fd = fields[f];
        Frame& cur = stack[depth - 1];
        hs.kind[f] = fd.kind;
        hs.off[f] = fd.offset;
        hs.len[f] = fd.len;
        hs.out_off[f] = cur.out;
        if (fd.kind == MK_FIELD_BYTES) {
            if (fd.offset % 4) return fail(MK_EINVAL, "bytes field %u: offset not 4-byte aligned", f);
            if (record_len && (uint64_t)fd.offset + fd.len > record_len)
                return fail(MK_EINVAL, "field %u exceeds the record", f);
            cur.out += 32;
        } else if (fd.kind == MK_FIELD_RAW) {
            if (fd.len != 1 && fd.len != 2 && fd.len != 4 && fd.len != 8)
                return fail(MK_EINVAL, "raw field %u: len %u not in {1,2,4,8}", f, fd.len);
            if (record_len && (uint64_t)fd.offset + fd.len > record_len)
                return fail(MK_EINVAL, "field %u exceeds the record", f);
            cur.out += fd.len;
        } else if (fd.kind == MK_FIELD_VARBYTES) {
            if (fd.offset % 4) return fail(MK_EINVAL, "varbytes field %u: offset not 4-byte aligned", f);
            if (record_len && (uint64_t)fd.offset + 4 + fd.len > record_len)
                return fail(MK_EINVAL, "varbytes field %u: its slot of 4 + %u bytes exceeds the record", f, fd.len);
            has_var = true;
            cur.out += 32;
        } else if (fd.kind == MK_FIELD_STRUCT) {
            if (fd.offset != 0) return fail(MK_EINVAL, "struct field %u: offset %u must be 0", f, fd.offset);
            if (fd.len == 0) return fail(MK_EINVAL, "struct field %u has no fields", f);
            if ((uint64_t)f + 1 + fd.len > cur.end)
                return fail(MK_EINVAL, "struct field %u: %u child entries run past entry %u", f, fd.len, cur.end);
            if (depth == kMaxStructDepth)
                return fail(MK_EINVAL, "struct field %u nests deeper than %u", f, kMaxStructDepth);
            has_struct = true;
            cur.out += 32;
            stack[depth++] = Frame{f, f + 1 + fd.len, 0, 0, 0};
        } else {
            return fail(MK_EINVAL, "field %u: unknown kind %u", f, fd.kind);
        }
    }
    while (depth > 1) {  // every open struct ends at nfields (its count was checked against its parent)
        mlen[stack[depth - 1].entry] = stack[depth - 1].out;
        sum += stack[depth - 1].out;
        --depth;
    }
    if (record_len % 4) return fail(MK_EINVAL, "record_len %u not a multiple of 4", record_len);
    hs.nfields = nfields;
    hs.rec_len = record_len;
    hs.top_len = stack[0].out;
    hs.msg_len = has_struct ? sum + stack[0].out : stack[0].out;
    hs.nested = (has_struct || has_var) ? 1u : 0u;
    if (!hs.nested) return MK_OK;

    // second walk: the program.  A struct's message sits in the column right
    // after its parent's whole message; once its digest is stored in the
    // parent the region is free for the next sibling.
    NestedSpec& ns = hs.prog;
    uint32_t peak = align4(hs.top_len);
    stack[0] = Frame{UINT32_MAX, nfields, 0, 0, 0};
    depth = 1;
    auto close = [&](const Frame& fr) {
        ns.op[ns.nops++] = NestedOp{kOpClose, fr.base, mlen[fr.entry], fr.dst};
    };
    for (uint32_t f = 0; f < nfields; ++f) {
        while (depth > 1 && stack[depth - 1].end == f) close(stack[--depth]);
        Frame& cur = stack[depth - 1];
        const uint32_t dst = cur.base + hs.out_off[f];
        if (hs.kind[f] == MK_FIELD_STRUCT) {
            const uint32_t own = cur.entry == UINT32_MAX ? hs.top_len : mlen[cur.entry];
            const uint32_t base = align4(cur.base + own);
            if (peak < align4(base + mlen[f])) peak = align4(base + mlen[f]);
            stack[depth++] = Frame{f, f + 1 + hs.len[f], 0, base, dst};
        } else {
            ns.op[ns.nops++] = NestedOp{hs.kind[f], hs.off[f], hs.len[f], dst};
        }
    }
    while (depth > 1) close(stack[--depth]);
    ns.op[ns.nops++] = NestedOp{kOpClose, 0, hs.top_len, 0};
    ns.rec_len = record_len;
    ns.peak = peak;
    if (peak > kNestedMaxPeak)
        return fail(MK_EINVAL,
                    "struct messages of %u bytes along one nesting path: a workgroup of %u threads would need more "
                    "than %u bytes of LDS (limit %u bytes per record)",
                    peak, kNestedThreadsMin, kNestedLdsBytes, kNestedMaxPeak);
    ns.threads = kNestedThreadsMax;
    while (ns.threads * peak > kNestedLdsBytes) ns.threads /= 2;
    return MK_OK;
}

int check_var_lengths(const HostSpec& hs, const uint8_t* records, uint64_t n) {
    if (!hs.nested || !records) return MK_OK;
    for (uint32_t f = 0; f < hs.nfields; ++f) {
        if (hs.kind[f] != MK_FIELD_VARBYTES) continue;
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t* p = records + i * hs.rec_len + hs.off[f];
            const uint32_t L = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            if (L > hs.len[f])
                return fail(MK_EINVAL, "record %llu, varbytes field %u: length %u above the slot's %u bytes",
                            (unsigned long long)i, f, L, hs.len[f]);
        }
    }
    return MK_OK;
}

}  // namespace mk
