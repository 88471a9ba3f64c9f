// Parsing and validation of mk_field layouts (struct_spec.hpp).  Plain C++:
// every check here runs before a device is looked up.
#include "struct_spec.hpp"

#include <cstring>

#include "planner.hpp"

namespace mk {

#define SPEC_TRY(x)                    \
    do {                               \
        const int rc_ = (x);           \
        if (rc_ != MK_OK) return rc_;  \
    } while (0)

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
// ---- layouts with a MK_FIELD_LIST: a recursive walk that emits ListSpec ops ----
struct ListWalk {
    const mk_field* fd;
    HostSpec* hs;
    uint32_t peak;  // column bytes so far
    uint32_t sum;   // message bytes of every nested struct (and item struct) so far
    uint32_t ext;   // record bytes the program reads
};

inline uint32_t out_len(const mk_field& f) { return f.kind == MK_FIELD_RAW ? f.len : 32; }

// entries the field at f takes, itself included, inside [f, end); 0: it runs past `end`
uint32_t entry_span(const mk_field* fd, uint32_t f, uint32_t end) {
    if (fd[f].kind == MK_FIELD_STRUCT) return (uint64_t)f + 1 + fd[f].len <= end ? 1 + fd[f].len : 0;
    if (fd[f].kind == MK_FIELD_LIST) {
        if (f + 1 >= end) return 0;
        if (fd[f + 1].kind == MK_FIELD_LIST) return 2;  // refused below with its own text
        const uint32_t s = entry_span(fd, f + 1, end);
        return s ? 1 + s : 0;
    }
    return 1;
}

int emit(ListWalk& w, uint32_t kind, uint32_t src, uint32_t len, uint32_t dst) {
    ListSpec& ls = w.hs->lprog;
    if (ls.nops >= kMaxListOps) return fail(MK_EINVAL, "layout needs more than %u program steps", kMaxListOps);
    ls.op[ls.nops++] = NestedOp{kind, src, len, dst};
    return MK_OK;
}

// a RAW, BYTES or VARBYTES field whose bytes must lie in [0, limit) (limit 0: a size query)
int leaf_field(ListWalk& w, uint32_t f, uint32_t limit, bool item, uint32_t flag, uint32_t dst) {
    const mk_field& fd = w.fd[f];
    uint32_t slot = fd.len;
    if (fd.kind == MK_FIELD_RAW) {
        if (fd.len != 1 && fd.len != 2 && fd.len != 4 && fd.len != 8)
            return fail(MK_EINVAL, "raw field %u: len %u not in {1,2,4,8}", f, fd.len);
    } else if (fd.kind == MK_FIELD_BYTES) {
        if (fd.offset % 4) return fail(MK_EINVAL, "bytes field %u: offset not 4-byte aligned", f);
    } else if (fd.kind == MK_FIELD_VARBYTES) {
        if (fd.offset % 4) return fail(MK_EINVAL, "varbytes field %u: offset not 4-byte aligned", f);
        if (fd.len > 0xFFFFFFFBu) return fail(MK_EINVAL, "varbytes field %u: capacity %u", f, fd.len);
        slot = 4 + fd.len;
    } else {
        return fail(MK_EINVAL, "field %u: unknown kind %u", f, fd.kind);
    }
    if (limit && (uint64_t)fd.offset + slot > limit)
        return item ? fail(MK_EINVAL, "field %u exceeds the list item's cell", f)
                    : fail(MK_EINVAL, "field %u exceeds the record", f);
    if (!item && !limit && (uint64_t)fd.offset + slot > 0xFFFFFFF0u)
        return fail(MK_EINVAL, "field %u: offset %u out of range", f, fd.offset);
    if (!item && w.ext < align4(fd.offset + slot)) w.ext = align4(fd.offset + slot);
    return emit(w, fd.kind | flag, fd.offset, fd.len, dst);
}

// The struct whose direct children start at f0 (entries [f0, f1)), its message
// at column byte `base`.  depth: of this struct (the top-level one is 1).
// item: inside a list item (offsets count from the cell, `limit` = the stride).
int walk_struct(ListWalk& w, uint32_t f0, uint32_t f1, uint32_t depth, bool item, uint32_t limit, uint32_t base,
                uint32_t& mlen) {
    const mk_field* fd = w.fd;
    uint32_t own = 0;
    for (uint32_t f = f0; f < f1;) {  // the message length first: the children's regions lie behind it
        if (fd[f].kind == MK_FIELD_STRUCT && fd[f].len == 0) return fail(MK_EINVAL, "struct field %u has no fields", f);
        const uint32_t s = entry_span(fd, f, f1);
        if (!s && fd[f].kind == MK_FIELD_LIST && f + 1 >= f1)
            return fail(MK_EINVAL, "list field %u: no item descriptor follows", f);
        if (!s) return fail(MK_EINVAL, "field %u: its entries run past entry %u", f, f1);
        own += out_len(fd[f]);
        f += s;
    }
    mlen = own;
    const uint32_t behind = align4(base + own);
    if (w.peak < behind) w.peak = behind;
    uint32_t out = 0;
    for (uint32_t f = f0; f < f1;) {
        const mk_field& e = fd[f];
        const uint32_t dst = base + out, s = entry_span(fd, f, f1);
        w.hs->out_off[f] = out;
        if (e.kind == MK_FIELD_STRUCT) {
            if (e.offset != 0) return fail(MK_EINVAL, "struct field %u: offset %u must be 0", f, e.offset);
            if (depth == kMaxStructDepth)
                return fail(MK_EINVAL, "struct field %u nests deeper than %u", f, kMaxStructDepth);
            uint32_t sub = 0;
            SPEC_TRY(walk_struct(w, f + 1, f + 1 + e.len, depth + 1, item, limit, behind, sub));
            w.sum += sub;
            SPEC_TRY(emit(w, kOpClose, behind, sub, dst));
        } else if (e.kind == MK_FIELD_LIST) {
            const mk_field& it = fd[f + 1];
            const uint32_t cap = e.len, stride = it.offset;
            if (item) return fail(MK_EINVAL, "list field %u inside a list item", f);
            if (e.offset % 4) return fail(MK_EINVAL, "list field %u: offset not 4-byte aligned", f);
            if (cap == 0) return fail(MK_EINVAL, "list field %u: capacity 0", f);
            if (it.kind == MK_FIELD_RAW) {
                if (it.len != 1 && it.len != 2 && it.len != 4 && it.len != 8)
                    return fail(MK_EINVAL, "list field %u: raw item len %u not in {1,2,4,8}", f, it.len);
                if (stride != it.len) return fail(MK_EINVAL, "list field %u: raw items of %u bytes at stride %u", f, it.len, stride);
            } else if (it.kind == MK_FIELD_BYTES) {
                if (it.len % 4 || stride % 4 || stride < it.len || stride == 0)
                    return fail(MK_EINVAL, "list field %u: byte items of %u bytes at stride %u (both multiples of 4, stride >= len)", f,
                                it.len, stride);
            } else if (it.kind == MK_FIELD_STRUCT) {
                if (stride % 4 || stride == 0)
                    return fail(MK_EINVAL, "list field %u: struct items at stride %u (a multiple of 4)", f, stride);
                if (it.len == 0) return fail(MK_EINVAL, "list field %u: item struct has no fields", f);
                if (depth == kMaxStructDepth)
                    return fail(MK_EINVAL, "list field %u: its item struct nests deeper than %u", f, kMaxStructDepth);
            } else if (it.kind == MK_FIELD_LIST) {
                return fail(MK_EINVAL, "list field %u: its items are lists", f);
            } else {
                return fail(MK_EINVAL, "list field %u: item kind %u (raw, bytes or struct)", f, it.kind);
            }
            const uint64_t slot = 4 + (uint64_t)cap * stride;
            if (limit ? e.offset + slot > limit : e.offset + slot > 0xFFFFFFF0u)
                return fail(MK_EINVAL, "list field %u: its slot of 4 + %u x %u bytes exceeds the record", f, cap, stride);
            const uint32_t ol = out_len(it), ipc = 128 / ol;
            const uint64_t chunks = ((uint64_t)cap + ipc - 1) / ipc;
            if (chunks > kListMaxChunks)
                return fail(MK_EINVAL, "list field %u: %llu chunks of %u items (limit %u)", f, (unsigned long long)chunks,
                            ipc, kListMaxChunks);
            const uint32_t levels = list_stack_levels((uint32_t)chunks);
            const uint32_t after = behind + kListPairBytes + 32 * levels;
            if (w.peak < after) w.peak = after;
            if (w.ext < align4(e.offset + (uint32_t)slot)) w.ext = align4(e.offset + (uint32_t)slot);
            const uint32_t lk = w.hs->lprog.nops;
            SPEC_TRY(emit(w, kOpList, e.offset, cap, dst));
            SPEC_TRY(emit(w, kOpItem, stride, ol, behind));
            w.hs->out_off[f + 1] = 0;
            if (it.kind == MK_FIELD_STRUCT) {
                uint32_t sub = 0;
                SPEC_TRY(walk_struct(w, f + 2, f + 2 + it.len, depth + 1, true, stride, after, sub));
                w.sum += sub;
                SPEC_TRY(emit(w, kOpClose | kOpItemOut, after, sub, behind));
            } else {
                SPEC_TRY(emit(w, it.kind | kOpItemOut, 0, it.len, behind));
            }
            SPEC_TRY(emit(w, kOpListEnd, lk, levels, 0));
        } else {
            SPEC_TRY(leaf_field(w, f, limit, item, 0, dst));
        }
        out += out_len(e);
        f += s;
    }
    return MK_OK;
}

int parse_list_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, HostSpec& hs) {
    for (uint32_t f = 0; f < nfields; ++f) {
        hs.kind[f] = fields[f].kind;
        hs.off[f] = fields[f].offset;
        hs.len[f] = fields[f].len;
    }
    if (record_len % 4) return fail(MK_EINVAL, "record_len %u not a multiple of 4", record_len);
    ListWalk w{fields, &hs, 0, 0, 4};
    uint32_t top = 0;
    SPEC_TRY(walk_struct(w, 0, nfields, 1, false, record_len, 0, top));
    ListSpec& ls = hs.lprog;
    SPEC_TRY(emit(w, kOpClose, 0, top, 0));
    hs.nfields = nfields;
    hs.rec_len = record_len;
    hs.top_len = top;
    hs.msg_len = w.sum + top;
    hs.nested = hs.lists = 1;
    hs.ext = w.ext;
    ls.rec_len = record_len;
    ls.peak = w.peak;
    if (ls.peak > kListMaxPeak)
        return fail(MK_EINVAL,
                    "struct messages, the list's chunk pair and its node stack take %u bytes along one nesting path: "
                    "a workgroup of %u threads would need more than %u bytes of LDS (limit %u bytes per record)",
                    ls.peak, kListThreadsMin, kNestedLdsBytes, kListMaxPeak);
    ls.threads = kListThreadsMax;
    while (ls.threads * ls.peak > kNestedLdsBytes) ls.threads /= 2;
    return MK_OK;
}

inline uint32_t le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
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

int parse_struct_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, HostSpec& hs) {
    if (!fields || nfields == 0 || nfields > kMaxStructFields)
        return fail(MK_EINVAL, "nfields %u out of range (1..%u)", nfields, kMaxStructFields);
    for (uint32_t f = 0; f < nfields; ++f)
        if (fields[f].kind == MK_FIELD_LIST) {
            std::memset(&hs, 0, sizeof hs);
            return parse_list_layout(fields, nfields, record_len, hs);
        }
    return parse_struct_spec(fields, nfields, record_len, hs);
}

int check_var_lengths(const HostSpec& hs, const uint8_t* records, uint64_t n) {
    if (!hs.nested || !records) return MK_OK;
    if (hs.lists) {  // by the program: a list's count, and the stored lengths inside its first `count` items
        const ListSpec& ls = hs.lprog;
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t* r0 = records + i * hs.rec_len;
            for (uint32_t k = 0; k < ls.nops; ++k) {
                const NestedOp& op = ls.op[k];
                if (op.kind == MK_FIELD_VARBYTES && le32(r0 + op.src) > op.len)
                    return fail(MK_EINVAL, "record %llu: varbytes length %u above the slot's %u bytes",
                                (unsigned long long)i, le32(r0 + op.src), op.len);
                if (op.kind != kOpList) continue;
                const uint32_t count = le32(r0 + op.src), stride = ls.op[k + 1].src;
                if (count > op.len)
                    return fail(MK_EINVAL, "record %llu: list count %u above the slot's capacity %u",
                                (unsigned long long)i, count, op.len);
                uint32_t e = k + 2;
                for (; ls.op[e].kind != kOpListEnd; ++e) {
                    if ((ls.op[e].kind & 0xFF) != MK_FIELD_VARBYTES) continue;
                    for (uint32_t j = 0; j < count; ++j) {
                        const uint32_t L = le32(r0 + op.src + 4 + (uint64_t)j * stride + ls.op[e].src);
                        if (L > ls.op[e].len)
                            return fail(MK_EINVAL, "record %llu, list item %u: varbytes length %u above the slot's %u bytes",
                                        (unsigned long long)i, j, L, ls.op[e].len);
                    }
                }
                k = e;
            }
        }
        return MK_OK;
    }
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
