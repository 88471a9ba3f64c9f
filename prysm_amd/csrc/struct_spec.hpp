// Record layouts of the struct-hash subsystem (makeStructHasher's type
// grammar, shared/ssz/hash.go:141-178): the flat spec the struct kernels take,
// the evaluation program of k_struct_nested, and the parser that turns an
// mk_field array into both.  No HIP here: tests/c_abi/struct_spec_fuzz.cpp
// builds struct_spec.cpp with -fsanitize=address,undefined on the CPU.
#pragma once
#include <stdint.h>

#include "prysm_merkle.h"

namespace mk {

constexpr uint32_t kMaxStructFields = 32;
struct StructSpec {                 // fixed-layout record (hash.go:141-159)
    uint32_t kind[kMaxStructFields];   // 1 = bytes (hashed with le32 prefix), 2 = raw scalar
    uint32_t off[kMaxStructFields];    // byte offset inside the record
    uint32_t len[kMaxStructFields];    // field length in bytes
    uint32_t out_off[kMaxStructFields];  // byte offset inside the struct message
    uint32_t nfields, rec_len, msg_len;
};

// ---- nested structs and variable-length byte fields (k_struct_nested) ----------
constexpr uint32_t kMaxStructDepth = 4;  // the top-level struct counts as depth 1
// One thread hashes one record with its messages staged in its own LDS
// column; a workgroup of kNestedThreads[i] threads needs threads * peak bytes,
// peak = the largest sum of message lengths along one root-to-leaf path.
// LDS one workgroup asks for at most: k_struct_fused's bound (256 threads x 160 B), four workgroups per CU
constexpr uint32_t kNestedLdsBytes = 40960;
constexpr uint32_t kNestedThreadsMax = 256, kNestedThreadsMin = 128;
constexpr uint32_t kNestedMaxPeak = kNestedLdsBytes / kNestedThreadsMin;  // 320 B

// The fields in evaluation order (pre-order; a struct closes after its last
// descendant).  Column offsets are bytes from the start of the thread's column.
constexpr uint32_t kOpClose = 0;  // hash column bytes [src, src + len) -> 32 B at column byte dst
                                  // MK_FIELD_BYTES / _RAW / _VARBYTES: record bytes at src -> column byte dst
struct NestedOp {
    uint32_t kind, src, len, dst;
};
struct NestedSpec {
    NestedOp op[kMaxStructFields + 1];  // one per field entry (a struct entry's is its close) plus the top-level close
    uint32_t nops;      // the last op closes the top-level struct (its digest is the record's root)
    uint32_t rec_len;
    uint32_t peak;      // column bytes, a multiple of 4
    uint32_t threads;   // workgroup size: the largest of 256, 128 with threads * peak <= kNestedLdsBytes
};

// ---- list fields inside records (MK_FIELD_LIST, k_struct_list) ------------------
// A layout with a list field runs a longer program on a kernel of its own;
// layouts without one keep NestedSpec and k_struct_nested as they are.  The
// ops are NestedOps; src of a field op counts from the record, or inside a
// list's body from the item's cell.
//   kOpList     src = the slot's record offset, len = cap, dst = column byte of the field's 32-B hash
//   kOpItem     (right after kOpList) src = stride, len = bytes one element hash adds to a chunk
//               (the raw length, else 32), dst = column byte of the list's working region
//   ...         the body: the ops that hash one item; the last one carries kOpItemOut and
//               stores at dst + the item's place in the chunk pair
//   kOpListEnd  src = index of the kOpList op, len = stack levels
// Working region of a list: a 256-B chunk pair, then `stack levels` pending
// 32-B nodes; a struct item's message (and its nested structs') lie behind it.
constexpr uint32_t kOpList = 5, kOpItem = 6, kOpListEnd = 7;
constexpr uint32_t kOpItemOut = 0x100;  // flag on the kind of a body's last op
constexpr uint32_t kListPairBytes = 256;
constexpr uint32_t kListMaxChunks = 256;   // per list field: at most 128 level-1 nodes, 8 stack levels
constexpr uint32_t kListMaxStack = 8;
constexpr uint32_t kListThreadsMax = 128;  // the 256-B chunk pair leaves no layout that fits 256 threads
constexpr uint32_t kListThreadsMin = 64;   // one wave per workgroup: doubles the column to 640 B
constexpr uint32_t kListMaxPeak = kNestedLdsBytes / kListThreadsMin;  // 640 B
constexpr uint32_t kMaxListOps = 2 * kMaxStructFields + 2;
struct ListSpec {
    NestedOp op[kMaxListOps];
    uint32_t nops;      // the last op closes the top-level struct
    uint32_t rec_len;
    uint32_t peak;      // column bytes, a multiple of 4
    uint32_t threads;   // the largest of 128, 64 with threads * peak <= kNestedLdsBytes
};
// stack levels a list of at most `chunks` chunks needs (0: one chunk, no tree)
inline uint32_t list_stack_levels(uint32_t chunks) {
    if (chunks <= 1) return 0;
    uint32_t m = (chunks + 1) / 2, s = 0;  // level-1 nodes
    while (m) ++s, m >>= 1;
    return s;
}

// What the host keeps of a parsed layout.  The base is what the flat kernels
// take (passing a HostSpec to one of them slices it); for a layout with
// MK_FIELD_STRUCT entries msg_len is the scratch size per record: the message
// lengths of the top-level struct and of every nested struct summed.
struct HostSpec : StructSpec {
    uint32_t nested;   // has MK_FIELD_VARBYTES or MK_FIELD_STRUCT: only k_struct_nested takes it
    uint32_t top_len;  // message length of the top-level struct
    NestedSpec prog;   // valid when nested and not lists
    uint32_t lists;    // has MK_FIELD_LIST (then nested is set too): only k_struct_list takes it
    uint32_t ext;      // lists: the bytes of a record the program may read, rounded up to 4
    ListSpec lprog;    // valid when lists
};

// MK_OK, or MK_EINVAL with the detail in the error sink (planner.hpp fail()).
// record_len == 0: a size query (no bounds against the record).
// The grammar without MK_FIELD_LIST (a list entry is an unknown kind here): flat layouts and k_struct_nested's.
int parse_struct_spec(const mk_field* fields, uint32_t nfields, uint32_t record_len, HostSpec& hs);
// The whole grammar, what every entry point parses with: a layout with a MK_FIELD_LIST entry gets the list
// program (hs.lists, hs.lprog), any other layout goes to parse_struct_spec unchanged.
int parse_struct_layout(const mk_field* fields, uint32_t nfields, uint32_t record_len, HostSpec& hs);
// Host records of a nested layout: MK_EINVAL when a MK_FIELD_VARBYTES slot
// stores a length above its capacity or a MK_FIELD_LIST slot a count above its.
int check_var_lengths(const HostSpec& hs, const uint8_t* records, uint64_t n);

}  // namespace mk
