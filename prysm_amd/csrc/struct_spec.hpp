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

// What the host keeps of a parsed layout.  The base is what the flat kernels
// take (passing a HostSpec to one of them slices it); for a layout with
// MK_FIELD_STRUCT entries msg_len is the scratch size per record: the message
// lengths of the top-level struct and of every nested struct summed.
struct HostSpec : StructSpec {
    uint32_t nested;   // has MK_FIELD_VARBYTES or MK_FIELD_STRUCT: only k_struct_nested takes it
    uint32_t top_len;  // message length of the top-level struct
    NestedSpec prog;   // valid when nested
};

// MK_OK, or MK_EINVAL with the detail in the error sink (planner.hpp fail()).
// record_len == 0: a size query (no bounds against the record).
int parse_struct_spec(const mk_field* fields, uint32_t nfields, uint32_t record_len, HostSpec& hs);
// Host records of a nested layout: MK_EINVAL when a MK_FIELD_VARBYTES slot
// stores a length above its capacity.
int check_var_lengths(const HostSpec& hs, const uint8_t* records, uint64_t n);

}  // namespace mk
