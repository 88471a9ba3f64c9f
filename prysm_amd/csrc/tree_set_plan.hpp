// The host side of a tree set (mk_tree_set, tree_set_api.cpp) that needs no
// device: the changes collected per tree and the plan of a flush -- what is
// uploaded where, and what each tree does with it.  Plain C++ (no HIP): also
// built host-only with ASan/UBSan by tests/c_abi/tree_set_plan_fuzz.cpp.
#pragma once
#include <cstdint>
#include <vector>

namespace mk::setplan {

// The pending changes of one tree.  `n` items are resident on the device; the
// list the caller sees is those with `idx` / `vals` applied in sequence (a log:
// any order, repeats allowed), then the `app` appended values.
struct Pending {
    uint32_t item_len = 0;
    uint64_t rebuild_div = 1;  // the kind's: rebuild instead of climbing when count / rebuild_div <= dirty
    uint64_t n = 0, cap = 0;   // resident items, capacity
    std::vector<uint64_t> idx;
    std::vector<uint8_t> vals;  // idx.size() x item_len
    std::vector<uint8_t> app;   // appended values

    uint64_t n_app() const { return app.size() / item_len; }
    uint64_t count() const { return n + n_app(); }  // pending appends included
};

// list[idx[j]] = values[j] in sequence.  False, and nothing changes, if an
// index is >= count(); an index inside the pending appends changes that
// pending value.
bool record_update(Pending& p, const uint64_t* idx, const uint8_t* values, uint64_t k);
void record_append(Pending& p, const uint8_t* values, uint64_t k);
// the list was replaced by n items through the build entry: nothing pending
void record_assign(Pending& p, uint64_t n, uint64_t cap);

enum Action : uint32_t {
    kClimb = 0,    // the multi-tree update climbs from the staged indices and values
    kRebuild = 1,  // dirty from the kind's rebuild_div share: write-through, then the build
    kGrow = 2,     // outgrew its capacity: double it, move the items, write-through, build
};

struct TreePlan {
    Action action = kClimb;
    uint64_t n_old = 0, n_new = 0;
    uint64_t k_idx = 0;          // strictly ascending indices < n_old, the last value of a repeated one
    uint64_t new_cap = 0;        // kGrow: max(2 * cap, n_new); else cap
    uint64_t idx_off = 0;        // staging offset of the k_idx indices (8-B aligned)
    uint64_t val_off = 0;        // staging offset of the k_idx values, then the appended ones (16-B aligned)
    std::vector<uint64_t> sidx;  // the indices
    std::vector<uint64_t> src;   // position in Pending::idx of the value of sidx[j]
};

struct SetPlan {
    std::vector<TreePlan> tree;
    uint64_t head = 0;   // bytes at offset 0 kept for the caller (the container message)
    uint64_t bytes = 0;  // the whole staging buffer
};

// The plan of a flush; `head` bytes at the front of the staging buffer stay the caller's.
void make_plan(const Pending* trees, uint32_t ntrees, uint64_t head, SetPlan& plan);
// every tree's indices and values into the staging buffer (plan.bytes; gaps are not written)
void pack(const Pending* trees, uint32_t ntrees, const SetPlan& plan, uint8_t* staging);
// the flush has run: tree i holds n_new items (capacity new_cap), nothing pending
void commit(Pending& p, const TreePlan& t);

}  // namespace mk::setplan
