// The changes of a tree set collected on the host and the plan of its flush
// (tree_set_plan.hpp).  No HIP in this file.
#include "tree_set_plan.hpp"

#include <algorithm>
#include <cstring>

namespace mk::setplan {

bool record_update(Pending& p, const uint64_t* idx, const uint8_t* values, uint64_t k) {
    const uint64_t count = p.count();
    for (uint64_t j = 0; j < k; ++j)
        if (idx[j] >= count) return false;
    const uint32_t L = p.item_len;
    for (uint64_t j = 0; j < k; ++j) {
        const uint8_t* v = values + j * L;
        if (idx[j] >= p.n) {  // a pending append: changed in place
            std::memcpy(p.app.data() + (idx[j] - p.n) * L, v, L);
        } else {
            p.idx.push_back(idx[j]);
            p.vals.insert(p.vals.end(), v, v + L);
        }
    }
    return true;
}

void record_append(Pending& p, const uint8_t* values, uint64_t k) {
    p.app.insert(p.app.end(), values, values + k * p.item_len);
}

void record_assign(Pending& p, uint64_t n, uint64_t cap) {
    p.n = n;
    p.cap = cap;
    p.idx.clear();
    p.vals.clear();
    p.app.clear();
}

void make_plan(const Pending* trees, uint32_t ntrees, uint64_t head, SetPlan& plan) {
    plan.tree.assign(ntrees, TreePlan{});
    plan.head = head;
    uint64_t pos = head;
    for (uint32_t i = 0; i < ntrees; ++i) {
        const Pending& p = trees[i];
        TreePlan& t = plan.tree[i];
        // ascending indices, of a repeated one the last value (the log is in call order)
        const uint64_t m = p.idx.size();
        std::vector<uint64_t> order(m);
        for (uint64_t j = 0; j < m; ++j) order[j] = j;
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return p.idx[a] < p.idx[b]; });
        for (uint64_t j = 0; j < m; ++j) {
            if (j + 1 < m && p.idx[order[j + 1]] == p.idx[order[j]]) continue;
            t.sidx.push_back(p.idx[order[j]]);
            t.src.push_back(order[j]);
        }
        t.k_idx = t.sidx.size();
        t.n_old = p.n;
        t.n_new = p.count();
        const uint64_t dirty = t.k_idx + p.n_app();
        t.new_cap = p.cap;
        if (t.n_new > p.cap) {
            t.action = kGrow;
            t.new_cap = std::max(2 * p.cap, t.n_new);
        } else if (dirty && t.n_new / p.rebuild_div <= dirty) {
            t.action = kRebuild;
        }
        pos = (pos + 7) & ~7ull;
        t.idx_off = pos;
        pos += 8 * t.k_idx;
        pos = (pos + 15) & ~15ull;
        t.val_off = pos;
        pos += dirty * p.item_len;
    }
    plan.bytes = (pos + 15) & ~15ull;
}

void pack(const Pending* trees, uint32_t ntrees, const SetPlan& plan, uint8_t* staging) {
    for (uint32_t i = 0; i < ntrees; ++i) {
        const Pending& p = trees[i];
        const TreePlan& t = plan.tree[i];
        const uint32_t L = p.item_len;
        if (t.k_idx) std::memcpy(staging + t.idx_off, t.sidx.data(), 8 * t.k_idx);
        uint8_t* v = staging + t.val_off;
        for (uint64_t j = 0; j < t.k_idx; ++j) std::memcpy(v + j * L, p.vals.data() + t.src[j] * L, L);
        if (!p.app.empty()) std::memcpy(v + t.k_idx * L, p.app.data(), p.app.size());
    }
}

void commit(Pending& p, const TreePlan& t) { record_assign(p, t.n_new, t.new_cap); }

}  // namespace mk::setplan
