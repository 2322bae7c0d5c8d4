// lpt_state.hpp -- the longest-tiles-first task order of a context, host half:
// which key its tile costs were counted for, whether they are still on the
// device, the task list built from them -- and the pure decision where a
// render's costs come from (lpt_source).  Host only, no HIP call: capi_lpt.cpp
// does the device work of each source and reports back through the transitions.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../../include/rtw.h"

namespace rtw {

// What a set of tile costs was counted for: the task order of the renders of
// the same key follows them.
struct LptKey {
    rtw_camera cam;
    uint64_t scene_serial;
    uint32_t rank, nranks, prec;      // prec: sizeof of the precision
    uint64_t split;                   // the split's id (0 = the round robin)
    bool operator==(const LptKey& o) const {
        return scene_serial == o.scene_serial && rank == o.rank && nranks == o.nranks && prec == o.prec &&
               split == o.split && memcmp(&cam, &o.cam, sizeof cam) == 0;
    }
};

struct LptState {
    bool valid = false;               // h_cost holds the costs of `key`
    bool pending = false;             // ... they are still on the device: counted by the render before
    LptKey key{};
    std::vector<uint32_t> h_cost;
    bool tab_valid = false;           // h_tasks is the task list of (h_cost, tab_*)
    uint32_t tab_chunks = 0, tab_group = 0;
    uint64_t tab_target = 0;
    uint32_t tab_cull = 0;            // the tile flags it leaves out (CullState::serial; 0: none)
    std::vector<uint32_t> h_tasks;

    // the context holds (or has pending) tile costs of this key
    bool has(const LptKey& k) const { return (valid || pending) && key == k; }

    // no costs, no task list (a new key is about to be counted)
    void invalidate() { valid = pending = tab_valid = false; }
    // h_cost was filled for k (a dealt split's costs, a pilot's counts)
    void adopt(const LptKey& k) {
        invalidate();
        valid = true;
        key = k;
    }
    // a counting render of k was launched: its counts are read back by the next render of k
    void counted(const LptKey& k) {
        key = k;
        pending = true;
    }
    // the pending counts were read into h_cost (ok), or the read-back failed: the next render recounts
    void read_back(bool ok) {
        pending = false;
        if (ok) valid = true;
    }

    // the task list is not the one of (h_cost, n_chunks, group, target, the culled tiles left out)
    bool table_stale(uint32_t n_chunks, uint32_t group, uint64_t target, uint32_t cull = 0) const {
        return !tab_valid || tab_chunks != n_chunks || tab_group != group || tab_target != target || tab_cull != cull;
    }
    void table_built(uint32_t n_chunks, uint32_t group, uint64_t target, uint32_t cull = 0) {
        tab_valid = true;
        tab_chunks = n_chunks;
        tab_group = group;
        tab_target = target;
        tab_cull = cull;
    }
};

// Where the tile costs of a render of `key` come from.
enum LptSource : int {
    kSplitCosts,    // a new key under a split dealt by costs: those costs, no counting
    kCountInline,   // a new key: this render counts on the way, in the plain tile order
    kPilot,         // a new key, inline counting off: a pilot render first
    kReadBack,      // the render before counted them: read back (waits for it, once per key)
    kCached,        // h_cost
};
inline LptSource lpt_source(const LptState& s, const LptKey& key, bool split_has_costs, bool lpt_inline) {
    if (s.has(key)) return s.pending ? kReadBack : kCached;
    return split_has_costs ? kSplitCosts : lpt_inline ? kCountInline : kPilot;
}

}  // namespace rtw
