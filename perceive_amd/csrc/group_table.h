// group_table.h — the probe of an id-keyed table (corpus.h; DESIGN.md §4 "Grouped results", "Item values and filtered search"):
// the one copy, for every kernel that reads such a table at rest (group_lookup_kernel, grouped_select_kernel, row_groups_kernel; the
// value table's readers go through value_table.h).  Everything here is inlined: the file defines no symbol.
#pragma once
#include "corpus.h"
#include "device_access.h"

namespace pcv {
namespace {

// The slot that holds `id` (!= kIdEmpty), or the free slot its chain ends at: plain loads, for readers of a table at rest.
// The table is never full (slots >= 2 * entries), so the walk ends.
__device__ __forceinline__ uint32_t find_slot(const int64_t* __restrict__ keys, uint32_t mask, int64_t id) {
    uint32_t h = id_hash(id, mask);
    for (;; h = (h + 1) & mask) {
        const int64_t k = gld(&keys[h]);
        if (k == id || k == kIdEmpty) return h;
    }
}
// What the table maps `id` to, or `none` (the table's own "no value": kNoGroup for the group table, kNoValue for the value table).
__device__ __forceinline__ int64_t group_of(const int64_t* __restrict__ keys, const int64_t* __restrict__ vals, uint32_t mask,
                                            int64_t side_val, int64_t id, int64_t none) {
    if (id == kIdEmpty) return side_val;
    if (keys == nullptr) return none;
    const uint32_t h = find_slot(keys, mask, id);
    return gld(&keys[h]) == id ? gld(&vals[h]) : none;
}

// The 32-bit tag of a group key (row_jobs.h, PairGroups): 0 for none, equal keys give equal non-zero tags, different keys may collide.
__device__ __forceinline__ uint32_t group_tag(int64_t g) { return g < 0 ? 0u : ((uint32_t)g & 0x7fffffffu) + 1u; }

}  // namespace
}  // namespace pcv
