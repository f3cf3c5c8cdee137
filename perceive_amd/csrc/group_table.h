// group_table.h — the probe of the group table (corpus.h; DESIGN.md §4 "Grouped results"): the one copy, for every kernel that reads
// the table at rest (group_lookup_kernel, grouped_select_kernel, row_groups_kernel).  Everything here is inlined: the file defines no symbol.
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
// The group of `id`, or -1.
__device__ __forceinline__ int64_t group_of(const int64_t* __restrict__ keys, const int64_t* __restrict__ vals, uint32_t mask,
                                            int64_t side_val, int64_t id) {
    if (id == kIdEmpty) return side_val;
    if (keys == nullptr) return -1;
    const uint32_t h = find_slot(keys, mask, id);
    return gld(&keys[h]) == id ? gld(&vals[h]) : (int64_t)-1;
}

// The 32-bit tag of a group key (row_jobs.h, PairGroups): 0 for none, equal keys give equal non-zero tags, different keys may collide.
__device__ __forceinline__ uint32_t group_tag(int64_t g) { return g < 0 ? 0u : ((uint32_t)g & 0x7fffffffu) + 1u; }

}  // namespace
}  // namespace pcv
