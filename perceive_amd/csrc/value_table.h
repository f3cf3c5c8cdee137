// value_table.h — the value of an item id and the predicate over it (corpus.h, "filtered search"; DESIGN.md §4 "Item values and
// filtered search"): the one copy, for every kernel that tests a row against a predicate (where_mark_kernel, where_select_kernel) or reads its value (boost_select_kernel).
// The table is the id-keyed table of group_table.h with kNoValue as its `none`.  Everything here is inlined: the file defines no symbol.
#pragma once
#include "group_table.h"

namespace pcv {
namespace {

// Does a row whose id has value `v` (kNoValue: none) pass?  With a value: lo <= v <= hi, negated under kWhereOutside.  Without:
// kWhereUnsetPasses alone decides.  lo > hi is the empty interval.
__device__ __forceinline__ bool where_passes(int64_t v, const WherePred& w) {
    if (v == kNoValue) return (w.flags & kWhereUnsetPasses) != 0;
    const bool inside = w.lo <= v && v <= w.hi;
    return inside != ((w.flags & kWhereOutside) != 0);
}

// The value of `id`, kNoValue if it has none.
__device__ __forceinline__ int64_t value_of(const ValueTable& t, int64_t id) {
    return group_of(t.keys, t.vals, t.mask, t.side_val, id, kNoValue);
}

}  // namespace
}  // namespace pcv
