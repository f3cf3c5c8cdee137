// corpus.h — launcher interface of the kernels that build and maintain a corpus segment (corpus_kernels.hip): staging, row
// scales, the screening and mid copies of scan.h, and hiding, updating, removing, viewing and gathering stored items by id — and of the
// id-keyed tables (grouped_kernels.hip), which share the id hash, and the predicate kernels over the value table (where_kernels.hip)
// and the boosted select step that reads it (boost_kernels.hip), and of the select step of compound queries (compound_kernels.hip).
#pragma once
#include "scan.h"

namespace pcv {

// ---- launchers (corpus_kernels.hip); they throw pcv::Error on a bad shape or a failed HIP call ----
void launch_pack_rows(hipStream_t st, const float* rows_rowmajor, int64_t n, int D, int D4, float4* blk, uint32_t row0);
void launch_iota_ids(hipStream_t st, int64_t* ids, int64_t first, int64_t n);
// scales of the rows in blocks [first_block, nblocks) of a segment
void launch_row_scales(hipStream_t st, const float4* blk, uint32_t first_block, uint32_t nblocks, uint32_t nrows, int D4,
                       int metric, float* scale, uint32_t* max_norm_bits);
// screening copy of the rows in blocks [first_block, nblocks): bf16(row * scale), zeros where scale == 0
void launch_coarse_pack(hipStream_t st, const float4* blk, const float* scale, uint4* blk16, uint32_t first_block, uint32_t nblocks,
                        int D4);
// int8 screening copy + quantisation scales of the rows in blocks [first_block, nblocks)
void launch_coarse_pack8(hipStream_t st, const float4* blk, const float* scale, uint4* blk8, float* scale8, uint32_t first_block,
                         uint32_t nblocks, int D4);
// the 6-bit copy (scale6 included) of blocks [first_block, nblocks) / of blocks[0..n), from the int8 copy and the f32 rows
void launch_pack6(hipStream_t st, const float4* blk, const float* scale, const uint4* blk8, const float* scale8, uint4* blk6, float4* scale6,
                  uint32_t first_block, uint32_t nblocks, int D4);
void launch_repack6_blocks(hipStream_t st, const float4* blk, const float* scale, const uint4* blk8, const float* scale8, const uint32_t* blocks,
                           uint32_t n, uint4* blk6, float4* scale6, int D4);
size_t six_copy_bytes(uint32_t nblocks, int Dp);  // bytes of blk6 for that many blocks
// mid copy + its scales of rows [first_row, nrows) of a segment
// (scale8: the quantisation scales of the segment's int8 copy if it covers these rows — the copy is then made block by block with
// the blocks' scales — or nullptr: row by row, each with its own)
void launch_mid_pack(hipStream_t st, const float4* blk, const float* scale, const float* scale8, uint4* mid16, float* scale16,
                     uint32_t first_row, uint32_t nrows, int D4);
// ---- hidden items (pcv_searcher_hide_ids) ----
// A batch of ids is looked up in an open-addressed table: capacity a power of two (mask = capacity - 1), linear probing from
// id_hash, kIdEmpty in free slots; a batch that holds kIdEmpty itself says so with has_empty instead of storing it.
constexpr int64_t kIdEmpty = INT64_MIN;
__host__ __device__ static inline uint32_t id_hash(int64_t id, uint32_t mask) {
    return (uint32_t)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}
// rows [row0, row1) of a segment whose id is in the table -> out_rows (the first `cap`), their number -> *out_n (zeroed here)
void launch_match_ids(hipStream_t st, const int64_t* ids, uint32_t row0, uint32_t row1, const int64_t* table, uint32_t tmask,
                      bool has_empty, uint32_t* out_rows, uint32_t* out_n, uint32_t cap);
// rows[0..n) become not searchable: scale 0, zeros in the screening copy (rows < copied_rows), mid scale NaN (rows < mid_rows)
void launch_hide_rows(hipStream_t st, const uint32_t* rows, uint32_t n, float* scale, uint4* blk8, uint4* blk16, uint32_t copied_rows,
                      float* scale16, uint32_t mid_rows, int D4);
// rows[0..n) searchable again: their scales as launch_row_scales computes them
void launch_restore_scales(hipStream_t st, const float4* blk, const uint32_t* rows, uint32_t n, int D4, int metric, float* scale);
// ... the int8 copy of blocks[0..n), whole blocks (new block scales)
void launch_repack8_blocks(hipStream_t st, const float4* blk, const float* scale, const uint32_t* blocks, uint32_t n, uint4* blk8,
                           float* scale8, int D4);
// ... the bf16 copy of rows[0..n)
void launch_repack16_rows(hipStream_t st, const float4* blk, const float* scale, const uint32_t* rows, uint32_t n, uint4* blk16, int D4);
// ... the mid copy: items are blocks (scale8 != nullptr: every row of each, with the block's scale) or rows; rows >= mid_rows skipped
void launch_repack_mid(hipStream_t st, const float4* blk, const float* scale, const float* scale8, const uint32_t* items, uint32_t n,
                       uint32_t mid_rows, uint4* mid16, float* scale16, int D4);
// ---- the id-keyed tables (pcv_searcher_set_groups, pcv_searcher_set_values; grouped_kernels.hip; DESIGN.md §4 "Grouped results",
// "Item values and filtered search") ----
// Item id -> int64, resident on the device: keys[slots] and vals[slots] (int64 each), slots a power of two, linear probing from
// id_hash, kIdEmpty in free slots.  The id kIdEmpty has no slot: its value lives in the head block, beside the two counters.
// One table type, two instances: what `none` is — the value that says "an entry and nothing else" — is a parameter of the table.
constexpr int64_t kNoGroup = -1;         // the group table's (PCV_NO_GROUP)
constexpr int64_t kNoValue = INT64_MIN;  // the value table's (PCV_NO_VALUE)
struct GroupHead {
    int64_t entries;        // ids that have an entry (the side slot included)
    int64_t ids;            // ... and a value other than `none`
    int64_t side_val;       // the value of id kIdEmpty (`none`: none)
    uint32_t side_claim;    // its word of `claim`
    uint32_t side_present;  // 1: id kIdEmpty has an entry
};
constexpr uint32_t kGroupSideSlot = 0xffffffffu;  // slot_of[] of id kIdEmpty
constexpr uint32_t kGroupBatch = 1u << 22;        // most ids of one upsert or lookup launch (the host feeds a longer batch in order)
// every slot free, every value `none`
void launch_group_fill(hipStream_t st, int64_t* keys, int64_t* vals, uint64_t slots, int64_t none);
// Upsert of (ids[i], groups[i]), i < n <= kGroupBatch: of an id that occurs more than once the LAST occurrence is stored, whatever
// order the atomics land in.  claim[slots] is all 0 before and after; slot_of[n] is scratch.  The table must have n free slots
// and stay half empty.  head->ids counts the transitions none -> set and set -> none.
void launch_group_upsert(hipStream_t st, int64_t* keys, int64_t* vals, uint32_t mask, uint32_t* claim, GroupHead* head, const int64_t* ids,
                         const int64_t* groups, uint32_t n, uint32_t* slot_of, int64_t none);
// every entry of an old table into a new one (launch_group_fill'ed, at least as large)
void launch_group_rehash(hipStream_t st, const int64_t* old_keys, const int64_t* old_vals, uint64_t old_slots, int64_t* keys, int64_t* vals,
                         uint32_t mask);
// out[i] = what the table holds for ids[i], `none` if nothing (keys == nullptr: a table without slots)
void launch_group_lookup(hipStream_t st, const int64_t* keys, const int64_t* vals, uint32_t mask, const GroupHead* head, const int64_t* ids,
                         uint32_t n, int64_t* out, int64_t none);
// ---- updated items (pcv_searcher_update_rows) ----
// launch_match_ids whose table also carries each id's slot in the batch (vals[h]; empty_slot for kIdEmpty): rows [row0, row1) of
// a segment whose id is in the batch -> (out_rows[i], out_slots[i]) for the first `cap`, their number -> *out_n (zeroed here)
void launch_match_id_slots(hipStream_t st, const int64_t* ids, uint32_t row0, uint32_t row1, const int64_t* table, const uint32_t* vals,
                           uint32_t tmask, bool has_empty, uint32_t empty_slot, uint32_t* out_rows, uint32_t* out_slots,
                           uint32_t* out_n, uint32_t cap);
// rows[i] of a segment takes staged row (slots[i] & 0x7fffffff) - slot0 of `stage` ([.][D] f32) and its scale as launch_row_scales
// computes it (max_norm_bits raised likewise); bit 31 of slots[i]: the row's id is hidden, its scale is 0
void launch_update_rows(hipStream_t st, const float* stage, uint32_t slot0, const uint32_t* rows, const uint32_t* slots, uint32_t n,
                        int D, int D4, int metric, float4* blk, float* scale, uint32_t* max_norm_bits);
// ---- views (pcv_searcher_create_view) ----
// Selection of the rows of a segment whose id is in the table, in row order: scratch flags4[view_tiles(nrows) * 256] and
// tile_cnt[view_tiles(nrows)]; launch_view_select leaves the tiles' offsets in tile_cnt and the number of rows in *total, then
// launch_view_compact writes the rows, ascending, to sel[0..*total).
// `invert`: the rows whose id is NOT in the table are selected (pcv_searcher_remove_ids: the rows that stay).  `off0`: flags4 and
// tile_off point at a later tile of the segment; rows are then numbered from that tile's first row and written from
// sel[tile_off[tile] - off0] on.
constexpr int kViewTile = 1024;  // rows per tile
uint32_t view_tiles(uint32_t nrows);
void launch_view_select(hipStream_t st, const int64_t* ids, uint32_t nrows, const int64_t* table, uint32_t tmask, bool has_empty,
                        uint32_t* flags4, uint32_t* tile_cnt, uint32_t* total, bool invert = false);
void launch_view_compact(hipStream_t st, const uint32_t* flags4, const uint32_t* tile_off, uint32_t nrows, uint32_t* sel,
                         uint32_t off0 = 0);
// the second half of launch_view_select alone: tile_cnt[0..ntiles) -> exclusive prefix sums in place, their sum -> *total
void launch_view_scan(hipStream_t st, uint32_t* tile_cnt, uint32_t ntiles, uint32_t* total);
// ---- filtered search (pcv_searcher_count_where / _search_where / _create_view_where; where_kernels.hip; DESIGN.md §4 "Item
// values and filtered search") ----
// The value table as its readers get it (keys == nullptr: a table without slots — no id has a value but, maybe, kIdEmpty), and
// a predicate over the value of a row's id (value_table.h: where_passes).
struct ValueTable {
    const int64_t* keys;
    const int64_t* vals;
    uint32_t mask;
    int64_t side_val;  // the value of id kIdEmpty, which has no slot (kNoValue: none)
};
struct WherePred {
    int64_t lo, hi;
    uint32_t flags;  // kWhere*
};
constexpr uint32_t kWhereUnsetPasses = 1u, kWhereOutside = 2u;  // PCV_WHERE_*
// Rows of a segment that pass: launch_view_select's first launch with the predicate in place of the id batch — the same flags4 /
// tile_cnt pair, so launch_view_scan and launch_view_compact follow unchanged — and tile_live[tile] = the flagged rows of the tile
// with scale != 0.  A row's id is ids ? ids[row] : id0 + row.  Reads the table, writes nothing to it.
void launch_where_mark(hipStream_t st, const int64_t* ids, int64_t id0, const float* scale, uint32_t nrows, const ValueTable& t,
                       const WherePred& w, uint32_t* flags4, uint32_t* tile_cnt, uint32_t* tile_live);
// acc[0] += sum of tile_cnt[0..ntiles), acc[1] += sum of tile_live[0..ntiles): integer adds, one workgroup
void launch_where_sum(hipStream_t st, const uint32_t* tile_cnt, const uint32_t* tile_live, uint32_t ntiles, int64_t* acc);
// The select step of pcv_searcher_search_where: the walk of search_grouped (scan.h, DistinctRec) with the predicate as the test —
// a hit is kept iff the value of its id passes.
struct WhereArgs {
    DistinctRec* rec;        // [B]
    DistinctRec* rec_host;   // [B] pinned host mirror, written after every pass
    pcv_hit_dev* kept;       // [B][kMaxK] the kept rows, best first, as the pass listed them
    int64_t* kept_value;     // [B][kMaxK] their values (kNoValue: an unset row that passed)
    ValueTable table;
    WherePred where;
    int num_results;
};
void launch_where_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const WhereArgs& a);
// ---- boosted results (pcv_searcher_search_boosted; boost_kernels.hip; DESIGN.md §4 "Boosted results") ----
// The select step: the same walk and record (scan.h, DistinctRec), but every pass's hits are re-ranked with the rows kept so far
// under m = fl(rel + boost(value)), ties -> lower rank.  kDistinctFull: the certificate holds; kDistinctEnd: the list ended.
// The knots are read with constant indices only (by value: nothing in it is indexed at run time).
struct BoostArgs {
    DistinctRec* rec;        // [B]
    DistinctRec* rec_host;   // [B] pinned host mirror, written after every pass
    pcv_hit_dev* kept;       // [B][kMaxK] the kept rows, best first in the boosted order
    double* kept_m;          // [B][kMaxK] their boosted scores
    int64_t* kept_value;     // [B][kMaxK] their values (kNoValue: an unset row)
    int32_t* kept_rank;      // [B][kMaxK] their ranks in the list
    ValueTable table;
    pcv_boost boost;
    double b_max;            // max over the knot boosts and unset_boost
    int num_results;
};
void launch_boost_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const BoostArgs& a);
// ---- compound queries (pcv_searcher_search_compound; compound_kernels.hip; DESIGN.md §4 "Compound queries") ----
// The select step: the wanted vectors of a compound are adjacent queries of the pass, walked in lockstep; after each pass the hits
// of all its lists are candidates, each scored under every vector of the compound, merged with the kept rows under
// m = fl(base - pen), ties -> lower position.  Every part query's record carries the compound's kept, examined and flags and its own
// last hit.  kDistinctFull: the certificate holds; kDistinctEnd: a list ended.
constexpr int kMaxCompoundParts = PCV_MAX_COMPOUND_PARTS;
struct CompoundDesc {
    int32_t first_query;  // of the pass: the compound's first wanted vector; the others follow it
    int32_t n_want;       // 1 .. kMaxCompoundParts
    int32_t first_avoid;  // row of CompoundArgs::avoid
    int32_t n_avoid;      // 0 .. kMaxCompoundParts
};
struct CompoundArgs {
    DistinctRec* rec;            // [B] one per part query
    DistinctRec* rec_host;       // [B] pinned host mirror, written after every pass
    const CompoundDesc* desc;    // [n_compounds] of the group (device)
    const double* want_norm;     // [B] canonical |q|^2 of the pass's queries
    const float* avoid;          // [.][Dp] the call's avoided vectors, zero padded
    const double* avoid_norm;    // [.] their canonical |q|^2
    pcv_hit_dev* kept;           // [n_compounds][kMaxK] the kept rows, best first; score: m
    double* kept_pen;            // [n_compounds][kMaxK] their penalties
    double* kept_part;           // [n_compounds][kMaxK][kMaxCompoundParts] their canonical scores under each wanted vector
    int n_compounds;
    int max_want;                // the largest n_want of the group: the workgroup has kMaxK threads for each
    int max_vectors;             // the largest n_want + n_avoid of the group: what the LDS staging is sized for
    int num_results;
    int mode;                    // PCV_COMPOUND_*
    double lambda;
};
void launch_compound_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const CompoundArgs& a);
// rows [dst_row0, dst_row0 + n_sel) of a view segment take rows sel[0..n_sel) of a parent segment (pieces, scale, id; parent
// position pos0 + row -> dst_ppos[row of the view segment], unless dst_ppos is nullptr); rows [dst_row0 + n_sel, dst_end) become
// padding
void launch_view_gather(hipStream_t st, const float4* src_blk, const float* src_scale, const int64_t* src_ids, int64_t src_id0,
                        int64_t src_pos0, const uint32_t* sel, uint32_t n_sel, int D4, uint32_t dst_row0, uint32_t dst_end,
                        float4* dst_blk, float* dst_scale, int64_t* dst_ids, int64_t* dst_ppos);
// ---- removed items (pcv_searcher_remove_ids) ----
// rows [dst_row0, dst_end) of a segment take the rows at the same place inside their blocks of a bounce buffer whose block 0
// stands for block dst_row0 / 32 (pieces, scale, id): the second launch of a compaction chunk, after launch_view_gather filled
// the bounce buffer with dst_row0 % 32 as its first row
void launch_compact_store(hipStream_t st, const float4* bounce_blk, const float* bounce_scale, const int64_t* bounce_ids, int D4,
                          uint32_t dst_row0, uint32_t dst_end, float4* dst_blk, float* dst_scale, int64_t* dst_ids);
// hits[0..n): pos in [0, nrows) -> ppos[pos]
void launch_view_remap(hipStream_t st, pcv_hit_dev* hits, int64_t n, const int64_t* ppos, int64_t nrows);
void launch_synth_fill(hipStream_t st, float4* blk, uint32_t nrows, uint32_t row0, int D, int D4, uint64_t seed,
                       int64_t first_row, int normalize, uint32_t n_clusters, float noise, float amp_lo = 0.0f, float amp_hi = 0.0f);
void launch_gather_rows(hipStream_t st, const SegDesc* d_segs, int nseg, const int64_t* d_pos, int64_t n, int D,
                        int D4, float* out_rows, int64_t* out_ids);
// ---- search by example (pcv_searcher_like_queries) ----
// One stored row that goes into a query vector, with its weight: row `row` of segs[seg].
struct LikeMember {
    uint32_t seg, row;
    float w;
};
// out[q][0..D) (row-major f32, device) = sum over members[first[q] .. first[q + 1]) of w * row, accumulated per component with one
// f32 fused multiply-add per member, in list order (first: [n_queries + 1], ascending from 0).  Same input, same bits.
void launch_like_queries(hipStream_t st, const SegDesc* d_segs, int nseg, const LikeMember* d_members, const uint32_t* d_first,
                         int n_queries, int D, int D4, float* out);

}  // namespace pcv
