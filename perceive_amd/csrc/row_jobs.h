// row_jobs.h — the calls that run kernels over the stored rows themselves, not over a scan's candidates (duplicate pairs, item labels,
// neighbours, matches, density clusters, the linkage tree, the reach tree, seeds, moments, projection): the arguments of their kernels and their launchers.
// The host side is row_jobs.cpp; a scan pass needs nothing of this file.
#pragma once
#include "scan.h"

namespace pcv {

// Duplicate pairs (pcv_searcher_find_duplicates; DESIGN.md §4 "Duplicate pairs"): rows against rows.  Rows are named by their
// number in the launch's block numbering, block * 32 + row of the block ("launch row": the rows behind a segment's last row in its
// last block have numbers too and take no part); launch rows ascend with the global position.
//   rinv[launch row] : 1/|x| rounded to f32 from the row's canonical |x|^2;  0: the row takes no part (unsearchable, behind nrows,
//                      no cosine);  kRinvWild: it takes part but |x| is outside [2^-20, 2^20], where the f32 screening score is
//                      not certified — every pair with such a row is a candidate and the f64 step decides
//   norm[launch row] : the canonical |x|^2 (f64, feature order)
struct DupPair {
    double c;            // canonical cosine
    int64_t pos_a, pos_b;  // global positions, pos_a < pos_b
    int64_t id_a, id_b;
};
constexpr float kRinvWild = -1.0f;
struct SelfJoinArgs {
    float* rinv;                    // [(total_blocks + tile_blocks) * 32], zero behind total_blocks * 32
    double* norm;                   // [total_blocks * 32]
    uint64_t* cand;                 // [cand_cap] (launch row a << 32) | launch row b, a < b
    unsigned long long* counters;   // [0]: candidates the screen found (not capped), [1]: duplicate pairs (not capped)
    DupPair* pairs;                 // [pair_cap]
    unsigned long long cand_cap, pair_cap, n_cand;  // n_cand: entries of `cand` the rescore step reads
    float screen_threshold;         // threshold - margin, rounded down
    double threshold;
    uint32_t tile_blocks;           // blocks of the LDS tile (4, 2 or 1)
    uint32_t span_blocks;           // blocks of one work item's stream
    const int64_t* grp;             // [total_blocks * 32] the rows' groups (PairGroups), or null: pcv_searcher_find_duplicates_grouped
    unsigned long long* skipped;    // with grp: sibling pairs with c >= threshold, counted and not emitted
};

// The groups of a row job's launch rows (pcv_searcher_neighbors_grouped, _match_grouped, _find_duplicates_grouped; DESIGN.md §4
// "Group-aware pairs"), gathered once behind the prep step from the searcher's group table (corpus.h):
//   grp[launch row] : the group key the row's id has in the table, -1: none (no entry, PCV_NO_GROUP, or the row takes no part).
//                     Two different rows are SIBLINGS iff both have grp >= 0 and the keys are equal: every exact step compares these
//   tag[launch row] : 0: no group, otherwise ((uint32_t)key & 0x7fffffff) + 1.  Equal keys give equal non-zero tags, different keys
//                     may collide: only the bound pass reads it, where "same group" by mistake can only lower a lower bound.  Zero
//                     behind total_blocks * 32
struct PairGroups {
    const float* rinv;              // [total_blocks * 32] as selfjoin_prep_kernel leaves it
    const int64_t* keys;            // the table (null: no slots)
    const int64_t* vals;
    uint32_t mask;
    int64_t side_val;
    int64_t* grp;                   // [total_blocks * 32]
    uint32_t* tag;                  // [(total_blocks + tile_blocks) * 32]
    unsigned long long* counters;   // kPairGroup* below
};
enum : int {
    kPairGroupRows = 0,   // launch rows with a group >= 0
    kPairGroupSiblings,   // listed candidates the f64 step dropped as siblings
    kPairGroupCollapsed,  // entries the select step passed over as members of a kept group
    kPairGroupCounters
};
constexpr uint32_t kGroupsSkipOwn = 1u, kGroupsOnePerGroup = 2u;  // PCV_GROUPS_* (perceive_hip.h)

// Item labels (pcv_searcher_assign, _label_sums, _kmeans; DESIGN.md §4 "Item labels"): every row against K label vectors.  Rows are
// launch rows as above, with rinv / norm exactly as selfjoin_prep_kernel leaves them (under the dot metric a participating row
// without a cosine is then marked kRinvWild: its dot products are still defined).  The labels are a small corpus of their own: one
// segment in the blocked f32 layout, `label_blocks` blocks (a whole number of tiles; scale 1 for the K labels, 0 behind them), so
// that the prep and rescore arithmetic of the rows is the labels' too.
//   w[label], mg[label] : the screening score of (row, label) is s = acc * rinv_row * w and |s - c'| <= mg, c' the canonical score
//                         in the row's units (cosine: c; dot: c / |x|).  cosine: w = 1/|l|, mg = selfjoin_margin; dot: w = 1,
//                         mg = selfjoin_margin * |l| rounded up.  w = 0: no score with this label is defined (or it is padding);
//                         w = kRinvWild: |l| outside [2^-20, 2^20], every participating row lists the label
//   lb[launch row]      : the largest s - mg seen so far over the tiles launched, a lower bound of the row's best c'; -inf at first
//   cand / cand_s       : (launch row << 32) | label and the s it was listed with (+inf for a wild row or label)
//   best_key / best_lab : per launch row, the order-preserving image of the largest c (0: none) and the lowest label reaching it
struct AssignArgs {
    float* rinv;                    // [total_blocks * 32]
    const double* norm;             // [total_blocks * 32]
    const float4* lab_blk;          // [label_blocks][D4][32] the labels, blocked f32
    const float* lab_rinv;          // [label_blocks * 32]
    const double* lab_norm;         // [label_blocks * 32]
    uint4* lab_tile;                // [label_blocks * 32][Dp / 8] bf16 pieces in the swizzled order of the LDS tile
    float* w;                       // [label_blocks * 32]
    float* mg;                      // [label_blocks * 32]
    float* lb;                      // [total_blocks * 32]
    uint64_t* cand;                 // [cand_cap]
    float* cand_s;                  // [cand_cap]
    unsigned long long* cand_key;   // [n_cand] image of c per candidate (0: below the final bound or undefined)
    unsigned long long* counters;   // [0]: candidates listed (not capped), [1]: rows whose label changed
    unsigned long long* best_key;   // [total_blocks * 32]
    uint32_t* best_lab;             // [total_blocks * 32]
    int32_t* row_label;             // [total_blocks * 32] the label of every launch row (-1: none, and before the first assignment),
                                    // kept between k-means steps: the finish step counts the rows whose entry it changes
    const int64_t* seg_out0;        // [nseg] output index of each segment's row 0
    int32_t* out_label;             // [rows]
    float* out_score;               // [rows]
    int64_t* out_ids;               // [rows]
    long long* out_counts;          // [K]
    long long* sums;                // [K][Dp] integer sums of pcv_searcher_label_sums
    long long* sum_counts;          // [K] rows that went into them
    unsigned long long cand_cap, n_cand;
    float margin;                   // selfjoin_margin(Dp)
    int K, metric;
    uint32_t tile_blocks;           // blocks of one label tile (4, 2 or 1)
    uint32_t label_blocks;
    uint32_t tile;                  // the tile of this screen launch
    uint32_t span_blocks;           // row blocks one screen workgroup streams (a multiple of its waves)
};

// Top-m labels (pcv_searcher_assign_top; DESIGN.md §4 "Top-m labels"): the m best labels of every row, in two passes over the rows per
// label tile.  `a` is the assignment's block, read as the assign kernels read it, except
//   a.lb[launch row]    : the row's FINAL threshold once every tile's bound pass and merge has run: the m-th largest column maximum
//                         (-inf: fewer than m are defined), under cosine at least min_score - margin, rounded down; -inf for a wild
//                         row.  Label j is listed for the row iff s_j + mg_j >= a.lb (or one of the two is wild)
// and best_key / best_lab / cand_key / row_label / out_* of `a` are not used.  A COLUMN of a tile is the labels 32 t + c of one lane
// column c: the columns of all tiles are disjoint label sets.
//   colmax[launch row][c]  : of the tile the bound pass last ran, the largest s - mg over the column's certified labels (-inf: none)
//   topm[launch row][8]    : the eight largest column maxima over the tiles merged so far, descending
//   row_cnt / row_off      : as NeighborArgs: the row's candidates, counted up then down, and where its stretch starts
//   sorted_key / sorted_lab: per row, in any order: the f64_key image of c (0: undefined, or below min_score) and the label
struct AssignTopArgs {
    AssignArgs a;
    float* colmax;                  // [total_blocks * 32][32]
    float* topm;                    // [total_blocks * 32][kMaxTopLabels]
    uint32_t* row_cnt;              // [total_blocks * 32]
    uint32_t* row_off;              // [total_blocks * 32 + 1]
    unsigned long long* sorted_key; // [n_cand]
    uint32_t* sorted_lab;           // [n_cand]
    int32_t* out_labels;            // [rows][m], unused slots -1
    float* out_scores;              // [rows][m], unused slots NaN
    int32_t* out_count;             // [rows]
    long long* out_label_rows;      // [K]
    float min_score;                // c >= (double)min_score; -inf: no bound
    int m;
};
constexpr int kMaxTopLabels = 8;    // PCV_MAX_TOP_LABELS

// Item neighbours and item matches (pcv_searcher_neighbors, pcv_searcher_match; DESIGN.md §4 "Item neighbours", "Item matches"): the
// k best partner rows of every owner row.  Rows are launch rows, rinv / norm exactly as selfjoin_prep_kernel leaves them.  The OWNERS
// are the rows of the launch blocks [owner_block0, total_blocks), the PARTNERS those of the blocks [0, partner_blocks): `neighbors`
// and the core step of `reach_tree` pass the whole launch for both, `match` a launch ordered [to only | to and from | from only].  A
// row is never its own partner.  A partner block with number gb is SAMPLED iff gb is a multiple of stride; sampled block
// j = gb / stride belongs to span j / span_len.  An OWNER ROW is a launch row counted from owner_block0 * 32.
//   span_max[span][owner row]  : the order-preserving image (f32_key) of the largest certified screening score of the row with a
//                                partner of that span's sampled blocks, 0: none.  The spans are disjoint sets of partners.
//   thr[launch row]            : (k-th largest defined span maximum) - 2 margin, rounded down (-inf: fewer than k are defined), and
//                                where the call has a score bound (min_score != -1) at least min_score - margin, rounded down;
//                                -inf for a wild row — every participating partner is a candidate
//   seg_ord0 / ord_seg         : the segments' order by global position, which the launch order of `match` is not: seg_ord0[i] is the
//                                launch row segment i's row 0 would have in that order (an ORDER ROW: the tie-break of select, and
//                                the launch row itself wherever the launch is in position order), ord_seg the segments sorted by it
//   cand                       : (owner launch row << 32) | partner launch row, DIRECTED: the pair (a, b) is listed for owner a
//                                iff s >= thr[a], and again for owner b iff s >= thr[b]
//   row_off[launch row]        : where the owner's candidates start in sorted_key / sorted_row (an exclusive scan of row_cnt;
//                                entry launch rows: the total); row_cnt is counted up, then counted down as the slots are taken
//   sorted_key / sorted_row    : per owner, in any order: the f64_key image of c (0: c is below the call's score bound) and the
//                                partner's order row
struct NeighborArgs {
    float* rinv;                    // [(total_blocks + tile_blocks) * 32], zero behind total_blocks * 32
    double* norm;                   // [total_blocks * 32]
    uint32_t* span_max;             // [spans][(total_blocks - owner_block0) * 32]
    float* thr;                     // [(total_blocks + tile_blocks) * 32]
    uint64_t* cand;                 // [cand_cap]
    unsigned long long* counters;   // [0]: candidates the list pass found (not capped)
    uint32_t* row_cnt;              // [total_blocks * 32]
    uint32_t* row_off;              // [total_blocks * 32 + 1]
    unsigned long long* sorted_key; // [n_cand]
    uint32_t* sorted_row;           // [n_cand]
    const int64_t* seg_out0;        // [nseg] output index of each segment's row 0 (segments with owners)
    const uint32_t* seg_ord0;       // [nseg]
    const uint32_t* ord_seg;        // [nseg]
    int64_t* out_ids;               // [rows]
    int64_t* out_nbr;               // [rows][k], unused slots -1
    float* out_score;               // [rows][k], unused slots NaN
    int32_t* out_count;             // [rows]
    unsigned long long cand_cap, n_cand;
    float margin;                   // selfjoin_margin(Dp)
    float min_score;                // the score bound of `match`: c >= (double)min_score; exactly -1: none
    int k;
    uint32_t owner_block0;          // the owners: launch blocks [owner_block0, total_blocks)
    uint32_t partner_blocks;        // the partners: launch blocks [0, partner_blocks)
    uint32_t tile_blocks;           // blocks of the LDS tile (4, 2 or 1)
    uint32_t stride;                // every stride-th partner block is streamed by this launch (the list pass: 1)
    uint32_t span_len;              // sampled blocks of one span
    uint32_t spans;                 // ceil(sampled blocks / span_len), at most kMaxNeighborSpans
    uint32_t walk_len;              // sampled blocks one workgroup streams against its tile
    // the grouped calls (PairGroups above; all null / 0 in the plain ones, whose launches do not read them)
    const int64_t* grp;             // [total_blocks * 32]; not null: the rescore step stores sorted_grp and drops siblings under
                                    // kGroupsSkipOwn, the select step writes out_grp and collapses under kGroupsOnePerGroup
    const uint32_t* tag;            // [(total_blocks + tile_blocks) * 32]
    unsigned long long* span_max64; // [spans][owner rows] group_flags != 0: (f32_key(maximum) << 32) | tag of a partner reaching it
    int64_t* sorted_grp;            // [n_cand] the partner's group, beside sorted_row
    int64_t* out_grp;               // [rows][k], unused slots -1
    unsigned long long* gcounters;  // kPairGroup*
    uint32_t group_flags;           // kGroupsSkipOwn | kGroupsOnePerGroup; != 0: the bound pass and the thresholds take their grouped form
};
constexpr uint32_t kMaxNeighborSpans = 512;  // (the threshold kernel keeps a row's maxima in eight registers a lane)

// Seed items (pcv_searcher_seeds; DESIGN.md §4 "Seed items"): k picks, one after the other, each by the weights the picks before it
// leave.  Rows are launch rows, rinv / norm exactly as selfjoin_prep_kernel leaves them (rinv != 0: the row takes part).  Workgroup
// g of the begin and cover kernels owns the launch rows [g * kSeedSpanRows, + kSeedSpanRows): launch rows ascend with the global
// position, so the order of the partials is the order of the prefix sums.
//   cover[launch row] : the largest canonical cosine with a seed so far; -inf before the first (the weight of step 0 is 1, not
//                       seed_weight(cover))
//   part[g]           : the sum of the span's weights, and its best (largest weight, lower launch row on ties; w = 0: none)
//   state             : what one step leaves for the next, and the call for the host
constexpr int kSeedSpanRows = 256;
struct SeedPart {
    unsigned long long sum;
    unsigned long long w;
    uint32_t row, pad;
};
struct SeedState {
    uint32_t centre;   // launch row of the last pick
    uint32_t done;     // a step found T == 0, or an error: every later kernel of the call returns at once
    int32_t count;     // picks made
    uint32_t error;    // kSeedNoFirst, kSeedTooManyRows, kSeedInternal
};
constexpr uint32_t kSeedNoFirst = 1u, kSeedTooManyRows = 2u, kSeedInternal = 3u;
constexpr unsigned long long kMaxSeedRows = 1ull << 30;  // weights <= 2^33: the int64 totals hold 2^30 of them
struct SeedArgs {
    const float* rinv;              // [total_blocks * 32]
    const double* norm;             // [total_blocks * 32]
    double* cover;                  // [total_blocks * 32]
    SeedPart* part;                 // [parts]
    SeedState* state;
    int64_t* out_ids;               // [k]
    int64_t* out_pos;               // [k]
    int64_t* out_totals;            // [k]
    float* out_cover;               // [k]
    uint32_t parts;                 // ceil(launch rows / kSeedSpanRows)
    int step;                       // of this launch
    int method;
    int has_first;                  // step 0 picks the first participating row carrying first_id
    int64_t first_id;
    uint64_t seed;
};

// The weight a row has once a seed exists (perceive_hip.h): rint(max(0, 1 - cover) * 2^32), ties to even.  One rounding in the
// subtraction; the product with 2^32 is exact.
__host__ __device__ static inline unsigned long long seed_weight(double cover) {
    const double d = 1.0 - cover;
    return (unsigned long long)__builtin_rint((d > 0.0 ? d : 0.0) * 0x1p32);
}
// The draw of step j among `total` units (perceive_hip.h, pcv_seed_draw): the one copy, for seed_pick_kernel and the host.
__host__ __device__ static inline uint64_t seed_draw(uint64_t seed, uint32_t j, uint64_t total) {
    uint64_t z = seed + (uint64_t)(j + 1u) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(z, total);
#else
    return (uint64_t)(((unsigned __int128)z * total) >> 64);
#endif
}

// Corpus moments and projection (pcv_searcher_moments, _project; DESIGN.md §4 "Corpus moments and principal axes").  Rows are launch
// rows, rinv / norm exactly as selfjoin_prep_kernel leaves them (rinv != 0: the row takes part).  t(r, d) is the fixed-point unit row
// of pcv_searcher_label_sums (launch_rows.h, unit_int), cut in two limbs t = h * 2^16 + l, h = t >> 16 in [-65537, 65536],
// l = t & 0xffff: both exact in f32, every limb product below 2^32.01, so an f64 sum of up to 2^20 of them is exact in any order.
//   sums[d]          : S_d = sum of t(r, d);  sums[Dp]: the participating rows
//   hh, hl, ll       : [Dp][Dp] int64, HH = H^T H, HL = H^T L, LL = L^T L summed over the participating rows; hh and ll hold the 64 x 64
//                      super-tiles on and above the diagonal only, hl all of them
//   range_blocks     : row blocks of one workgroup's accumulation chain, at most kMomentChainBlocks
constexpr uint32_t kMomentChainBlocks = 1u << 15;
static_assert((uint64_t)kMomentChainBlocks * kBlockRows <= (1ull << 20), "an f64 chain of more than 2^20 limb products is not exact");
constexpr int kMomentSide = 64;  // features of one side of a super-tile
struct MomentArgs {
    const double* norm;             // [total_blocks * 32]
    long long* sums;                // [Dp + 1]
    long long* hh;                  // [Dp][Dp]
    long long* hl;
    long long* ll;
    uint32_t range_blocks;
};
// Projection: the canonical f64 dot of every participating row with m axes.  The axes are packed like rows: axis j is lane j & 31 of
// block j >> 5 of a blocked f32 matrix with zero padding up to a whole number of blocks.
struct ProjectArgs {
    const float* rinv;              // [total_blocks * 32]
    const double* norm;             // [total_blocks * 32]
    const float4* axes;             // [ceil(m / 32)][D4][32]
    const double* offsets;          // [m]
    const int64_t* seg_out0;        // [nseg] output index of each segment's row 0
    float* out_coords;              // [rows][m]
    int64_t* out_ids;               // [rows]
    int m;
};

// Density clusters (pcv_searcher_density_clusters; DESIGN.md §4 "Density clusters"): DBSCAN under the canonical cosine.  Rows are
// launch rows, rinv / norm exactly as selfjoin_prep_kernel leaves them.  near(a, b) <=> c(a, b) >= threshold; the screening score s
// of a pair of certified rows decides it alone where s >= hi (near: a SURE pair) or s < lo (not near); the band between, and every
// pair with a wild row, is listed and decided by the f64 step.
//   degree[launch row] : partners near the row (sure pairs and confirmed band pairs, each counted once for both rows)
//   core[launch row]   : 1 iff the row takes part and degree + 1 >= min_items
//   parent[launch row] : the union-find forest over the core rows; parent[r] <= r always, so a component's root is its core row of
//                        the lowest global position
//   attach[launch row] : the lowest core launch row near a row that is not core (UINT32_MAX: none)
//   root / rank        : after the link step: the root of a core row's component, or of the component a border row attaches to
//                        (UINT32_MAX: noise or no part); rank[r] = roots at launch rows below r = the cluster number of root r
struct DensityArgs {
    float* rinv;                    // [(total_blocks + tile_blocks) * 32], zero behind total_blocks * 32
    double* norm;                   // [total_blocks * 32]
    uint64_t* cand;                 // [cand_cap] band pairs, (launch row a << 32) | launch row b, a < b
    uint64_t* conf;                 // [n_cand] the band pairs with c >= threshold, in any order
    unsigned long long* counters;   // kDensity* below
    uint32_t* degree;               // [(total_blocks + tile_blocks) * 32]
    uint8_t* core;                  // [(total_blocks + tile_blocks) * 32], zero behind total_blocks * 32
    uint32_t* parent;               // [total_blocks * 32]
    uint32_t* attach;               // [total_blocks * 32]
    uint32_t* root;                 // [total_blocks * 32]
    uint32_t* rank;                 // [total_blocks * 32]
    const int64_t* seg_out0;        // [nseg] output index of each segment's row 0
    int32_t* out_label;             // [rows]
    int8_t* out_kind;               // [rows]
    int32_t* out_degree;            // [rows]
    int64_t* out_ids;               // [rows]
    unsigned long long cand_cap, n_cand;
    float hi, lo;                   // threshold + margin rounded up, threshold - margin rounded down
    double threshold;
    int min_items;
    uint32_t tile_blocks;           // blocks of the LDS tile (4, 2 or 1)
    uint32_t span_blocks;           // blocks of one work item's stream
};
enum : int {
    kDensityBand = 0,       // band pairs the degree pass found (not capped)
    kDensityConfirmed,      // band pairs with c >= threshold
    kDensitySure,           // pairs the screen decided alone
    kDensityParticipating,
    kDensityCore,
    kDensityBorder,
    kDensityNoise,
    kDensityClusters,
    kDensityCounters
};

// Linkage tree (pcv_searcher_linkage_tree; DESIGN.md §4 "Linkage tree"): the maximum-cosine spanning tree of the participating rows
// in Borůvka rounds.  Rows are launch rows, rinv / norm exactly as selfjoin_prep_kernel leaves them.  An edge is BETTER than another
// iff its c is larger, then its lower launch row is lower, then its higher launch row is lower (launch rows ascend with the position).
//   comp[launch row]   : the root of the row's component as the round found it: the component's lowest launch row.  Plain loads:
//                        no kernel that reads it writes it.  Zero behind total_blocks * 32
//   parent[launch row] : the union-find forest the merge step works on; parent[r] <= r always ("Density clusters")
//   cert[root]         : 1 iff the component has a certified row (rinv > 0)
//   comp_max[root]     : the f32_key image of the largest certified screening score of a certified row of the component with a
//                        certified row of another component, over the partner blocks streamed so far; 0: none
//   thr[root]          : comp_max - 2 margin, rounded down; -inf: no bound — every foreign partner is a candidate
//   cand               : (owner launch row << 32) | partner launch row, DIRECTED: listed for owner a iff comp[a] != comp[b] and
//                        s >= thr[comp[a]] (or one of the two is wild);  cand_key: the f64_key image of its c
//   best_key[root]     : the largest cand_key among the component's candidates (0: none);  best_pair[root]: the lowest
//                        (lower row << 32) | higher row among those that reach it
//   edge_pair/edge_key : the edges chosen so far, in any order
struct LinkEdge {
    double c;
    int64_t pos_a, pos_b;  // output positions, pos_a < pos_b
    int64_t id_a, id_b;
};
struct LinkageArgs {
    float* rinv;                    // [(total_blocks + tile_blocks) * 32], zero behind total_blocks * 32
    double* norm;                   // [total_blocks * 32]
    uint32_t* comp;                 // [(total_blocks + tile_blocks) * 32]
    uint32_t* parent;               // [total_blocks * 32]
    uint32_t* cert;                 // [total_blocks * 32]
    uint32_t* comp_max;             // [total_blocks * 32]
    float* thr;                     // [total_blocks * 32]
    uint64_t* cand;                 // [cand_cap]
    unsigned long long* cand_key;   // [cand_cap]
    unsigned long long* best_key;   // [total_blocks * 32]
    unsigned long long* best_pair;  // [total_blocks * 32]
    unsigned long long* edge_pair;  // [edge_cap]
    unsigned long long* edge_key;   // [edge_cap]
    unsigned long long* counters;   // kLink* below
    const int64_t* seg_out0;        // [nseg] output index of each segment's row 0
    int64_t* out_ids;               // [rows]
    int8_t* out_part;               // [rows]
    LinkEdge* out_edges;            // [n_edges]
    unsigned long long cand_cap, n_cand, edge_cap, n_edges;
    float margin;                   // selfjoin_margin(Dp)
    uint32_t tile_blocks;           // blocks of the LDS tile (4, 2 or 1)
    uint32_t stride;                // every stride-th block is a partner block of this launch (the list pass: 1)
    uint32_t walk_len;              // sampled blocks one workgroup streams against its tile
};
enum : int {
    kLinkListed = 0,      // candidates the list pass of this round found (not capped)
    kLinkEmitted,         // edges chosen, all rounds
    kLinkRoots,           // components of participating rows behind this round's merge
    kLinkUnbounded,       // components with a certified row and no bound behind this round's bound pass
    kLinkCertRoots,       // components with a certified row
    kLinkParticipating,
    kLinkCounters
};

// Reach tree (pcv_searcher_reach_tree; DESIGN.md §4 "Reach tree"): the spanning tree under w(a, b) = min(core(a), core(b), c(a, b)),
// in the linkage rounds with the cap applied.  `l` is the linkage call's block, read by the linkage kernels the rounds share (begin,
// cert, the screen — given klo / khi —, threshold, choose, merge) and by the kernels of reach_kernels.hip; there cand_key, best_key
// and edge_key hold images of w, not of c.
//   core[launch row]     : the j-th largest c of the row with another participating row, f64; +inf for j == 0; NaN: no part
//   klo, khi[launch row] : core rounded down and up to f32 (-inf for a row that takes no part); zero behind total_blocks * 32
//   row_off, sorted_key  : what the neighbours' rescore step left (NeighborArgs), read by the core step alone;  k = j
struct ReachEdge {
    double w, c;
    int64_t pos_a, pos_b;  // output positions, pos_a < pos_b
    int64_t id_a, id_b;
};
struct ReachArgs {
    LinkageArgs l;
    double* core;                         // [total_blocks * 32]
    float* klo;                           // [(total_blocks + tile_blocks) * 32]
    float* khi;                           // [(total_blocks + tile_blocks) * 32]
    const uint32_t* row_off;              // [total_blocks * 32 + 1]
    const unsigned long long* sorted_key; // [candidates of the core step]
    unsigned long long* short_rows;       // participating rows with fewer than k rescored partners (never, by the neighbours' proof)
    double* out_core;                     // [rows]
    ReachEdge* out_edges;                 // [n_edges]
    int k;                                // j = min(min_items - 1, P - 1)
};

// ---- duplicate pairs (selfjoin_kernels.hip); `p` needs seg, nseg, total_blocks, D, D4 only ----
float selfjoin_margin(int Dp);  // certified bound on |screening score - canonical cosine| (DESIGN.md §4 "Duplicate pairs")
void launch_selfjoin_prep(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SelfJoinArgs& a);
void launch_selfjoin_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SelfJoinArgs& a);
void launch_selfjoin_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SelfJoinArgs& a);
// ---- item labels (assign_kernels.hip); `p` as for the duplicate pairs, plus metric ----
void launch_assign_labels(hipStream_t st, const ScanParams& p, const AssignArgs& a);  // lab_rinv, lab_norm -> w, mg, lab_tile
void launch_assign_begin(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a);  // lb, best_*, dot marks
void launch_assign_screen(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a);  // one label tile
void launch_assign_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a);
void launch_assign_finish(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a);  // winners -> outputs
void launch_label_sums(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignArgs& a);
// ---- top-m labels (assign_kernels.hip); the prep steps are the assignment's.  Per label tile a.tile: bound, then merge; then list per tile ----
void launch_assign_top_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x);    // one label tile -> colmax
void launch_assign_top_merge(hipStream_t st, const ScanParams& p, const AssignTopArgs& x);                          // colmax -> topm, a.lb
void launch_assign_top_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x);     // one label tile, a.lb -> cand
void launch_assign_top_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x);  // cand -> row_off, sorted_*
void launch_assign_top_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const AssignTopArgs& x);   // sorted_* -> outputs
// ---- item neighbours and item matches (neighbors_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_neighbors_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);    // -> span_max
void launch_neighbors_threshold(hipStream_t st, const ScanParams& p, const NeighborArgs& a);                      // span_max -> thr
void launch_neighbors_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);     // thr -> cand
void launch_neighbors_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);  // cand -> sorted_*
void launch_neighbors_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);   // sorted_* -> outputs
// the count and offsets steps alone, for any list of (owner launch row << 32) | x: row_cnt (zero before) counted up, row_off its scan
void launch_owner_offsets(hipStream_t st, const uint64_t* cand, unsigned long long n_cand, uint32_t* row_cnt, uint32_t* row_off, uint32_t launch_rows);
// ---- the rows' groups (grouped_kernels.hip); behind launch_selfjoin_prep ----
void launch_row_groups(hipStream_t st, const ScanParams& p, const ScanParams* dp, const PairGroups& a);  // rinv, the table -> grp, tag
// ---- density clusters (density_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_density_degree(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);   // -> degree, cand, counters
void launch_density_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);  // cand -> degree, conf
void launch_density_core(hipStream_t st, const ScanParams& p, const DensityArgs& a);                           // degree -> core, parent, attach
void launch_density_link(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);     // sure pairs, conf -> parent, attach
void launch_density_labels(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);   // parent, attach -> outputs
// ---- linkage tree (linkage_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
// The bound and list passes take the reach tree's cap: klo / khi of ReachArgs (the capped screen), or null (the linkage tree's).
void launch_linkage_begin(hipStream_t st, const ScanParams& p, const LinkageArgs& a);                          // comp, parent = the row; participating
void launch_linkage_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a, const float* klo = nullptr);  // comp -> cert, comp_max
void launch_linkage_threshold(hipStream_t st, const ScanParams& p, const LinkageArgs& a);                      // comp_max -> thr, counters
void launch_linkage_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a, const float* khi = nullptr);   // thr, comp -> cand
void launch_linkage_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a);   // cand -> best_key, best_pair
void launch_linkage_choose(hipStream_t st, const LinkageArgs& a);                                              // cand_key, best_key -> best_pair (the rescore step's second half)
void launch_linkage_merge(hipStream_t st, const ScanParams& p, const LinkageArgs& a);                          // best_pair -> edges, parent, comp, roots
void launch_linkage_output(hipStream_t st, const ScanParams& p, const ScanParams* dp, const LinkageArgs& a);    // edges, rinv -> outputs
// ---- reach tree (reach_kernels.hip); the core step's candidates are the neighbours', the other steps of a round the linkage tree's ----
void launch_reach_core(hipStream_t st, const ScanParams& p, const ReachArgs& a);                               // sorted_key -> core, klo, khi
void launch_reach_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a);       // cand, core -> best_key, best_pair
void launch_reach_output(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ReachArgs& a);        // edges, rinv, core -> outputs
// ---- seed items (seed_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_seed_begin(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a);  // cover = none, the partials of step 0
void launch_seed_cover(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a);  // the last pick -> cover, the partials of a.step
void launch_seed_pick(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a);   // the partials -> pick a.step, its outputs
// ---- corpus moments and projection (moments_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_moment_sums(hipStream_t st, const ScanParams& p, const ScanParams* dp, const MomentArgs& a);  // norm -> sums
void launch_moment_syrk(hipStream_t st, const ScanParams& p, const ScanParams* dp, const MomentArgs& a);  // norm -> hh, hl, ll
uint32_t moment_row_ranges(const ScanParams& p, const MomentArgs& a);
void launch_project(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ProjectArgs& a);

}  // namespace pcv
