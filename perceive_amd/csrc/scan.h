// scan.h — device data layout + launcher interface of the similarity scan.
//
// HBM layout of a corpus segment ("row-block interleaved", DESIGN.md §HBM layout):
//   rows are grouped in blocks of 32; features are padded to Dp (multiple of 64) and cut in
//   16-byte pieces f4 = feature/4; the float4 of (block b, piece f4, row r) lives at
//       blk[(b * D4 + f4) * 32 + r]            D4 = Dp/4
//   so one wave instruction (lanes r=0..31 | h=0,1) reads two contiguous 512-byte runs and each
//   lane receives exactly the 8 consecutive features an MFMA 32x32x16 A-fragment wants.
//   Same bytes as row-major f32 (plus zero padding), permuted at 16-byte granularity.
//
// Screening copy (optional, one per segment): the same rows, already multiplied by their scale and rounded to
// bf16 — exactly the A operand the MFMA screen builds from the f32 rows — in 16-byte pieces of 8 features:
//       blk16[(b * D8 + f8) * 32 + r]          D8 = Dp/8
// The coarse screen then streams 2 bytes per feature instead of 4; the f32 rows are read only for the coarse
// survivors (fine screen) and the finalists (exact rescoring), so results are unchanged.
//
// Int8 screening copy (PCV_SCREEN_COPY_INT8): y = row x scale quantised per 32-row block, x^_i = rint(y_i * s_row) in [-127, 127],
// s_row = s_blk = 127 / max|y_i| over the block's searchable rows, in 16-byte pieces of 16 features (feature dimension padded
// to a multiple of 128):
//       blk8[(b * D16 + f16) * 32 + r]         D16 = roundup(Dp, 128) / 16;      scale8[b] = s_blk
// The screen is then an exact integer dot product (v_mfma_i32_32x32x32_i8) of quantised row and quantised query,
// 384 B per 384-d vector, with the certified bound
//       |c - acc / (s_row s_q)| <= |q'|_1 * 0.5 / s_row  +  |x^|_1 / s_row * 0.5 / s_q        (+ the f32 term eps32)
// and |x^|_1 <= sqrt(D) (s_row |y|_2 + 0.5 sqrt(D)), so one float per block is all the test needs (any s_row <= 127 / max|y_i|
// of the row keeps both |x^_i| <= 127 and |y_i - x^_i / s_row| <= 0.5 / s_row).
//
// Mid copy (optional, built when the coarse screen of a corpus lets many rows through: clustered embeddings): y = row x scale
// quantised per row to int16, Y_i = rint(y_i * s2), s2 = 32766 / max|y_i|, stored ROW-MAJOR, Dp int16 per row:
//       mid16[row * (Dp / 8) + piece]          scale16[row] = s2  (NaN = row not searchable)
// A coarse survivor's exact-f32 check reads its f32 row out of the blocked layout — 96 pieces of 16 bytes, 512 bytes apart:
// 96 cache lines, 12 KB of traffic for 1536 bytes.  With the mid copy the fine screen first reads the row's 768 contiguous bytes
// (6 lines) and drops it unless   q'.Y / s2  >=  tau - (|q'|_1 * 0.5002 / s2 + margin32 * 1.5)   — |y_i - Y_i / s2| <= 0.5002 / s2,
// so the bound is ~1e-4 in cosine, the size of the f32 margin itself: what passes goes on to the f32 row as before.
//
// 6-bit screening copy (beside the int8 copy, built by AUTO for large sources): the int8 codes with their two low
// bits dropped, h = x^ >> 2 in [-32, 31], stored biased as u = h + 32 in [0, 63]; u stands for 4h + 1.5 in int8 units, i.e.
// x~ = (4h + 1.5) / s_blk in units of y.  Per block, chunk of 128 features and lane of the int8 layout (the 64 int8 values a lane
// feeds its four MFMAs of the chunk: 16 dwords d = 4 ks + j), three 16-byte pieces — 3 KB per chunk instead of 4:
//       blk6[((b * NCH + ch) * 3 + piece) * 64 + lane]      pieces 0, 1: low nibbles (dword i: d = 2i in bits 0-3, 2i + 1 in bits
//                                                          4-7 of each byte);  piece 2: the 2-bit high parts (dword k: d = 4k + m
//                                                          in bits 2m, 2m + 1 of each byte)
//       scale6[b] = {s_blk, s_blk * r_blk, s_blk * n_blk, 0}    r_blk = max |y - x~|_2, n_blk = max |x~|_2 over the block's
//                                                          searchable rows (rounded up)
// The screen multiplies u with the int8 query (acc = sum u_i q^_i, exact) and keeps a row by the L2 (Cauchy-Schwarz) bound
//       |c - (4 acc - 126.5 sum q^) / (s_blk s_q)|  <=  |q'|_2 r_blk + |e_q|_2 n_blk     (+ eps32),   e_q = q' - q^ / s_q
// one number per (block, query) like the int8 test's.  Its survivors are screened again against their int8 row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/perceive_hip.h"

namespace pcv {

constexpr int kBlockRows = 32;      // rows per corpus block
constexpr int kMaxK = PCV_MAX_RESULTS;  // largest num_results the running top-k slots hold (128)
constexpr int kSeedPartRows = 256;   // rows one seed workgroup ranks (one per thread)
constexpr int kSeedParts = 64;       // seed workgroups per query group -> up to 16384 seed rows
constexpr int kMaxWaveQueries = 4;  // wave-reduction kernel handles 1..4 queries per pass
constexpr int kHot = 256;            // uint32 words between per-query hot words (tau, cand_cnt): 1 KB apart,
                                     // so the device-wide atomics on them do not queue on one HBM channel
constexpr int kMfmaQueries = 256;   // most queries of one pass (the int8 scan up to 384-d: 256; the other MFMA scans 128)
constexpr int kScale8Stride = 1;    // floats per block in SegDesc::scale8: the block's quantisation scale

// One corpus segment as a scan launch sees it.  A launch walks any number of them: the table lives in
// device memory next to the ScanParams (one source of the reference = one or more segments,
// search.rs:24-27; every incremental add can append one).
struct SegDesc {
    const float4* blk;   // blocked matrix
    const float* scale;  // [nblocks*32] 1/|x| (cosine) or 1 (dot); 0 = row not searchable
    const int64_t* ids;  // [nblocks*32] item ids, or nullptr -> id = id0 + row
    int64_t id0;
    int64_t pos0;        // global position of row 0
    uint32_t nrows;
    uint32_t nblocks;
    uint32_t blk0;       // first block index of this segment in the launch's block numbering
    uint32_t pad;
    const uint4* blk16;  // bf16 screening copy (see below), or nullptr
    const uint4* blk8;   // int8 screening copy, or nullptr
    const uint4* mid16;  // row-major 16-bit copy (see below), or nullptr
    const float* scale16;
    const float* scale8; // [nblocks] quantisation scale of the int8 copy's blocks (NaN = no searchable row in the block)
    const uint4* blk6;   // 6-bit screening copy (above), or nullptr
    const float4* scale6;  // [nblocks] its per-block constants
};
// ---- ScanParams::flags, bit by bit ----
// One word carries the user's tuning / comparison knobs (PCV_SCAN_FLAGS at searcher creation, pcv_searcher_set_tuning) and what the
// searcher decides for the pass.  Tests, bench.py, tools/ab_scan.py and recorded profiles use the numeric words: no value moves.
constexpr uint32_t kFlagPlainLoads = 1u << 0;   // plain (temporal) corpus loads instead of non-temporal ones
constexpr uint32_t kFlagSeed16 = 1u << 1;       // 16 queries per seed workgroup (VALU seed)
constexpr uint32_t kFlagValuSeed = 1u << 2;     // the VALU seed kernel instead of the MFMA one
constexpr uint32_t kFlagTile128 = 1u << 3;      // the 128-query tile instead of the block-holding int8 scan
constexpr uint32_t kFlagSrc16 = 1u << 4;        // searcher: every segment has its bf16 screening copy, the pass streams that
constexpr uint32_t kFlagNoGuess = 1u << 5;      // no speculative start threshold
constexpr uint32_t kFlagSrc8 = 1u << 6;         // searcher: every segment has its int8 screening copy, the pass streams that
constexpr uint32_t kFlagNoLearnedGuess = 1u << 7;  // no learned part of the speculative threshold
constexpr uint32_t kFlagFourWave = 1u << 28;    // the older 4-waves-a-workgroup int8 scan instead of the DRAIN form
constexpr uint32_t kTuneNoSix = 1u << 29;       // never build or stream the 6-bit copy
constexpr uint32_t kTuneFailCopyAlloc = 1u << 30;  // the public PCV_TUNE_FAIL_COPY_ALLOC: taken out of the word by set_tuning, never in a pass
constexpr uint32_t kFlagSix = 1u << 31;         // searcher: the pass streams the 6-bit copies
constexpr uint32_t kTuneForceSix = 1u << 31;    // user: AUTO builds the 6-bit copy at any size
constexpr uint32_t flags_groups_per_cu(uint32_t f) { return (f >> 8) & 0xffu; }  // bits 8..15: workgroups per CU (0: the launcher's own)
constexpr uint32_t flags_seed_parts(uint32_t f) { return (f >> 16) & 0xffu; }    // bits 16..23: seed workgroups (0: kSeedParts)
constexpr uint32_t flags_chunk_bufs(uint32_t f) { return (f >> 24) & 0xfu; }     // bits 24..27: chunk buffers (0: the launcher's own)
// The bits the searcher sets itself for every pass, whatever the user's word holds there.  Bit 31 has two readers: in the
// searcher's tuning word it is the user's wish (kTuneForceSix, asked when the copies are built), in ScanParams::flags it is the
// searcher's decision for this pass (kFlagSix) — a pass starts from the tuning word with these bits cleared.
constexpr uint32_t kFlagsSearcherOwned = kFlagSrc16 | kFlagSrc8 | kFlagSix;
static_assert(kFlagPlainLoads == 1u && kFlagSeed16 == 2u && kFlagValuSeed == 4u && kFlagTile128 == 8u && kFlagSrc16 == 16u &&
                  kFlagNoGuess == 32u && kFlagSrc8 == 64u && kFlagNoLearnedGuess == 128u,
              "the low flag bits are part of recorded PCV_SCAN_FLAGS words");
static_assert(kFlagFourWave == 0x10000000u && kTuneNoSix == 0x20000000u && kTuneFailCopyAlloc == 0x40000000u &&
                  kTuneFailCopyAlloc == (uint32_t)PCV_TUNE_FAIL_COPY_ALLOC && kFlagSix == 0x80000000u && kTuneForceSix == 0x80000000u,
              "the high flag bits are part of recorded PCV_SCAN_FLAGS words");
static_assert(kFlagsSearcherOwned == 0x80000050u, "bits 4, 6 and 31 are the searcher's");
static_assert(flags_groups_per_cu(0x0000ab00u) == 0xabu && flags_seed_parts(0x00cd0000u) == 0xcdu && flags_chunk_bufs(0x0e000000u) == 0xeu &&
                  flags_groups_per_cu(~0xff00u) == 0u && flags_seed_parts(~0xff0000u) == 0u && flags_chunk_bufs(~0x0f000000u) == 0u,
              "the multi-bit fields are bits 8..15, 16..23 and 24..27");

struct pcv_hit_dev {
    double score;
    int64_t pos;
    int64_t id;
};

// More results than a pass ranks (num_results > kMaxK): pcv_searcher_search goes over the rows again for the next kMaxK, and
// again, each pass counting only the rows that rank strictly AFTER the last hit of the pass before it — the pass's ceiling, one
// per query (the reference has no limit on num_results: search.rs:157-182; perceive-cli's --num-results is user input).
//   score, pos : the canonical score and position of that hit; +inf / -1: no ceiling for this query; -inf / INT64_MAX: nothing
//                ranks after it (the query has all the rows there are)
//   lo, hi     : the same boundary in units of the f32 screening score, one fine margin below and above it.  A row with
//                screening score s < lo certainly ranks after the boundary: it counts and may raise the running thresholds;
//                lo <= s <= hi: it counts (the exact ranking decides) but must not raise them; s > hi: it ranks at or before
//                the boundary and is not listed.  The thresholds thus rest on k rows that count, and the argument for the
//                screens (scan_kernels.hip) holds among the rows that count.
struct CeilRec {
    double score;
    int64_t pos;
    float lo, hi;
};

// A range pass (pcv_searcher_search_range; DESIGN.md §4 "Range search"): every row is of class 1 of a CeilRec (lo = -inf,
// hi = +inf: listed, never raising a threshold), and the thresholds are fixed before the scan, one per query.
//   bound : the caller's bound on the REPORTED f32 score (cosine: score >= bound; dot: distance <= bound)
//   tau   : the canonical value of the bound in f32, rounded towards "keeps more": no in-range row has c < tau
struct RangeRec {
    float bound, tau;
};
constexpr int kRangeRun = 4096;  // survivors one workgroup of range_select_kernel scores and sorts in LDS

// Everything one pass needs, resident in device memory (uploaded with the segment table and the
// queries in ONE copy): the kernels index p.seg[] at run time, which a by-value kernel argument would
// force through scratch memory.
struct ScanParams {
    const SegDesc* seg;      // [nseg] device table, blk0 ascending
    int nseg;
    uint32_t total_blocks;
    int D;                   // embedding width
    int D4;                  // Dp / 4
    int B;                   // queries in this pass
    int k;
    int metric;
    uint32_t tile_rows;      // rows of the bf16 query tile the scan kernel stages (rows >= B are zeroed)
    const CeilRec* ceil;     // [B] the pass's ceilings, or nullptr (the first kMaxK results: every row counts)
    const float* queries;    // [B][D]    raw queries as the caller passed them
    float* qf32;             // [B][Dp]   scan-side query (normalised for cosine), zero padded
    uint16_t* qbf16;         // [128][Dp] same, rounded to bf16
    int8_t* q8;              // [256][Dp8] same, quantised per query to int8 (int8 screen; Dp8 = Dp rounded up to 128)
    float* q8c;              // [256][4]  s_q (quantisation scale, 0 = dead query), V_q of the int8 test (scan_mfma8_kernel), |q'|_1 (mid screen), -;
                             // then [256][4] of the 6-bit test: s_q |q'|_2, s_q |e_q|_2 (both rounded up), -W_q + slack (scan_mfma8_kernel), -
    float* qraw;             // [B][Dp]   original query values, zero padded (exact rescoring)
    float* margin;           // [B]  coarse screen: rows with s16 < tau - margin are dropped       (eps16 + eps32)
    float* margin32;         // [B]  fine screen:   rows with s32 < tau - margin32 are dropped     (2 * eps32)
    uint32_t* tau;           // [B*kHot]  ordered key of the running k-th best f32 score (word q*kHot)
    uint32_t* tau_c;         // [256]     the same keys side by side (raised right after tau, so never above it): one load instead of a
                             //           64-line gather for a wave that wants all thresholds of the pass — for FEW readers (the one drain
                             //           wave per CU of scan_mfma8_kernel's DRAIN form, about once a microsecond).  Read by every wave at
                             //           every block these 256 bytes are one hot spot in one memory channel: the 4-waves-a-workgroup form
                             //           went from 0.94 to 1.04 ms at 12.5M rows with it, which is what the 1 KB spacing of `tau` is for
    uint32_t* slots;         // [B][kMaxK] ordered keys of k distinct rows' f32 scores
    uint32_t* cand_cnt;      // [B*kHot]  survivors emitted per query (word q*kHot); word q*kHot + 32: rows that passed the COARSE screen
                             //           (statistics only: pcv_scan_stats.coarse_survivors)
    uint64_t* cand;          // [B][cand_cap]  (segment index << 32) | row
    float* cand_s;           // [B][cand_cap]  f32 screening score the row was emitted with
    pcv_hit_dev* out;        // [B][k] device results
    pcv_hit_dev* out_host;   // pinned host mirror of `out`, or nullptr
    uint32_t* cnt_host;      // [B] pinned host: survivors per query, uncapped (the host sizes a rerun from it)
    uint32_t* coarse_host;   // [2][256] pinned host: coarse survivors per query (MFMA scans), then the pairs the mid screen let through
    pcv_hit_dev* flag_rec;   // overflow record behind a shard's hit list (device), or nullptr
    uint32_t cand_cap;
    uint32_t seed_blocks;    // blocks of segment 0 ranked by the seed kernel: blocks i << seed_shift, i < seed_blocks — spread
    uint32_t seed_shift;     // over the whole segment, so that rows stored in an order that goes with their content (by topic, by
                             // date) still give a sample of all of it
    uint32_t flags;          // kFlag* / kTune* bits and the flags_*() fields above
    unsigned long long* stamps;  // diagnostic build only (-DPCV_STAMPS, tools/build_stamps.sh): 8 words per wave of the scan launch, else nullptr
    float eps16, eps32;      // |s - c| bounds of the bf16 / f32 screening scores, relative to |q||x|
    float max_norm;          // upper bound of |x| over the corpus (dot metric margins)
    // Speculative start threshold (MFMA scans; 0 = off).  The k slots the seed kernel fills are the best scores of k
    // disjoint groups of seed rows; min(slots) is a certified k-th best, but a weak one, and every wave screens its
    // first block against it.  set_guess (quantize_queries_kernel / set_guess_kernel) therefore raises tau to the spec_rank-th LARGEST slot — a guess
    // that at least k rows of the whole pass score that high — and rescore_select_kernel checks the guess: it counts the
    // survivors whose f32 score is above it by the fine margin; fewer than k and the query reports 0xffffffff survivors,
    // the pass is repeated without the guess (searcher.cpp: finish_pass).  A checked guess keeps the result exact:
    // with k rows at or above it the true k-th best is too, and no screen drops a row at or above tau - its margin.
    // The host picks spec_rank so that, for rows in an order unrelated to the query, a guess fails with probability
    // < 1e-6 (C(k-1, j) (seed rows / rows)^j: j of the k-1 best rows of the pass would have to be seed rows).
    //
    // On top of that distribution-free guess the searcher learns one from its own passes (spec_gap, NaN = none): how far
    // the k-th best score of a pass ended up above the MEDIAN seed slot of its query (both come back through pinned
    // memory: kth_host, spec_base_host); a fraction of the smallest gap of the recent passes is added to the median
    // slot of the next queries.  Self-calibrating, and checked like the other: a corpus whose queries differ a lot
    // simply learns a small gap.
    uint32_t* spec;          // [256] key of the guess per query (kKeyNegInf: none), written by set_guess
    int spec_rank;
    float spec_gap;
    float spec_spread;       // learned: mean (best - median) seed slot; a query takes the learned gap only if its own is within 50 %
    float* spec_base_host;   // [256] pinned: median seed slot per query (NaN: none)
    float* spec_top_host;    // [256] pinned: best seed slot per query
    float* kth_host;         // [256] pinned: k-th best exact score per query (NaN: fewer than k hits)
    // A range pass (RangeRec above; nullptr: a top-k pass).  range_select_kernel takes the place of rescore_select_kernel: the
    // in-range rows of run r of query q (listed survivors [r * kRangeRun, +kRangeRun)) in canonical order.
    const RangeRec* range;   // [B]
    pcv_hit_dev* range_out;  // pinned host [B][range_runs][range_keep]: the first range_keep in-range rows of each run
    uint32_t* range_cnt;     // pinned host [B][range_runs]: in-range rows of the run (not capped by range_keep)
    uint32_t range_runs;     // runs per query the lists have room for: ceil(cand_cap / kRangeRun)
    uint32_t range_keep;     // min(kRangeRun, max_results)
};
constexpr uint32_t kSpecFailed = 0xffffffffu;  // cnt_host value of a query whose speculative threshold did not hold

// Distinct results (pcv_searcher_search_distinct; DESIGN.md §4 "Distinct results"): the ranked list of a query is walked best
// first, kMaxK hits a pass, and a row is kept iff its canonical cosine with every row kept before it is below the threshold.
// What the walk of one query has come to, between the passes (device) and as the host reads it after each (pinned):
//   kept, examined : rows kept; entries of the ranked list walked
//   flags          : kDistinctFull: the num_results-th row was kept; kDistinctEnd: the list ended — either way the query is
//                    finished and distinct_select_kernel leaves its record, kept rows and counters as they are
//   last_score/pos : the last entry walked, the ceiling of the query's next pass (scan.h, CeilRec)
struct DistinctRec {
    uint32_t kept, examined, flags, pad;
    double last_score;
    int64_t last_pos;
};
constexpr uint32_t kDistinctFull = 1u, kDistinctEnd = 2u;
// The select step's own arguments (by value: nothing in it is indexed at run time).
struct DistinctArgs {
    DistinctRec* rec;        // [B]
    DistinctRec* rec_host;   // [B] pinned host mirror, written after every pass
    pcv_hit_dev* kept;       // [B][kMaxK] the kept rows, best first, as the pass listed them
    double* kept_norm;       // [B][kMaxK] their canonical |x|^2 (f64, feature order)
    int32_t* similar;        // [B][kMaxK] walked rows dropped in favour of each
    int num_results;
    double threshold;
};

// Grouped results (pcv_searcher_search_grouped; DESIGN.md §4 "Grouped results"): the same walk, kMaxK hits a pass, with another
// relation — a row is kept iff no kept row carries its group key (the searcher's group table, corpus.h).  The walk's record is
// DistinctRec, with the same meaning of every field.
struct GroupedArgs {
    DistinctRec* rec;        // [B]
    DistinctRec* rec_host;   // [B] pinned host mirror, written after every pass
    pcv_hit_dev* kept;       // [B][kMaxK] the kept rows, best first, as the pass listed them
    int64_t* kept_group;     // [B][kMaxK] their group keys (-1: a row without a group)
    int32_t* collapsed;      // [B][kMaxK] walked rows collapsed into each
    const int64_t* keys;     // the group table (nullptr: it has no slots — every row is a group of its own)
    const int64_t* vals;
    uint32_t mask;
    int64_t side_val;        // the group of id INT64_MIN, which has no slot (-1: none)
    int num_results;
};

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
};

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

// Item neighbours (pcv_searcher_neighbors; DESIGN.md §4 "Item neighbours"): the k best other rows of every row.  Rows are launch
// rows, rinv / norm exactly as selfjoin_prep_kernel leaves them.  A launch block with number gb is SAMPLED iff gb is a multiple of
// stride; sampled block j = gb / stride belongs to span j / span_len.
//   span_max[span][launch row] : the order-preserving image (f32_key) of the largest certified screening score of the row with a
//                                partner of that span's sampled blocks, 0: none.  The spans are disjoint sets of partners.
//   thr[launch row]            : (k-th largest defined span maximum) - 2 margin, rounded down; -inf: fewer than k are defined, or
//                                the row is wild — every participating partner is a candidate
//   cand                       : (owner launch row << 32) | partner launch row, DIRECTED: the pair (a, b) is listed for owner a
//                                iff s >= thr[a], and again for owner b iff s >= thr[b]
//   row_off[launch row]        : where the owner's candidates start in sorted_key / sorted_row (an exclusive scan of row_cnt;
//                                entry launch rows: the total); row_cnt is counted up, then counted down as the slots are taken
//   sorted_key / sorted_row    : per owner, in any order: the f64_key image of c and the partner's launch row
struct NeighborArgs {
    float* rinv;                    // [(total_blocks + tile_blocks) * 32], zero behind total_blocks * 32
    double* norm;                   // [total_blocks * 32]
    uint32_t* span_max;             // [spans][total_blocks * 32]
    float* thr;                     // [(total_blocks + tile_blocks) * 32]
    uint64_t* cand;                 // [cand_cap]
    unsigned long long* counters;   // [0]: candidates the list pass found (not capped)
    uint32_t* row_cnt;              // [total_blocks * 32]
    uint32_t* row_off;              // [total_blocks * 32 + 1]
    unsigned long long* sorted_key; // [n_cand]
    uint32_t* sorted_row;           // [n_cand]
    const int64_t* seg_out0;        // [nseg] output index of each segment's row 0
    int64_t* out_ids;               // [rows]
    int64_t* out_nbr;               // [rows][k], unused slots -1
    float* out_score;               // [rows][k], unused slots NaN
    int32_t* out_count;             // [rows]
    unsigned long long cand_cap, n_cand;
    float margin;                   // selfjoin_margin(Dp)
    int k;
    uint32_t tile_blocks;           // blocks of the LDS tile (4, 2 or 1)
    uint32_t stride;                // every stride-th block is a partner block of this launch (the list pass: 1)
    uint32_t span_len;              // sampled blocks of one span
    uint32_t spans;                 // ceil(sampled blocks / span_len), at most kMaxNeighborSpans
    uint32_t walk_len;              // sampled blocks one workgroup streams against its tile
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

// float <-> order-preserving uint32 key (for atomicMax / CAS on scores)
__host__ __device__ static inline uint32_t f32_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float key_f32(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}
constexpr uint32_t kKeyNegInf = 0x007fffffu;  // f32_key(-inf)
// the same for a double (no finite value has key 0)
__host__ __device__ static inline uint64_t f64_key(double d) {
    uint64_t u = __builtin_bit_cast(uint64_t, d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ static inline double key_f64(uint64_t k) {
    uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __builtin_bit_cast(double, u);
}

// The f32 score a result carries, from the canonical f64 score c (the reference's convention: cosine (float)c; dot: the distance
// max(0, 1 - c/D), search.rs:275-277).  The one copy of this arithmetic: the top-k outputs, the range outputs and the in-range
// test of range_select_kernel all call it, which is what makes a range result bit-for-bit a cut top-k result.
__host__ __device__ static inline float reported_score(int metric, int D, double c) {
    if (metric == PCV_METRIC_DOT) {
        const double d = 1.0 - c / (double)D;
        return (float)(d > 0.0 ? d : 0.0);
    }
    return (float)c;
}

// ---- launchers (scan_kernels.hip); they throw pcv::Error on a bad shape or a failed HIP call ----
// `p` is the host copy (shapes for the launch geometry), `dp` the same struct resident in device memory.
void launch_upload(hipStream_t st, const void* src_pinned, void* dst, size_t bytes);  // pinned host -> device, on the compute queue
void launch_prep_seed(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SegDesc& seg0);
void launch_scan_wave(hipStream_t st, const ScanParams& p, const ScanParams* dp, int num_cus);
void launch_scan_mfma(hipStream_t st, const ScanParams& p, const ScanParams* dp, int num_cus);
int mfma_pass_queries(int Dp);   // queries one MFMA pass can take at this padded dim (LDS-limited), 0 = none
uint32_t mfma_tile_rows(int B);  // rows of the bf16 query tile the MFMA kernel stages for B queries
void launch_scan_mfma8(hipStream_t st, const ScanParams& p, const ScanParams* dp, int num_cus);  // quantises the queries first
int mfma8_pass_queries(int Dp);  // queries one int8 MFMA pass can take (LDS-limited)
// whether a pass of B queries over rows of Dp padded features streams the 6-bit copy when every segment has one (the DRAIN form)
bool mfma8_six_pass(int B, int Dp, uint32_t flags, int nseg);
void launch_rescore_select(hipStream_t st, const ScanParams& p, const ScanParams* dp);
// ---- range search (pcv_searcher_search_range) ----
void launch_range_thresholds(hipStream_t st, const ScanParams& p, const ScanParams* dp);  // RangeRec::tau -> tau, tau_c
void launch_range_select(hipStream_t st, const ScanParams& p, const ScanParams* dp);
// ---- distinct results (distinct_kernels.hip): walks the p.k hits per query the pass left in p.out ----
void launch_distinct_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DistinctArgs& a);
// ---- grouped results (grouped_kernels.hip): likewise, against the group table ----
void launch_grouped_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const GroupedArgs& a);
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
// ---- item neighbours (neighbors_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_neighbors_bound(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);    // -> span_max
void launch_neighbors_threshold(hipStream_t st, const ScanParams& p, const NeighborArgs& a);                      // span_max -> thr
void launch_neighbors_list(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);     // thr -> cand
void launch_neighbors_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);  // cand -> sorted_*
void launch_neighbors_select(hipStream_t st, const ScanParams& p, const ScanParams* dp, const NeighborArgs& a);   // sorted_* -> outputs
// ---- density clusters (density_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_density_degree(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);   // -> degree, cand, counters
void launch_density_rescore(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);  // cand -> degree, conf
void launch_density_core(hipStream_t st, const ScanParams& p, const DensityArgs& a);                           // degree -> core, parent, attach
void launch_density_link(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);     // sure pairs, conf -> parent, attach
void launch_density_labels(hipStream_t st, const ScanParams& p, const ScanParams* dp, const DensityArgs& a);   // parent, attach -> outputs
// ---- seed items (seed_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_seed_begin(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a);  // cover = none, the partials of step 0
void launch_seed_cover(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a);  // the last pick -> cover, the partials of a.step
void launch_seed_pick(hipStream_t st, const ScanParams& p, const ScanParams* dp, const SeedArgs& a);   // the partials -> pick a.step, its outputs
// ---- corpus moments and projection (moments_kernels.hip); `p` as for the duplicate pairs; the prep step is launch_selfjoin_prep ----
void launch_moment_sums(hipStream_t st, const ScanParams& p, const ScanParams* dp, const MomentArgs& a);  // norm -> sums
void launch_moment_syrk(hipStream_t st, const ScanParams& p, const ScanParams* dp, const MomentArgs& a);  // norm -> hh, hl, ll
uint32_t moment_row_ranges(const ScanParams& p, const MomentArgs& a);
void launch_project(hipStream_t st, const ScanParams& p, const ScanParams* dp, const ProjectArgs& a);
void launch_reset_scan_state(hipStream_t st, uint32_t* tau, uint32_t* slots, uint32_t* cand_cnt);
void launch_merge(hipStream_t st, const pcv_hit_dev* lists, int n_shards, int B, int k, pcv_hit_dev* out,
                  int flagged = 0);
void launch_similarity_matrix(hipStream_t st, const float* a, int B, const float* m, int64_t N, int D, int cosine,
                              float* out);

}  // namespace pcv
