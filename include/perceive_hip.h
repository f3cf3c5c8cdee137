/*
 * perceive_hip.h — C ABI of the MI355X-native replacement for perceive-core's hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer: the path
 * sits behind ordinary Rust `pub` items of crate `perceive-core`.  Each entry point below names
 * the reference item it replaces (paths relative to the reference checkout).  A Rust shim
 * (`extern "C"` block + `Model`/`Searcher` wrappers) binds exactly these symbols.
 *
 * Conventions
 *   - every function returns a pcv_status (0 = ok); no C++ exception or abort crosses the boundary;
 *   - pcv_last_error() returns a thread-local, NUL-terminated description of the last failure;
 *   - all handles are opaque; outputs are caller-allocated; the library never frees caller memory;
 *   - host pointers unless a parameter is documented as a device pointer;
 *   - a searcher handle may be searched from several host threads (calls serialise on an internal
 *     mutex, like the reference's model worker channel `model.rs:161,187`).
 */
#ifndef PERCEIVE_HIP_H
#define PERCEIVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int pcv_status;
enum {
    PCV_OK = 0,
    PCV_ERR_INVALID = 1,      /* bad argument / bad handle state                                */
    PCV_ERR_DEVICE = 2,       /* a HIP call failed (no GPU, out of memory, launch failure)      */
    PCV_ERR_UNSUPPORTED = 3,  /* shape outside what the kernels implement                       */
    PCV_ERR_IO = 4,           /* weight / vocab file problems                                   */
    PCV_ERR_INTERNAL = 5
};

/* Ranking metric of a searcher.
 * PCV_METRIC_COSINE : score = cos(q, x), the brute-force path `lib.rs:67-77`
 *                     (cosine_similarity_single_query / _multi_query); results best-first.
 * PCV_METRIC_DOT    : ranks by the raw dot product and reports the reference Searcher's distance
 *                     `max(0, 1 - dot/len)` (`search.rs:266-279`), ascending like `search.rs:179`. */
enum { PCV_METRIC_COSINE = 0, PCV_METRIC_DOT = 1 };

typedef struct pcv_ctx pcv_ctx;
typedef struct pcv_searcher pcv_searcher;
typedef struct pcv_model pcv_model;
typedef struct pcv_tokenizer pcv_tokenizer;

/* ---- library / device context ------------------------------------------------------------- */

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* pcv_last_error(void);

/* Library version string, e.g. "perceive-hip 0.1 (gfx950)". */
const char* pcv_version(void);

/* Number of visible HIP devices (0 when there is no GPU; never fails). */
int pcv_device_count(void);

/* Bind a context to one GPU.  One process drives one GPU (one rank per device); the context owns
 * the HIP stream every kernel of its handles is launched on.
 * Replaces: `tch::Device::cuda_if_available()` at model.rs:117 / configs.rs:117. */
pcv_status pcv_init(int device_index, pcv_ctx** out_ctx);
pcv_status pcv_shutdown(pcv_ctx* ctx);
/* Block until everything queued on the context's stream has finished. */
pcv_status pcv_synchronize(pcv_ctx* ctx);
/* The context's hipStream_t (as void*), for callers that order their own work against it. */
void* pcv_stream(pcv_ctx* ctx);
/* adopt != 0: queue all further work of this context on the caller's hipStream_t `hip_stream` (NULL = the
 * device's default stream) — e.g. the stream a host framework runs its collectives against — so that
 * both are ordered without host synchronisation.  adopt == 0: back to the context's own stream.  The
 * handle must come from the HIP runtime this library is bound to.  Drains the stream in use first. */
pcv_status pcv_set_stream(pcv_ctx* ctx, void* hip_stream, int adopt);

/* Plain device buffers for hosts that have no HIP binding of their own (the per-shard hit lists that
 * an RCCL all-gather exchanges live in such buffers). */
pcv_status pcv_device_alloc(pcv_ctx* ctx, size_t n_bytes, void** out_dptr);
pcv_status pcv_device_free(pcv_ctx* ctx, void* dptr);
pcv_status pcv_copy_to_host(pcv_ctx* ctx, void* dst_host, const void* src_dev, size_t n_bytes);
pcv_status pcv_copy_to_device(pcv_ctx* ctx, void* dst_dev, const void* src_host, size_t n_bytes);

/* ---- embedding blob codec (search.rs:281-294) ---------------------------------------------- */

/* deserialize_embedding: `n_bytes/4` little-endian f32 (trailing bytes that do not fill a chunk
 * are an error here; the reference would panic on the short chunk). */
pcv_status pcv_deserialize_embedding(const uint8_t* blob, size_t n_bytes, float* out, size_t out_cap,
                                     size_t* out_len);
/* serialize_embedding: writes 4*n bytes, little-endian. */
pcv_status pcv_serialize_embedding(const float* v, size_t n, uint8_t* out, size_t out_cap);

/* ---- Searcher (search.rs:29-260) ------------------------------------------------------------ */

/* Searcher::build, part 1 (search.rs:38-56): an empty index for `dim`-wide f32 embeddings. */
pcv_status pcv_searcher_create(pcv_ctx* ctx, int dim, int metric, pcv_searcher** out);
pcv_status pcv_searcher_destroy(pcv_searcher* s);

/* build_sources row insert (search.rs:87-113,146-148): append `n` rows (row-major [n][dim] f32,
 * host memory) with their item ids to source `source_id`.  The rows are uploaded and packed into the HBM
 * layout before the call returns (staged in bounded steps: the library keeps no host copy, so a corpus can
 * be streamed through a buffer of any size); they become searchable after pcv_searcher_finalize.
 * `ids` may be NULL: ids are then the row's running index in the source. */
pcv_status pcv_searcher_add_rows(pcv_searcher* s, int64_t source_id, const int64_t* ids,
                                 const float* rows, int64_t n);
/* Same, from the on-disk form: `n` blobs of dim*4 bytes each, back to back (search.rs:99,281). */
pcv_status pcv_searcher_add_blobs(pcv_searcher* s, int64_t source_id, const int64_t* ids,
                                  const uint8_t* blobs, int64_t n);
/* Synthetic rows generated on the device (never cross PCIe): row r (0-based within this call) of
 * the source is synth_row(seed, first_row + r); ids are first_row + r.  See DESIGN.md §synthetic
 * data; oracle/synth.c is the CPU twin.  normalize != 0 stores x/|x| instead of x. */
pcv_status pcv_searcher_add_synthetic(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed,
                                      int64_t first_row, int normalize);
/* Clustered synthetic rows (what a fixed-width screen has to survive on real sentence embeddings):
 * row = centroid(cluster(row)) / sqrt(dim) + noise * u(row) * synth_row(seed, row), u uniform in [0.5, 1.5), with
 * n_clusters seeded centroids; the cosines inside a cluster spread over ~noise^2 * dim.  n_clusters = 0: plain rows. */
pcv_status pcv_searcher_add_synthetic_clustered(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed,
                                                int64_t first_row, int normalize, int n_clusters, float noise);
/* Un-normalised synthetic rows whose norms spread — what a dot-product model (the reference's default
 * MsMarcoBertBaseDotV5, perceive-cli/state.rs:24) stores: row = a(row) * synth_row(seed, row), a(row) uniform in
 * [amp_lo, amp_hi) from a hash of the row number; 0 < amp_lo < amp_hi.  Bit-identical CPU twin: oracle/synth.c. */
pcv_status pcv_searcher_add_synthetic_scaled(pcv_searcher* s, int64_t source_id, int64_t n, uint64_t seed,
                                             int64_t first_row, float amp_lo, float amp_hi);
/* Capacity hint (search.rs:138-140 sizes each source's index from its row count before inserting): the
 * host is about to add `n_rows` more rows to `source_id`, e.g. the COUNT(*) of the build query.  The rows
 * then land in one device segment instead of a chain of growing ones.  Optional; no-op for n_rows = 0. */
pcv_status pcv_searcher_reserve(pcv_searcher* s, int64_t source_id, int64_t n_rows);
/* Searcher::rebuild_source (search.rs:58-79): drop every row of `source_id`; follow with
 * add_* + finalize to install the replacement.  Unknown source: no-op. */
pcv_status pcv_searcher_clear_source(pcv_searcher* s, int64_t source_id);
/* The swap of Searcher::rebuild_source (search.rs:57-79: the new SourceSearch is built first and takes the old one's
 * place only once it exists): the rows of source `from_source_id` become the rows of `to_source_id`, whose old rows
 * are dropped; `from_source_id` disappears.  `from` unknown or empty: `to` is left absent (search.rs:67-69).  Build
 * the replacement under a staging id (add_* + finalize: a failure on the way leaves `to` untouched — clear the
 * staging id then), swap, finalize.  PCV_STAGING_SOURCE is the id this library's own loaders stage under: rows under it are
 * not counted (pcv_searcher_num_rows / num_sources / source_ids) and a search of "every source" (source_ids = NULL) does not
 * see them; between pcv_searcher_add_* and the next pcv_searcher_finalize every search fails (rows without scales), as after
 * any add — a rebuild has to be serialised against searches by the caller, like Searcher::rebuild_source's &mut self. */
#define PCV_STAGING_SOURCE INT64_MIN
pcv_status pcv_searcher_replace_source(pcv_searcher* s, int64_t from_source_id, int64_t to_source_id);
/* Pack pending rows into the HBM layout, compute row norms (set_searching_mode, search.rs:150). */
pcv_status pcv_searcher_finalize(pcv_searcher* s);

/* Searcher::build (search.rs:38-56) / rebuild_source (search.rs:58-79) straight from the reference's SQLite
 * file: runs `SELECT id FROM sources` and the items / item_embeddings join of search.rs:87-93 for
 * (model_id, model_version) — rows with `skipped` or `hidden_at` set never enter the index — streams the
 * embedding blobs into the device (one segment per source, sized from a COUNT), and finalizes.
 *   only_source   NULL: every source of the database; else that source is reloaded: its new rows are read, checked and
 *                 packed under PCV_STAGING_SOURCE first and replace the old ones only when all of them are in
 *                 (search.rs:57-79) — after a failure (a blob of the wrong size, an SQLite error) the old rows are
 *                 still there and searchable
 *   out_rows      rows loaded (may be NULL)
 * SQLite is bound at run time (libsqlite3.so.0); PCV_ERR_UNSUPPORTED if it is not installed. */
pcv_status pcv_searcher_load_sqlite(pcv_searcher* s, const char* db_path, uint32_t model_id, uint32_t model_version,
                                    const int64_t* only_source, int64_t* out_rows);

pcv_status pcv_searcher_dim(pcv_searcher* s, int* out_dim);
pcv_status pcv_searcher_num_rows(pcv_searcher* s, int64_t* out_rows);
/* Device segments the rows currently occupy (diagnostics: adds append in place while a segment has room). */
pcv_status pcv_searcher_num_segments(pcv_searcher* s, int* out_n);
pcv_status pcv_searcher_num_sources(pcv_searcher* s, int* out_n);
pcv_status pcv_searcher_source_ids(pcv_searcher* s, int64_t* out_ids, int cap);
/* Rows held for one source (0 if the source is unknown). */
pcv_status pcv_searcher_source_num_rows(pcv_searcher* s, int64_t source_id, int64_t* out_rows);
/* Read rows back (row-major) by global position (sources in insertion order, rows in insertion
 * order inside a source).  Test/diagnostic path. */
pcv_status pcv_searcher_get_rows(pcv_searcher* s, const int64_t* positions, int64_t n, float* out_rows,
                                 int64_t* out_ids);

/* Hidden items (Searcher::hidden, search.rs:31-34; `perceive hide <id>`, cmd/hide.rs:16-17): the searcher keeps a set of hidden
 * item ids, and a row is a possible result of a search (pcv_searcher_search, _search_device, _search_device_begin[_dq] / _end,
 * _search_sharded[_dq]) iff its id is not in the set and its norm is valid.  No rebuild: the rows stay where they are.
 *   - by id, not by position: every row carrying a hidden id is hidden, in every source (rows staged under PCV_STAGING_SOURCE too);
 *   - the set persists: ids that match no row are remembered, rows added later with a hidden id are hidden when
 *     pcv_searcher_finalize gives them their scale, pcv_searcher_clear_source / _replace_source do not forget it;
 *   - hidden rows keep their global positions: pcv_searcher_num_rows, _source_num_rows and _get_rows still count and read them;
 *     the scores and tie order of the other rows are those of a searcher that never held the hidden ones, and a search returns
 *     fewer than num_results hits only when fewer visible rows exist;
 *   - unhiding returns the rows exactly: every search afterwards returns what it returned before they were hidden (ids, scores,
 *     counts), for every kernel, screening copy, mid copy and num_results;
 *   - with an empty set nothing runs differently (finalize does no extra work).
 * hide_ids / unhide_ids add ids to / remove ids from the set (duplicates and ids not present allowed).  They need a finalized
 * searcher (PCV_ERR_INVALID with pending rows, like pcv_searcher_source_num_rows) and no queued pass.  out_rows (may be NULL):
 * rows whose state changed, i.e. rows carrying an id that entered / left the set. */
pcv_status pcv_searcher_hide_ids(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows);
pcv_status pcv_searcher_unhide_ids(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows);
/* The hidden set, ascending: the first min(cap, *out_n) ids into out_ids, *out_n = its size (call with cap 0 to ask).
 * out_hidden_rows (may be NULL): rows hidden now (rows added since the last finalize count from the next one on). */
pcv_status pcv_searcher_hidden_ids(pcv_searcher* s, int64_t* out_ids, int64_t cap, int64_t* out_n, int64_t* out_hidden_rows);

/* Updated items (update_db.rs upserts re-embedded items into item_embeddings; a source scan then needs their new vectors in the
 * index): every row whose id is ids[i] takes rows[i] as its vector, in place.  No rebuild: the rows stay where they are.
 *   - by id, like hide_ids: every source (rows staged under PCV_STAGING_SOURCE too), explicit-id and implicit-id segments
 *     (pcv_searcher_add_rows with ids == NULL, synthetic rows: id = id0 + row);
 *   - out_found (may be NULL): n bytes, out_found[i] = 1 iff some row carries ids[i]; out_rows (may be NULL): the rows
 *     rewritten.  Ids that match no row change nothing and are not remembered (unlike the hidden set);
 *   - exact: afterwards every search entry point returns bit for bit what a searcher built fresh from the updated rows returns
 *     (ids, scores, counts, order), for every kernel, screening copy, mid copy, metric, num_results and source filter.
 *     Positions, pcv_searcher_num_rows and _source_num_rows do not change; pcv_searcher_get_rows reads the new vector;
 *   - a new vector a fresh build would not make searchable (non-finite norm; zero norm under PCV_METRIC_COSINE) makes the row
 *     unsearchable; an unsearchable row that gets a valid vector becomes searchable.  A row whose id is hidden takes the new vector and stays hidden (unhiding returns it
 *     with the new vector);
 *   - all or nothing on bad input: duplicate ids in one call, n < 0, or NULL ids / rows with n > 0 give PCV_ERR_INVALID and
 *     change nothing; n == 0 does nothing.  Every device buffer is allocated before the first row is written (a failed
 *     allocation: PCV_ERR_DEVICE, nothing changed).  The rows go to the device through a bounded staging buffer, given back
 *     at the end; the library keeps no host copy.
 * Needs a finalized searcher (PCV_ERR_INVALID with pending rows) and no queued pass, as hide_ids does.  A mid copy that AUTO is
 * building beside the searches is waited for first.  update_blobs takes n blobs of dim*4 bytes each, as add_blobs does. */
pcv_status pcv_searcher_update_rows(pcv_searcher* s, const int64_t* ids, const float* rows, int64_t n, uint8_t* out_found,
                                    int64_t* out_rows);
pcv_status pcv_searcher_update_blobs(pcv_searcher* s, const int64_t* ids, const uint8_t* blobs, int64_t n, uint8_t* out_found,
                                     int64_t* out_rows);

/* Removed items (the reference drops items by rebuilding a source from SQLite, Searcher::rebuild_source, search.rs:58-79): every
 * row whose id is in ids[0..n) leaves the searcher, in every source (rows staged under PCV_STAGING_SOURCE too), explicit-id and
 * implicit-id segments alike.  No rebuild and no upload: the rows behind a removed row move down inside their segment, on the
 * device; source order and row order inside a source are kept.
 *   - exact: afterwards every search entry point returns bit for bit what a searcher built fresh from the remaining rows returns
 *     (ids, scores, counts, order) — the remaining rows added in the same source order and row order, with the same hidden set —,
 *     for every kernel, screening copy (off, bf16, int8, its 6-bit form), mid copy mode, metric, num_results (beyond 128 too)
 *     and source filter;
 *   - positions shift: pcv_searcher_num_rows, _source_num_rows and _get_rows count and read the remaining rows at their new
 *     global positions.  A sharded host must call pcv_searcher_set_shard_offset again on the ranks behind a rank that shrank;
 *   - not remembered: unlike the hidden set, removed ids are forgotten — a later pcv_searcher_add_rows with the same id is a new
 *     item.  The hidden set itself is left as it is (it persists independently of the rows);
 *   - the ids of the remaining rows never change: an implicit-id segment (ids == NULL, synthetic rows: id0 + row) that loses a
 *     row gets an id column on the device first (8 bytes per row, as an explicit-id segment carries);
 *   - a segment that loses all its rows is freed; a source that loses all its rows stays known with 0 rows, as after
 *     pcv_searcher_clear_source.  The tail room of a segment that shrank stays with it: the next add_rows to that source appends
 *     into it;
 *   - out_rows (may be NULL): the rows removed.  Duplicate ids and ids that match no row are allowed, as in hide_ids; n == 0
 *     does nothing.  NULL s, NULL ids with n > 0, n < 0, a view as s, pending rows (no finalize) or a queued pass give
 *     PCV_ERR_INVALID with nothing changed;
 *   - every row is found and every device buffer is allocated before the first row moves (a failed allocation: PCV_ERR_DEVICE,
 *     nothing changed).  The extra device memory of the call — one byte per row of flags, a bounce buffer of at most 2^18 rows,
 *     the id table — is given back at the end; an id column a segment got stays.  Never a second copy of a segment;
 *   - a mid copy that AUTO is building beside the searches is waited for first; a captured pass is dropped, so no replay runs
 *     over moved rows.  The narrow copies are packed again from the block of the first moved row of each segment on;
 *   - the call counts as a result-changing call for views: a view copies its rows again at its next call, removed ids then match
 *     nothing, and its hits carry the parent's new positions.
 * The dot-metric bound max_norm does not shrink (as after update_rows): results do not depend on it. */
pcv_status pcv_searcher_remove_ids(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_rows);

/* Views (a search restricted to a set of items: the items of a tag, of an author, "search again within these results"): a
 * read-only searcher handle that holds a compact device copy of the rows of `parent` whose id is in ids[0..n).
 *   - exact: every search of the view returns bit for bit what a searcher built fresh from only those rows returns (ids, scores,
 *     counts, order) — the rows added in the parent's source order and row order, with the parent's hidden set applied —, for
 *     every kernel, screening copy, metric, num_results and source filter;
 *   - every search entry point takes a view (pcv_searcher_search, _search_device, _search_device_begin[_dq] / _end,
 *     _search_sharded[_dq]), and so do _last_stats, _num_rows, _num_segments, _num_sources, _source_ids, _source_num_rows,
 *     _set_kernel, _set_candidate_capacity, _set_tuning, _repeat_without_guess.  A view keeps one source per parent source
 *     with matches, in parent order; the source filter behaves as on the parent (PCV_STAGING_SOURCE rows only for a search
 *     that names that source);
 *   - positions: a hit that carries one (pcv_hit.pos of _search_device, _begin / _end, the sharded exchange) carries the
 *     PARENT's position, shard offset included, so view lists of several ranks merge with pcv_merge_topk* like parent lists;
 *   - read-only: add / reserve / finalize / clear / replace / hide / unhide / update / remove / set_shard_offset /
 *     set_screening_copy / set_mid_copy and get_rows give PCV_ERR_INVALID on a view;
 *   - never stale: every parent call that may change a result (finalize, hide / unhide, update, remove, clear / replace source,
 *     set_screening_copy OFF, set_shard_offset) makes the view copy the rows again, from its stored id list and under the
 *     parent's lock, at the start of its next call.  Rows added to the parent later with an allowed id join the view after the
 *     parent's finalize (a view call fails with PCV_ERR_INVALID while the parent has cleared rows without a finalize).  A
 *     view must not be used concurrently with its parent;
 *   - a view has its own pass workspace and statistics: searching it does not change how the parent's next search runs.
 *     It keeps the screening copy its parent keeps, and a mid copy only if the parent's mode is PCV_MID_COPY_ON;
 *   - pcv_searcher_destroy(view) frees it; pcv_searcher_destroy(parent) gives PCV_ERR_INVALID while views of it are alive.
 * create_view needs a finalized parent without a queued pass.  Duplicate ids and ids that match no row are allowed; n == 0
 * makes an empty view.  NULL ids with n > 0, n < 0, or a view as the parent give PCV_ERR_INVALID; a failed allocation
 * PCV_ERR_DEVICE, with nothing left allocated. */
pcv_status pcv_searcher_create_view(pcv_searcher* parent, const int64_t* ids, int64_t n, pcv_searcher** out_view);
/* A view's state (after bringing it up to date with its parent): rows it holds (every source, PCV_STAGING_SOURCE included),
 * distinct ids of its allow list, how many times it was copied again from its parent, and the device time in ms of its
 * last copy.  Any pointer may be NULL.  PCV_ERR_INVALID for a searcher that is not a view. */
pcv_status pcv_searcher_view_stats(pcv_searcher* view, int64_t* out_rows, int64_t* out_ids, int32_t* out_refreshes, float* out_build_ms);

/* Which scan kernel pcv_searcher_search uses. AUTO: wave-reduction kernel for n_queries <= 4,
 * MFMA tile kernel otherwise (up to 128 queries per corpus pass at dim <= 640; 256 with the int8 screening copy at
 * dim <= 384; among the ranks of a sharded search a pass is 128 queries on every rank, whatever copies each holds).
 * More queries than one pass takes are searched in several passes.  Under AUTO a pass of 5..64 queries over rows of at most
 * 384 features streams the 6-bit form of the int8 copy where every selected segment has one (pcv_searcher_set_screening_copy),
 * re-screening its survivors against their int8 rows; MFMA pins the whole-int8 scan (same results, pcv_scan_stats.screen_bits 8). */
enum { PCV_KERNEL_AUTO = 0, PCV_KERNEL_WAVE = 1, PCV_KERNEL_MFMA = 2 };
pcv_status pcv_searcher_set_kernel(pcv_searcher* s, int kernel);

/* Tuning: rows per query the candidate lists of a pass hold at first (default 8192; 20 bytes each, 128
 * lists).  A pass that needs more repeats itself with larger lists (pcv_scan_stats.overflow_reruns). */
pcv_status pcv_searcher_set_candidate_capacity(pcv_searcher* s, uint32_t n_candidates);

/* Diagnostic / comparison switches of one searcher; results never depend on them.  `flags` replaces what the
 * environment variable PCV_SCAN_FLAGS gave the searcher at creation (bit meanings: csrc/scan.h, ScanParams::flags —
 * bit 0 plain instead of non-temporal corpus loads, bit 3 the 128-query tile instead of the block-holding int8 scan,
 * bit 5 no speculative start threshold, bit 7 no learned part of it, bits 8..15 workgroups per CU, ..., bit 29 never build or
 * stream the 6-bit screening copy, bit 31 let AUTO build it at any size instead of from 8M rows on), plus
 *   PCV_TUNE_FAIL_COPY_ALLOC : while set, every allocation of a screening copy is treated as failed (how the tests
 *                              reach the out-of-memory branches of pcv_searcher_finalize). */
enum { PCV_TUNE_FAIL_COPY_ALLOC = 1073741824 }; /* bit 30 */
pcv_status pcv_searcher_set_tuning(pcv_searcher* s, uint32_t flags);

/* Screening copy: next to the f32 rows a segment can hold the same rows, already scaled, in a narrow form that
 * only the coarse screen reads; the f32 rows are then read for the rows that pass it (fine screen) and for the
 * finalists (exact ranking), so results are identical — the screens are certified bounds, not approximations.
 *   PCV_SCREEN_COPY_BF16 : the operand of the bf16 MFMA screen ready-made, 2 bytes per feature (+50 % HBM);
 *                          coarse margin 2^-8 relative
 *   PCV_SCREEN_COPY_INT8 : rows quantised per row to int8, 1 byte per feature + 4 bytes per row (+25 % HBM), screened
 *                          by an exact integer dot product with the quantised query; coarse margin ~0.024 in cosine
 *                          for 384-d unit rows (certified per row and query from the quantisation steps): more rows
 *                          reach the fine screen, a quarter of the bytes are streamed; dimensions up to 1024
 *   PCV_SCREEN_COPY_AUTO (default): INT8 (BF16 for rows wider than 1024 features), built at finalize; given up — for good, on this searcher — when an
 *                          allocation for rows or for a copy fails (the f32 rows are scanned then).  From 8M rows on (rows of at most
 *                          384 features) AUTO also keeps a 6-bit form of the int8 copy, 3/4 of a byte per feature + 16 bytes per
 *                          32 rows, screened with an L2 bound (pcv_searcher_set_kernel) — if a tenth of the device, at least
 *                          4 GB, stays free after it.  It is the first copy to give way when an allocation for rows or for a
 *                          copy fails, it is freed before AUTO builds a mid copy, and when the mode leaves AUTO
 *   PCV_SCREEN_COPY_OFF  : never built; existing copies are freed
 * BF16 / INT8 asked for explicitly: a failed copy allocation is an error at finalize.  Takes effect at the next
 * finalize (OFF: at once).  100M x 384: 153.6 GB of rows + 38.4 GB (INT8) or 76.8 GB (BF16); AUTO: + 28.8 GB for the 6-bit form. */
enum { PCV_SCREEN_COPY_OFF = 0, PCV_SCREEN_COPY_BF16 = 1, PCV_SCREEN_COPY_AUTO = 2, PCV_SCREEN_COPY_INT8 = 3 };
pcv_status pcv_searcher_set_screening_copy(pcv_searcher* s, int mode);

/* Mid copy: a third, optional representation of the rows — 16-bit fixed point per row, ROW-MAJOR (2 bytes per feature + 4 per
 * row: 76.8 GB for 100M x 384) — read by the fine screen in front of the f32 rows.  Worth its memory where the f32 rows of the
 * coarse (int8) screen's survivors are a visible share of a pass: corpora that let thousands of rows per query through
 * (clustered embeddings), wide rows, small shards.  A coarse survivor then costs 2 contiguous bytes per feature instead of
 * one 128-byte cache line per 4 features of the blocked f32 layout, and only rows within ~1e-4 of the running threshold go on
 * to their f32 row.  Results are identical with and without it (a certified bound, like the other screens).
 *   PCV_MID_COPY_AUTO (default): built by a search call after 2 passes in a row over int8 copies in which the coarse screen let
 *                        more than 4096 rows per query through, or in which the survivors' f32 rows came to more than 1/25 of
 *                        the bytes streamed — if the memory is there (4 GB stay free); dropped again, before the screening
 *                        copies, when an allocation for rows or for a screening copy fails
 *   PCV_MID_COPY_ON    : built at the next finalize (an allocation failure is an error)
 *   PCV_MID_COPY_OFF   : never built; an existing one is freed */
enum { PCV_MID_COPY_OFF = 0, PCV_MID_COPY_AUTO = 1, PCV_MID_COPY_ON = 2 };
pcv_status pcv_searcher_set_mid_copy(pcv_searcher* s, int mode);
/* AUTO builds the mid copy BESIDE the searches (a stream and a helper thread of its own): the search call that decides to
 * build it returns like any other, and so do the calls after it, without the copy, until it is complete — while it is being
 * built they share the memory system with the build.  This call waits for such a build to finish (a benchmark that wants
 * the steady state; nothing needs it for correctness).  Returns at once when nothing is under way. */
pcv_status pcv_searcher_wait_background(pcv_searcher* s);

/* Most hits ONE PASS over the rows ranks per query.  pcv_searcher_search takes any num_results (search.rs:157-182 has no limit;
 * the reference's callers ask for 10 and 20, perceive-cli's --num-results is user input): beyond this many it goes over the rows
 * again for the next PCV_MAX_RESULTS below the last hit of the pass before, and so on — every pass exact, results as from one
 * ranking.  The entry points that exchange fixed-size hit lists (pcv_searcher_search_device*, pcv_searcher_search_sharded,
 * pcv_merge_topk*) take at most this many. */
enum { PCV_MAX_RESULTS = 128 };

/* Searcher::search_vector (search.rs:157-182), batched over `n_queries` query vectors.
 *   queries      [n_queries][dim] f32
 *   source_ids   sources to search (search.rs:166 filter): NULL = all sources (n_sources ignored);
 *                non-NULL = exactly the n_sources listed ones, so n_sources = 0 matches nothing,
 *                like `sources.contains(..)` on an empty slice
 *   k            num_results
 *   out_ids      [n_queries][k] item ids, best first
 *   out_scores   [n_queries][k] cosine (COSINE) or reference distance (DOT)
 *   out_counts   [n_queries] entries actually filled (< k when fewer valid rows exist)
 * Result order: COSINE descending cosine, DOT ascending distance; ties -> lower global position.
 * Rows whose norm is 0 or not finite (cosine undefined; the reference would yield NaN and panic at
 * search.rs:179) are never returned.  Exactness: the returned set is the exact top-k under the
 * canonical f64 score (DESIGN.md §canonical ranking), not an approximation.
 * Magnitudes (DESIGN.md §4 "Magnitudes").  A result differs from the canonical one only together with an error status.
 * COSINE: exact for every row and query whose squared norm (f64, feature order) lies in [2^-126, inf), whatever the magnitudes:
 * subnormal features, norms up to sqrt(dim) * FLT_MAX.  DOT: rows and queries enter the f32 screens unnormalised; per quantity —
 *   rows         exact for every row of finite squared norm.  The quantisation scales of the screening copies, 127 / max|x_i| of a
 *                block and 32766 / max|x_i| of a row, are capped at 2^100: no feature is too small.
 *   queries      a query with a non-zero feature whose largest |q_i| is below 2^-120 is refused with PCV_ERR_INVALID (the message
 *                names s_q = 127 / max|q_i|, which is inf below 3.73e-37);
 *   |q| max|x|   max|x| the LARGEST row norm the searcher has held (one huge row widens the screens' margins, multiples of this
 *                product, for every row): a query for which it is non-zero and outside [2^-120, 2^127] is refused with
 *                PCV_ERR_INVALID (the message names unit).  This covers every case in which a single product q_i x_i, and so an
 *                f32 accumulator, could pass FLT_MAX.
 * Both refusals come from the call that brings the query (pcv_searcher_search, _search_range, _search_device, the ranked calls and
 * _search_compound) before anything is queued.  The calls of the sharded protocol with host queries
 * (pcv_searcher_search_device_begin, _search_sharded) refuse by the query alone (s_q): max|x| differs from rank to rank, and among
 * ranks only a condition all of them evaluate alike may refuse; |q| max|x| is the caller's to keep there.  Queries that are
 * already on the device (pcv_searcher_search_device_begin_dq, _search_sharded_dq, the like_item calls) are not read on the host
 * at all: there the whole query envelope is the caller's to keep.  The threshold of the int8 and 6-bit screens in units of the
 * quantised query, up to 127 sqrt(dim) max|x| whatever the query's scale, is capped at FLT_MAX in the kernels (exact).  Inside it
 * rows and queries may differ by any power of two (tested: 2^-60 x 2^-60 up to 2^40 x 2^40, one row 2^40 above and one block
 * 2^40 below the rest, blocks and whole segments of features 2^-122).  An all-zero query and a query with a value that is not finite
 * are answered as before (every row scores 0; no hits). */
pcv_status pcv_searcher_search(pcv_searcher* s, const float* queries, int n_queries,
                               const int64_t* source_ids, int n_sources, int k, int64_t* out_ids,
                               float* out_scores, int* out_counts);

/* Range search: every item within a score bound, in one pass over the rows.
 * Per query q with bound bounds[q], the in-range rows are the searchable rows (in the selected sources, not hidden, with a
 * canonical score: as in pcv_searcher_search) whose REPORTED f32 score passes the test
 *   COSINE : score >= bounds[q]        DOT : distance <= bounds[q]
 * where the reported score is the value pcv_searcher_search would return for that row: (float)c for cosine, max(0, 1 - c/dim) in
 * f32 for the dot metric, c the canonical f64 score.  Results are the in-range rows in the canonical order —
 * descending c, ties -> lower global position —, at most max_results per query; out_more[q] is 1 exactly when more in-range rows
 * exist than were returned.  This is what pcv_searcher_search returns with num_results = the number of searchable rows, cut after
 * the last hit that passes the test: ids and scores agree bit for bit.
 *   queries, source_ids, n_sources : as in pcv_searcher_search (NULL = all sources; an empty list matches nothing)
 *   bounds       [n_queries]; infinite bounds are legal and mean everything or nothing; a negative DOT bound matches nothing
 *   max_results  1 .. PCV_MAX_RANGE_ROWS
 *   out_ids      [n_queries][max_results], -1 behind the results;  out_scores likewise, NaN behind them (may be NULL)
 *   out_counts   [n_queries] results returned;  out_more [n_queries] (may be NULL)
 * A NULL searcher, NULL queries, n_queries <= 0, NULL bounds, a NaN bound or max_results outside its range give PCV_ERR_INVALID
 * before any device work; a searcher with pending rows fails as in pcv_searcher_search.
 * The scan runs with thresholds that are fixed from the start (DESIGN.md §4 "Range search"), so a call costs one pass per group
 * of queries — two if a candidate list was too short (pcv_scan_stats.overflow_reruns) — however many rows match; the settings of
 * set_kernel, set_screening_copy, set_mid_copy, set_tuning and set_candidate_capacity hold, pcv_searcher_last_stats describes
 * the call, and a view searches its own rows.  If the pass of a query lists more than PCV_MAX_RANGE_ROWS rows the call returns
 * PCV_ERR_UNSUPPORTED, naming the query and the count, before any list of that size is allocated; the searcher stays usable.  For
 * such a bound use pcv_searcher_search, which pages through the rows PCV_MAX_RESULTS at a time.
 * Memory: the lists and the result block of a call grow with the rows its passes list — up to 0.4 GB on the device and 0.8 GB of
 * pinned host memory for the widest bounds.  What exceeds 64 MB is released when the call returns; smaller blocks are kept for
 * the next call.
 * The sharded and device-list entry points (pcv_searcher_search_device*, pcv_searcher_search_sharded*, pcv_merge_topk*) exchange
 * fixed-size lists and have no range form. */
enum { PCV_MAX_RANGE_ROWS = 16777216 }; /* 2^24: the limit pcv_searcher_search already puts on num_results */
pcv_status pcv_searcher_search_range(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                     const float* bounds, int64_t max_results, int64_t* out_ids, float* out_scores,
                                     int64_t* out_counts, uint8_t* out_more);

/* Distinct results: the exact top-k with near-duplicates collapsed on the device.
 * Per query, L is the ranked list pcv_searcher_search returns (canonical score, ties -> lower position; the searchable rows of the
 * selected sources: hidden rows and a view's restriction apply as everywhere).  L is walked best first with an empty kept set: a
 * row is KEPT iff dup(row, j) is false for every kept row j, otherwise it is dropped and counted for the best-ranked kept row it
 * duplicates; the walk stops right after the num_results-th kept row, or after `pool` entries of L.
 *   dup(a, b) = canonical cosine of the two stored f32 rows >= (double)threshold
 * — f64, products exact, sums in feature order, for BOTH metrics: near-duplicate is a scale-free notion and the
 * rows of a dot-metric corpus differ in norm.  A row without a cosine (zero or non-finite norm) duplicates nothing.
 *   threshold    in (-1, 1]; at exactly 1 even equal rows collapse only where the f64 quotient rounds to 1 or above (about two rows
 *                in three): use the f32 below 1 for "exact copies"
 *   pool         num_results .. PCV_MAX_DISTINCT_POOL: entries of L the walk may examine
 *   out_ids      [n_queries][num_results] the kept rows, best first, -1 behind them;  out_scores likewise, NaN behind them (may be
 *                NULL) — ids and scores are bit for bit what pcv_searcher_search reports for those rows
 *   out_counts   [n_queries] rows kept
 *   out_similar  [n_queries][num_results] examined rows dropped in favour of this hit, 0 behind the results (may be NULL)
 *   out_examined [n_queries] entries of L examined (may be NULL)
 *   out_more     [n_queries] 1: the walk stopped at `pool` with fewer than num_results kept and L had more rows (may be NULL)
 * A NULL searcher, no queries, num_results outside [1, PCV_MAX_RESULTS], pool outside [num_results, PCV_MAX_DISTINCT_POOL] or a
 * threshold that is NaN or outside (-1, 1] give PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in
 * pcv_searcher_search.  A call makes at most ceil(pool / PCV_MAX_RESULTS) passes per group of queries (DESIGN.md §4 "Distinct
 * results") — each followed by a select step on the device; the host reads back counters only — and one short pass more where
 * out_more has to be decided.  Works on views (a view walks its own rows).
 * Not in scope: a sharded form (the walk needs the rows of every shard's hits) and device-resident output. */
enum { PCV_MAX_DISTINCT_POOL = 4096 };
pcv_status pcv_searcher_search_distinct(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                        int num_results, float threshold, int pool, int64_t* out_ids, float* out_scores,
                                        int32_t* out_counts, int32_t* out_similar, int32_t* out_examined, uint8_t* out_more);

/* Grouped results: the exact top-k collapsed by a stored group key per item ("which k documents are closest, when every document is
 * stored as several rows").
 *
 * The group table is state of a searcher: an open-addressed hash table on the device from item id to group key.
 *   - A group key is any int64 >= 0; PCV_NO_GROUP (-1) means "no group".  An id without an entry, or with PCV_NO_GROUP, is a
 *     group of its own — and such a singleton is the ROW, not the id: two ungrouped rows that share an item id do not collapse,
 *     two rows that share an id with a group do (they share the group).
 *   - Keyed by id, not by row: hide, update, remove, replace_source and the screening copies know nothing of it, and an entry
 *     SURVIVES pcv_searcher_remove_ids, clear_source and replace_source — an id that comes back has its group again.  Only
 *     pcv_searcher_clear_groups forgets (everything: the searcher is then as created, counters included).
 *   - It lives with the root searcher.  A view reads its parent's table at call time (a set_groups on the parent is seen by the
 *     view's next search); the three mutators on a view fail as every change of a view does.
 *   - Memory: 16 bytes per slot, slots a power of two >= 2 * entries, 1024 at least: 100M grouped ids take 2^28 slots, 4.3 GB.
 *     While a set_groups call runs it holds 4 bytes per slot more, and up to 2^22 ids of the batch at a time (84 MB).
 * pcv_searcher_set_groups: an upsert of (ids[i], groups[i]), i < n.  groups[i] == PCV_NO_GROUP ungroups the id (its entry stays;
 *   there are no tombstones); any other negative group, a NULL list with n > 0 or n < 0 give PCV_ERR_INVALID before any device
 *   work.  Of an id that occurs more than once in a batch the LAST occurrence holds.  A batch is one growth decision: the table is
 *   sized for entries + n before the batch goes in (ids already present count twice there: growth may come one batch early).
 *   More than 2^30 entries give PCV_ERR_UNSUPPORTED before anything is allocated; a failed allocation (PCV_ERR_DEVICE) leaves
 *   the table as it was.
 * pcv_searcher_get_groups: out_groups[i] = the group of ids[i], PCV_NO_GROUP if it has none.  Works on a view (the parent's table).
 * pcv_searcher_group_stats: ids with a group >= 0 / occupied slots / capacity / growths by rehash since creation (or the last
 *   clear_groups) / device time of the last set_groups, growth included (hipEvent). */
#define PCV_NO_GROUP (-1)
typedef struct pcv_group_stats {
    int64_t ids;
    int64_t entries;
    int64_t slots;
    int32_t rehashes;
    float last_set_ms;
} pcv_group_stats;
pcv_status pcv_searcher_set_groups(pcv_searcher* s, const int64_t* ids, const int64_t* groups, int64_t n);
pcv_status pcv_searcher_clear_groups(pcv_searcher* s);
pcv_status pcv_searcher_get_groups(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_groups);
pcv_status pcv_searcher_group_stats(pcv_searcher* s, pcv_group_stats* out);
/* pcv_searcher_search_grouped.  Per query, L is the ranked list pcv_searcher_search returns (canonical score, ties -> lower
 * position; the searchable rows of the selected sources: hidden rows and a view's restriction apply as everywhere).  L is walked
 * best first and only its first `pool` entries are examined: a row is KEPT iff no kept row has its group, otherwise it is COLLAPSED
 * into that kept row; the walk stops right after the num_results-th kept row, or at the end of the examined prefix.  A kept row is
 * therefore the best-scoring member of its group among the selected rows, and with out_more == 0 the kept rows are the
 * num_results best groups of the corpus by best member.
 *   pool          num_results .. PCV_MAX_GROUPED_POOL: entries of L the walk may examine
 *   out_ids       [n_queries][num_results] the kept rows, best first, -1 behind them;  out_scores likewise, NaN behind them (may be
 *                 NULL) — ids and scores are bit for bit what pcv_searcher_search reports for those rows
 *   out_groups    [n_queries][num_results] the group key of each kept row, PCV_NO_GROUP for an ungrouped row and behind the results
 *                 (may be NULL)
 *   out_counts    [n_queries] rows kept
 *   out_collapsed [n_queries][num_results] examined rows collapsed into this hit, 0 behind the results (may be NULL)
 *   out_examined  [n_queries] entries of L examined (may be NULL)
 *   out_more      [n_queries] 1: the walk stopped at `pool` with fewer than num_results kept and L had another row (may be NULL)
 * A NULL searcher, no queries, num_results outside [1, PCV_MAX_RESULTS] or pool outside [num_results, PCV_MAX_GROUPED_POOL] give
 * PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in pcv_searcher_search.  An empty table is legal:
 * the result is the plain top-num_results.  A call makes at most ceil(pool / PCV_MAX_RESULTS) passes per group of queries, each
 * followed by a select step on the device whose cost is fixed (DESIGN.md §4 "Grouped results"), and one short pass more where
 * out_more has to be decided.  Known limit: a large group near a query costs passes — a 500-row document costs four; `pool`
 * bounds that and out_more reports it.
 * Group-aware neighbours, matches and duplicate pairs: pcv_searcher_neighbors_grouped, _match_grouped, _find_duplicates_grouped below.
 * Not in scope: group-aware search by example, a sharded form, device-resident output, more than one member per group. */
enum { PCV_MAX_GROUPED_POOL = 4096 };
pcv_status pcv_searcher_search_grouped(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, int pool, int64_t* out_ids, float* out_scores, int64_t* out_groups,
                                       int32_t* out_counts, int32_t* out_collapsed, int32_t* out_examined, uint8_t* out_more);

/* Item values and filtered search: a stored int64 per item (a time stamp, a price, a version) and exact search under a range
 * predicate on it ("the best matches among the items modified since last week") — what vector stores call metadata filtering.
 *
 * The value table is state of a searcher, a second instance of the table the groups live in, and its contract is that table's:
 *   - A value is any int64 but PCV_NO_VALUE (INT64_MIN), which means "no value": negative time stamps, INT64_MAX and
 *     INT64_MIN + 1 are values like any other.
 *   - Keyed by id, not by row: hide, update, remove, replace_source and the screening copies know nothing of it, and an entry
 *     SURVIVES pcv_searcher_remove_ids, clear_source and replace_source — an id that comes back has its value again.  Only
 *     pcv_searcher_clear_values forgets (everything: the table is then as created, counters included).  Two rows that share an id
 *     share its value.
 *   - It lives with the root searcher.  A view reads its parent's table at call time; the two mutators on a view fail as every
 *     change of a view does.
 *   - Memory: 16 bytes per slot, slots a power of two >= 2 * entries, 1024 at least; 4 bytes per slot more and up to 2^22 ids of
 *     the batch at a time while a set_values call runs.
 * pcv_searcher_set_values: an upsert of (ids[i], values[i]), i < n.  values[i] == PCV_NO_VALUE unsets the id (its entry stays;
 *   there are no tombstones).  A NULL list with n > 0 or n < 0 give PCV_ERR_INVALID before any device work.  Of an id that occurs
 *   more than once in a batch the LAST occurrence holds.  A batch is one growth decision: the table is sized for entries + n before
 *   the batch goes in.  More than 2^30 entries give PCV_ERR_UNSUPPORTED before anything is allocated; a failed allocation
 *   (PCV_ERR_DEVICE) leaves the table as it was.  There is no host sort: the cost is the upload and two launches per 2^22 ids.
 * pcv_searcher_get_values: out_values[i] = the value of ids[i], PCV_NO_VALUE if it has none.  Works on a view (the parent's table).
 * pcv_searcher_value_stats: ids with a value / occupied slots / capacity / growths by rehash since creation (or the last
 *   clear_values) / device time of the last set_values, growth included (hipEvent).
 *
 * A PREDICATE is (lo, hi, flags) over the value of a row's id: a row passes iff its id has a value v with lo <= v <= hi.
 *   PCV_WHERE_UNSET_PASSES  rows whose id has no value pass too (without it they never do)
 *   PCV_WHERE_OUTSIDE       the interval test is negated for rows that have a value (unset rows still follow the other bit only)
 * lo > hi is legal: the empty interval.  Any other flag bit gives PCV_ERR_INVALID.
 * pcv_searcher_count_where: *out_rows = rows of the selected sources that pass, *out_searchable = those of them a search could
 *   return (hidden and unsearchable rows excluded); either may be NULL.  The source filter is pcv_searcher_search's
 *   (PCV_STAGING_SOURCE rows only where that source is named); on a view the view's own rows are counted.  Exact: one kernel over
 *   the ids of every selected segment, integer sums on the device, one 16-byte download.  Pending rows fail as in a search. */
#define PCV_NO_VALUE (INT64_MIN)
enum { PCV_WHERE_UNSET_PASSES = 1, PCV_WHERE_OUTSIDE = 2 };
typedef struct pcv_value_stats {
    int64_t ids;
    int64_t entries;
    int64_t slots;
    int32_t rehashes;
    float last_set_ms;
} pcv_value_stats;
pcv_status pcv_searcher_set_values(pcv_searcher* s, const int64_t* ids, const int64_t* values, int64_t n);
pcv_status pcv_searcher_clear_values(pcv_searcher* s);
pcv_status pcv_searcher_get_values(pcv_searcher* s, const int64_t* ids, int64_t n, int64_t* out_values);
pcv_status pcv_searcher_value_stats(pcv_searcher* s, pcv_value_stats* out);
pcv_status pcv_searcher_count_where(pcv_searcher* s, const int64_t* source_ids, int n_sources, int64_t lo, int64_t hi, uint32_t flags,
                                    int64_t* out_rows, int64_t* out_searchable);
/* pcv_searcher_search_where: for BROAD predicates.  Per query, L is the ranked list pcv_searcher_search returns (canonical score,
 * ties -> lower position; the searchable rows of the selected sources: hidden rows and a view's restriction apply as everywhere).  L
 * is walked best first and only its first `pool` entries are examined: a row is KEPT iff it passes; the walk stops right after the
 * num_results-th kept row, or at the end of the examined prefix.  With out_more == 0 the kept rows are the exact top num_results
 * of the passing rows.
 *   pool          num_results .. PCV_MAX_WHERE_POOL: entries of L the walk may examine
 *   out_ids       [n_queries][num_results] the kept rows, best first, -1 behind them;  out_scores likewise, NaN behind them (may be
 *                 NULL) — ids and scores are bit for bit what pcv_searcher_search reports for those rows
 *   out_values    [n_queries][num_results] the value of each kept row, PCV_NO_VALUE for an unset row that passed and behind the
 *                 results (may be NULL)
 *   out_counts    [n_queries] rows kept
 *   out_examined  [n_queries] entries of L examined (may be NULL)
 *   out_more      [n_queries] 1: the walk stopped at `pool` with fewer than num_results kept and L had another row (may be NULL)
 * A NULL searcher, no queries, num_results outside [1, PCV_MAX_RESULTS], pool outside [num_results, PCV_MAX_WHERE_POOL] or an
 * unknown flag bit give PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in pcv_searcher_search.  An
 * empty table is legal.  A call makes at most ceil(pool / PCV_MAX_RESULTS) passes per group of queries, each followed by a select
 * step on the device whose cost is fixed, and one short pass more where out_more has to be decided.  Known limit: a predicate that
 * passes a fraction p of the rows near a query needs about num_results / p examined entries, and `pool` caps that at 4096 —
 * p = 0.25 % for ten results.  Below that use pcv_searcher_create_view_where; pcv_searcher_count_where reports p.
 * Not in scope: the predicate inside the scan, a sharded form, several values per item, float values. */
enum { PCV_MAX_WHERE_POOL = 4096 };
pcv_status pcv_searcher_search_where(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                     int num_results, int pool, int64_t lo, int64_t hi, uint32_t flags, int64_t* out_ids, float* out_scores,
                                     int64_t* out_values, int32_t* out_counts, int32_t* out_examined, uint8_t* out_more);
/* pcv_searcher_create_view_where: for SELECTIVE predicates.  A view (see pcv_searcher_create_view) in every respect — the same handle
 * type, every search entry point takes it, positions are the parent's, read-only, the copy kind its parent keeps — whose rows are
 * those whose id passes the predicate: there is no stored id list (pcv_searcher_view_stats reports 0 ids), the rows are selected
 * on the device from the parent's value table, id columns and implicit ids alike, with no host work per id.  It is stale, and copies
 * its rows again at its next call, when the parent changed as for every view OR the parent's value table changed (set_values with
 * n > 0, clear_values); views made by pcv_searcher_create_view never look at the value table.  Unknown flag bits, a NULL argument or
 * a view as the parent give PCV_ERR_INVALID; a failed allocation PCV_ERR_DEVICE, with nothing left allocated. */
pcv_status pcv_searcher_create_view_where(pcv_searcher* parent, int64_t lo, int64_t hi, uint32_t flags, pcv_searcher** out_view);

/* Diverse results: exact greedy maximal marginal relevance (MMR), selected on the device — the graded form of what
 * pcv_searcher_search_distinct and pcv_searcher_search_grouped do all-or-nothing.  Per query:
 *   L      the ranked list pcv_searcher_search returns (canonical score, ties -> lower position; the searchable rows of the selected
 *          sources: hidden rows and a view's restriction apply as everywhere; a row without a canonical score never appears).
 *   P      the pool: the first min(pool, |L|) entries of L.  The RANK of an entry is its index in L, from 0.
 *   rel_i  relevance, from the canonical f64 score c_i: cosine metric c_i; dot metric c_i / (double)dim, one f64 division (the
 *          similarity whose complement that metric reports as distance, without the clamp).
 *   div_i  redundancy: the largest cos(i, j) over the rows j picked so far, 0 while nothing is picked.  cos is the canonical cosine
 *          of the two stored f32 rows for BOTH metrics, exactly the dup arithmetic of pcv_searcher_search_distinct — f64, products
 *          exact, sums in feature order — and symmetric bit for bit.  A pair without a cosine (a norm that is zero or not finite)
 *          counts as cos = 0.
 *   m_i    marginal value: with l = (double)lambda and u = 1.0 - l in f64,  m_i = fl(fl(l * rel_i) - fl(u * div_i)) — three separate
 *          roundings, no fused multiply-add.
 * The walk, num_results times or until P is used up: pick the entry of P not yet picked with the largest m_i, ties -> lower rank.
 * The first pick is therefore always L[0], and lambda = 1 gives the plain top-num_results.
 *   lambda       in [0, 1]: 1 is relevance alone, 0 is diversity alone (after L[0])
 *   pool         num_results .. PCV_MAX_DIVERSE_POOL: entries of L the walk chooses among
 *   out_ids      [n_queries][num_results] the picks in pick order, -1 behind them
 *   out_scores   likewise, NaN behind the picks (may be NULL): the reported f32 score, bit for bit what pcv_searcher_search gives
 *                for that row
 *   out_marginal [n_queries][num_results] f64: m of each pick at the moment it was picked, NaN behind the picks (may be NULL)
 *   out_ranks    [n_queries][num_results] rank of each pick in L, -1 behind the picks (may be NULL)
 *   out_counts   [n_queries] picks made = min(num_results, |P|)
 *   out_examined [n_queries] |P| (may be NULL)
 *   out_exact    [n_queries] 1: the picks are provably those the same walk over ALL of L would make (may be NULL).  A 1 is a proof,
 *                a 0 is no disproof.  Set in exactly two cases: (a) |P| < pool — the list ended inside the pool; (b) every pick has
 *                m_t > fl(fl(l * rel_last) + fl(u * d0)), rel_last the relevance of P's last entry and d0 = 1 + 2^-40: every row
 *                outside P has rel <= rel_last, no canonical cosine falls below -d0 (the f64 quotient may round a few ulps past
 *                -1), and rounding is monotone, so no outside row can reach m_t at any step.  (b) needs no extra pass; where
 *                |L| == pool exactly and (b) fails the flag is 0.
 * A NULL searcher, no queries, num_results outside [1, PCV_MAX_RESULTS], pool outside [num_results, PCV_MAX_DIVERSE_POOL] or a
 * lambda that is NaN or outside [0, 1] give PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in
 * pcv_searcher_search.  A call makes ceil(pool / PCV_MAX_RESULTS) passes per group of queries (fewer where every list ends
 * sooner: nothing else stops a query early), each followed by a collect step that gathers the pass's rows, and one select launch
 * per group (DESIGN.md §4 "Diverse results"); the host reads back the result block and one record per query.  The gathered rows
 * take pool x padded row bytes per query, at most 512 MB a group: wide rows and large pools take fewer queries a group, and what
 * exceeds 64 MB is given back when the call ends.  Works on views (a view walks its own rows).
 * Not in scope: a sharded form (the walk needs the rows of every shard's hits), device-resident output, a duplicate threshold
 * combined with lambda, and group-aware diversity. */
enum { PCV_MAX_DIVERSE_POOL = 4096 };
pcv_status pcv_searcher_search_diverse(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, float lambda, int pool, int64_t* out_ids, float* out_scores,
                                       double* out_marginal, int32_t* out_ranks, int32_t* out_counts, int32_t* out_examined,
                                       uint8_t* out_exact);

/* Boosted results: the exact top-k under score plus a prior from the item's value ("the best matches, with recent items ranked a
 * little higher") — the graded form of what pcv_searcher_search_where does all-or-nothing, re-ranked on the device, with a
 * certificate that says when the answer is that of the whole list.  Per query:
 *   L      the ranked list pcv_searcher_search returns (canonical f64 score, ties -> lower position; the searchable rows of the
 *          selected sources: hidden rows and a view's restriction apply as everywhere).  The RANK of an entry is its index in L.
 *   rel_i  relevance, exactly as in diverse results: cosine metric c_i; dot metric c_i / (double)dim, one f64 division.
 *   b_i    boost(v), piecewise linear in the value v of the row's id (pcv_searcher_set_values; a view reads its parent's table):
 *            no value                 unset_boost
 *            v <= knot_values[0]      knot_boosts[0];      v >= knot_values[n-1]   knot_boosts[n-1]
 *            otherwise, with knot_values[j] <= v < knot_values[j+1]:
 *              num = (double)(uint64_t)(v - knot_values[j]), den = (double)(uint64_t)(knot_values[j+1] - knot_values[j]) — both
 *              differences in wrapping 64-bit arithmetic, so they are exact for any pair of int64 —, t = num / den and
 *              b = fl(knot_boosts[j] + fl(t * fl(knot_boosts[j+1] - knot_boosts[j]))): separate roundings, no fused multiply-add;
 *              then b is clamped into [min, max] of the segment's two knot boosts (t can round to 1 and the sum land an ulp past
 *              the knot: the clamp keeps b_max below a true bound).
 *          A step function is two knots at v and v + 1; one knot is a constant.
 *   m_i    the boosted score fl(rel_i + b_i).  ORDER: m descending, ties -> lower rank in L.
 *   b_max  the maximum over all knot_boosts and unset_boost.
 * The walk: the examined prefix of L grows in steps of PCV_MAX_RESULTS entries (the last step shorter, so that the prefix never
 * exceeds `pool`).  After each step the KEPT rows are the first min(num_results, examined) entries of the prefix in the order above,
 * and the walk ends at the first step where one of these holds:
 *   (a) the list delivered fewer entries than the step asked for — it ended: exact = 1;
 *   (b) num_results rows are kept and m_k >= fl(rel_last + b_max), m_k the last kept row's m and rel_last the relevance of the last
 *       examined entry: exact = 1.  A row outside the prefix has rel <= rel_last and b <= b_max, rounding is monotone, so its m is
 *       at most the bound; it also has a higher rank than every examined row, so it loses a tie: >= suffices;
 *   (c) examined == pool: exact = 0.  Where |L| == pool exactly and (b) fails the flag is 0, as in diverse results.
 * A 1 is a proof, a 0 is no disproof.
 *   pool          num_results .. PCV_MAX_BOOST_POOL: entries of L the walk may examine
 *   boost         n_knots in 1 .. PCV_MAX_BOOST_KNOTS; knot_values strictly increasing, none PCV_NO_VALUE; every boost finite
 *   out_ids       [n_queries][num_results] the kept rows, best first, -1 behind them
 *   out_scores    likewise, NaN behind (may be NULL): the plain f32 score, bit for bit what pcv_searcher_search reports for the row
 *   out_boosted   [n_queries][num_results] f64: m of each kept row, NaN behind (may be NULL)
 *   out_values    [n_queries][num_results] the value of each kept row, PCV_NO_VALUE for an unset row and behind (may be NULL)
 *   out_ranks     [n_queries][num_results] rank of each kept row in L, -1 behind (may be NULL)
 *   out_counts    [n_queries] rows kept
 *   out_examined  [n_queries] entries of L examined (may be NULL)
 *   out_exact     [n_queries] the certificate (may be NULL)
 * A NULL searcher, no queries, num_results outside [1, PCV_MAX_RESULTS], pool outside [num_results, PCV_MAX_BOOST_POOL], a NULL
 * boost, n_knots outside [1, PCV_MAX_BOOST_KNOTS], knot values not strictly increasing or equal to PCV_NO_VALUE, or a boost that is
 * not finite give PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in pcv_searcher_search.  An empty
 * value table is legal: every row then gets unset_boost, and the result is the plain top-k.  No selected rows give the blank answer
 * with exact = 1.  A call makes at most ceil(pool / PCV_MAX_RESULTS) passes per group of queries, each followed by a select step on
 * the device whose cost is fixed (DESIGN.md §4 "Boosted results"); there is no extra pass.  Works on views.
 * Not in scope: a sharded form, device-resident output, a predicate combined with the boost, boosts from the group table, float
 * values. */
enum { PCV_MAX_BOOST_KNOTS = 16, PCV_MAX_BOOST_POOL = 4096 };
struct pcv_boost {
    int32_t n_knots;                          /* 1 .. PCV_MAX_BOOST_KNOTS */
    int64_t knot_values[PCV_MAX_BOOST_KNOTS]; /* strictly increasing; none is PCV_NO_VALUE */
    double knot_boosts[PCV_MAX_BOOST_KNOTS];  /* finite */
    double unset_boost;                       /* finite: the boost of an item without a value */
};
typedef struct pcv_boost pcv_boost;
pcv_status pcv_searcher_search_boosted(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                                       int num_results, int pool, const pcv_boost* boost, int64_t* out_ids, float* out_scores,
                                       double* out_boosted, int64_t* out_values, int32_t* out_ranks, int32_t* out_counts,
                                       int32_t* out_examined, uint8_t* out_exact);

/* Compound queries: the exact top-k under "all of these", "any of these" and "but not like that" — the three requests that are not
 * linear in the row and so are no single query vector (a sum A + B is topped by rows excellent for one part and indifferent to the
 * other; q - w n pushes down every row in proportion to its similarity to n, related to n or not).  A compound has W wanted vectors
 * (1 .. PCV_MAX_COMPOUND_PARTS) and A avoided vectors (0 .. PCV_MAX_COMPOUND_PARTS), the call a mode and an avoid_weight w >= 0 (f32,
 * widened to f64).  For a searchable row x of the selected sources (hidden rows and a view's restriction apply as everywhere):
 *   rel_j(x)  relevance of x under vector j, exactly as in boosted and diverse results: with c_j the canonical f64 score of the pair
 *             (the bits pcv_searcher_search ranks by), cosine metric c_j; dot metric c_j / (double)dim, one f64 division.
 *   base(x)   PCV_COMPOUND_ALL: min over the wanted vectors of rel_j(x); PCV_COMPOUND_ANY: max.
 *   pen(x)    fl(w * max(0, max over the avoided vectors of rel_n(x))): a hinge — a row that does not resemble any avoided vector pays
 *             nothing; 0 when A = 0.
 *   m(x)      fl(base(x) - pen(x)): every operation rounded once, no fused multiply-add.  With A = 0, m = base bit for bit.
 * ORDER: m descending, ties -> lower global position (the library's canonical order).  A row whose score is undefined under any of
 * the compound's vectors (a zero row under the cosine) is no candidate.  The answer is the first num_results rows in that order, each
 * row at most once.
 * The walk (Fagin's threshold algorithm, the random accesses done where the rows live): the W ranked lists of the wanted vectors are
 * walked in lockstep, PCV_MAX_RESULTS entries of each a step (the last step shorter, so that no list is walked past `pool`); the
 * avoided vectors are never ranked.  After each step every row met for the first time is scored under ALL the compound's vectors — m
 * does not depend on which list brought it in — and the KEPT rows are the first min(num_results, rows met) in the order above.  With
 * T = min (ALL) or max (ANY) over the lists of the relevance of the last entry walked, the walk ends at the first step where one of
 * these holds:
 *   (a) a list delivered fewer entries than the step asked for: every selectable row has been met — exact = 1;
 *   (b) num_results rows are kept and the last of them has m > T: exact = 1.  A row met in NO list has each rel_j at most its list's
 *       last relevance, so base <= T; pen >= 0 and both roundings are monotone, so m <= T.  The test is STRICT: an unmet row with
 *       m == T may have a lower position than the kept one, and then it wins the tie;
 *   (c) `pool` entries of each list are walked: exact = 0 — the best rows met so far.  A 1 is a proof, a 0 is no disproof.
 *   want, want_offsets    [sum W][dim] f32; compound i owns vectors want_offsets[i] .. want_offsets[i + 1] ([n_compounds + 1], from 0)
 *   avoid, avoid_offsets  likewise [sum A][dim] and [n_compounds + 1]; both NULL: no avoided vectors anywhere
 *   pool              num_results .. PCV_MAX_COMPOUND_POOL: entries of each list the walk may examine
 *   out_ids           [n_compounds][num_results] the kept rows, best first, -1 behind them (may be NULL, as every output)
 *   out_combined      [n_compounds][num_results] f64: m, NaN behind
 *   out_part_scores   [n_compounds][num_results][PCV_MAX_COMPOUND_PARTS] f32: the score pcv_searcher_search reports for the row under
 *                     each wanted vector, bit for bit; NaN behind W and behind the kept rows
 *   out_penalties     [n_compounds][num_results] f64: pen, NaN behind
 *   out_counts        [n_compounds] rows kept;  out_examined  [n_compounds] entries walked per list (of the longest walk, where an
 *                     undefined score shortened another);  out_exact  [n_compounds] the certificate
 * A NULL searcher, n_compounds <= 0, num_results outside [1, PCV_MAX_RESULTS], pool outside [num_results, PCV_MAX_COMPOUND_POOL], an
 * unknown mode, a negative or non-finite avoid_weight, NULL or non-ascending offsets (offsets[0] != 0; one of avoid / avoid_offsets
 * NULL alone), W outside [1, PCV_MAX_COMPOUND_PARTS], A outside [0, PCV_MAX_COMPOUND_PARTS], a vector value that is not finite and,
 * under the cosine, a vector whose squared norm (f64, feature order) lies outside [2^-126, inf) give PCV_ERR_INVALID before any
 * device work; pending rows and a queued pass fail as in pcv_searcher_search_boosted.  The wanted vectors of a compound share the
 * passes of one group of queries: a compound with more wanted vectors than a pass takes (4 with PCV_KERNEL_WAVE) gives
 * PCV_ERR_UNSUPPORTED, naming both numbers, before any launch.  No selected rows give the blank answer with exact = 1.  Works on views.
 * Not in scope: a sharded form, device-resident output, a weighted-sum mode (that is one query vector today), a combination with the
 * group table, the value table or distinct results. */
enum { PCV_MAX_COMPOUND_PARTS = 8, PCV_MAX_COMPOUND_POOL = 4096 };
enum { PCV_COMPOUND_ALL = 0, PCV_COMPOUND_ANY = 1 };
pcv_status pcv_searcher_search_compound(pcv_searcher* s, const int64_t* source_ids, int n_sources, int num_results, int pool, int mode,
                                        float avoid_weight, const float* want, const int64_t* want_offsets, const float* avoid,
                                        const int64_t* avoid_offsets, int n_compounds, int64_t* out_ids, double* out_combined,
                                        float* out_part_scores, double* out_penalties, int32_t* out_counts, int32_t* out_examined,
                                        uint8_t* out_exact);
/* The same call with every vector built on the device from stored items, as pcv_searcher_like_queries builds them: part p of the
 * wanted side is the weighted sum of the rows that carry want_ids[want_example_offsets[p] .. want_example_offsets[p + 1]) (weights
 * NULL: all 1), compound i owns parts want_offsets[i] .. want_offsets[i + 1]; likewise the avoided side, whose four arrays may all
 * be NULL.  A view looks its examples up in its parent.  The built vectors are held to the checks above (a part none of whose
 * examples is stored is a zero vector: PCV_ERR_INVALID under the cosine).  exclude_examples != 0: rows that carry one of the compound's
 * WANTED example ids are left out of its answer, as in pcv_searcher_search_like — the walk keeps num_results plus the number of such
 * rows (the largest over the compounds), which must not exceed PCV_MAX_RESULTS (else PCV_ERR_UNSUPPORTED), and the host drops
 * them: a certified walk of the longer answer certifies the shorter one. */
pcv_status pcv_searcher_search_compound_like(pcv_searcher* s, const int64_t* source_ids, int n_sources, int num_results, int pool, int mode,
                                             float avoid_weight, const int64_t* want_ids, const float* want_weights,
                                             const int64_t* want_example_offsets, const int64_t* want_offsets, const int64_t* avoid_ids,
                                             const float* avoid_weights, const int64_t* avoid_example_offsets,
                                             const int64_t* avoid_offsets, int n_compounds, int exclude_examples, int64_t* out_ids,
                                             double* out_combined, float* out_part_scores, double* out_penalties, int32_t* out_counts,
                                             int32_t* out_examined, uint8_t* out_exact);

/* The select steps of the most recent ranked call on this handle (pcv_searcher_search_distinct, _grouped, _where, _boosted, _diverse,
 * _compound): the hipEvent time of the launches that follow the passes — events recorded right before and after each, summed — and
 * their number.  A diagnostic beside pcv_searcher_last_stats, whose total_ms times the passes themselves (tools/bench_compound.py).
 * Either output may be NULL. */
pcv_status pcv_searcher_last_select_stats(pcv_searcher* s, float* out_ms, int32_t* out_launches);

/* Duplicate pairs: the exact self-join of the corpus on the device — every pair of searchable rows that are near-duplicates of each
 * other, found once and corpus-wide (what pcv_searcher_search_distinct collapses per query, for pcv_searcher_remove_ids /
 * pcv_searcher_hide_ids to act on).
 * The rows taking part are exactly those a pcv_searcher_search with the same source filter could return: hidden rows and
 * unsearchable rows (scale 0) take no part, a view joins its own rows, source_ids == NULL means all sources, an empty list matches
 * nothing (out_count = out_total = 0).  A pair is two different rows a, b with global position a < b; it is a duplicate pair iff
 * dup(a, b) exactly as pcv_searcher_search_distinct defines it: the canonical cosine c of the two stored f32 rows — f64, products
 * exact, sums in feature order — is >= (double)threshold, for BOTH metrics.  A row without a cosine (zero or
 * non-finite norm) pairs with nothing.  Two rows carrying the same item id are a pair like any other (id_a == id_b).
 *   threshold    in (-1, 1]; at exactly 1 see pcv_searcher_search_distinct: use the f32 below 1 for "exact copies"
 *   max_pairs    1 .. PCV_MAX_DUPLICATE_PAIRS
 *   out_id_a/b   [max_pairs] the first min(total, max_pairs) pairs in the order: descending c, ties -> lower position of a, then
 *                lower position of b; out_id_a is the id of the lower-positioned row of the pair
 *   out_scores   [max_pairs] (float)c (may be NULL)
 *   out_count    pairs written
 *   out_total    the exact number of duplicate pairs (may be NULL); total > count is the "more" signal
 * A NULL searcher, NULL id outputs or out_count, max_pairs out of range or a threshold that is NaN or outside (-1, 1] give
 * PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in pcv_searcher_search.  If the join finds more than
 * PCV_MAX_DUPLICATE_PAIRS pairs (or its screen lists more than four times as many candidates) the call returns
 * PCV_ERR_UNSUPPORTED naming the count reached, before any larger list is allocated; the searcher stays usable.  A dimension whose
 * bf16 row tile does not fit the LDS of a CU gives PCV_ERR_UNSUPPORTED.  The result does not depend on which screening copies
 * exist, nor on pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity: the join reads the f32 rows (DESIGN.md §4
 * "Duplicate pairs").  Not in scope: a sharded form (the pairs across shards need the rows of both) and device-resident output. */
enum { PCV_MAX_DUPLICATE_PAIRS = 16777216 }; /* 2^24 */
pcv_status pcv_searcher_find_duplicates(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int64_t max_pairs,
                                        int64_t* out_id_a, int64_t* out_id_b, float* out_scores, int64_t* out_count,
                                        int64_t* out_total);

/* Counters of the most recent pcv_searcher_find_duplicates on this handle. */
typedef struct pcv_duplicate_stats {
    int64_t rows;        /* rows of the selected segments (those taking no part included) */
    int64_t candidates;  /* pairs the bf16 screen listed and the f64 step scored            */
    int64_t pairs;       /* duplicate pairs (the call's total)                              */
    int32_t tile_rows;   /* rows of the LDS tile the screen kernel staged                   */
    int32_t reruns;      /* screen launches repeated because the candidate list was short   */
    float prep_ms;       /* hipEvent times of the three steps (a repeated screen included)  */
    float screen_ms;
    float rescore_ms;
} pcv_duplicate_stats;
pcv_status pcv_searcher_last_duplicate_stats(pcv_searcher* s, pcv_duplicate_stats* out);

/* Item labels: the exact best of K label vectors for EVERY row — the transpose of a search (which rows are best for a few vectors).
 * A host encodes K tag or topic prompts and wants each stored item tagged with its best one and a count per tag; every Lloyd
 * iteration of k-means is the same pass.  Computed where the rows live, in one pass over the f32 rows per tile of labels.
 * The rows concerned are those of the selected segments in global position order, n of them (hidden and unsearchable rows
 * included: they keep their place); source_ids == NULL means all sources, an empty list selects nothing (n = 0); a view assigns
 * its own rows.  A row TAKES PART iff a pcv_searcher_search with the same filter could return it (searchable, not hidden,
 * scale != 0).  For such a row r, c(r, j) = the canonical score of labels[j] in the query's place and the stored f32 row — f64,
 * products exact, sums in feature order, with the searcher's metric — and label(r) is the j with the largest
 * defined c(r, j), ties to the lower j.  If no c(r, j) is defined (under cosine: a row or label of zero or non-finite norm), or the
 * row takes no part, label = -1 and the score is NaN.
 *   labels       host [K][dim] f32, 1 <= K <= PCV_MAX_LABELS, every value finite
 *   capacity     entries the per-row outputs have room for; the call fails with PCV_ERR_INVALID if capacity < n (out_n is set)
 *   out_label    [capacity] int32
 *   out_score    [capacity] what pcv_searcher_search reports for that (label vector, row) pair, bit for bit: cosine (float)c, dot
 *                the f32 distance (may be NULL)
 *   out_ids      [capacity] the item id of every position (may be NULL)
 *   out_counts   [K] rows per label (may be NULL)
 *   out_n        n.  With out_label == NULL and capacity == 0 the call only reports n (the style of pcv_searcher_hidden_ids) and does no
 *                device work
 * A NULL searcher, labels or out_n, K out of range, a NaN or Inf in a label, or out_label == NULL with capacity != 0 give
 * PCV_ERR_INVALID before any device work; a searcher with pending rows fails as in pcv_searcher_search.  A dimension whose bf16
 * label tile does not fit the LDS of a CU gives PCV_ERR_UNSUPPORTED, and so does a call whose bf16 screen lists more than 2^28
 * (row, label) candidates (thousands of near-identical labels over millions of rows).  The result does not depend on which screening
 * copies exist, nor on pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity: the pass reads the f32 rows and touches no
 * pass state (DESIGN.md §4 "Item labels").  Everything the call allocates on the device is given back when it returns.
 * The top-m labels per row are pcv_searcher_assign_top's.  Not in scope: a sharded form, device-resident output. */
enum { PCV_MAX_LABELS = 4096 };
pcv_status pcv_searcher_assign(pcv_searcher* s, const float* labels, int n_labels, const int64_t* source_ids, int n_sources, int64_t capacity,
                               int32_t* out_label, float* out_score, int64_t* out_ids, int64_t* out_counts, int64_t* out_n);

/* Top-m labels: the exact m best of K label vectors for every row, with an optional score bound — multi-label tagging ("every topic
 * prompt that scores at least 0.3, at most five"), soft assignment after pcv_searcher_kmeans, the runner-up label and its gap (the
 * ambiguous items, the centroid silhouette of a clustering: INTEGRATION.md).  Rows, their order, participation and c(r, j) are those of
 * pcv_searcher_assign.  The labels of row r are the j with c(r, j) defined and c(r, j) >= (double)min_score, ordered by (c descending,
 * j ascending); the first m of them are kept.  min_score = -INFINITY: no bound; under dot the bound is on the raw canonical dot, not
 * on the reported distance.
 *   m               1 .. PCV_MAX_TOP_LABELS (m > K is allowed: the slots behind K stay unused)
 *   out_labels      [capacity][m] int32, best first, unused slots -1
 *   out_scores      [capacity][m] what pcv_searcher_search reports for that pair, bit for bit; unused slots NaN (may be NULL)
 *   out_ids         [capacity] the item id of every position (may be NULL)
 *   out_counts      [capacity] int32 labels listed for the row (0 for a row that takes no part)
 *   out_label_rows  [K] rows that list label j in any slot (may be NULL)
 *   out_n           n; with out_labels == NULL and capacity == 0 the call only reports n and does no device work
 * With m = 1 and no bound, labels, scores and ids are pcv_searcher_assign's bit for bit and out_label_rows its out_counts.  Errors as
 * pcv_searcher_assign, plus m out of range, a NaN min_score and a NULL out_counts (PCV_ERR_INVALID, before any device work).  The
 * result does not depend on screening copies, pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity; a view assigns its own
 * rows; everything the call allocates on the device is given back when it returns (DESIGN.md §4 "Top-m labels": two passes over the
 * f32 rows per label tile).  Not in scope: a sharded form, device-resident output. */
enum { PCV_MAX_TOP_LABELS = 8 };
pcv_status pcv_searcher_assign_top(pcv_searcher* s, const float* labels, int n_labels, int m, float min_score, const int64_t* source_ids,
                                   int n_sources, int64_t capacity, int32_t* out_labels, float* out_scores, int64_t* out_ids,
                                   int32_t* out_counts, int64_t* out_label_rows, int64_t* out_n);

/* Counters of the most recent pcv_searcher_assign_top on this handle. */
typedef struct pcv_assign_top_stats {
    int64_t rows;         /* rows of the selected segments (those taking no part included)       */
    int64_t candidates;   /* (row, label) pairs the list pass listed and the f64 step scored      */
    int64_t listed;       /* the sum of out_counts                                                */
    int32_t m;
    int32_t label_tiles;  /* label tiles: two passes over the f32 rows each                       */
    int32_t tile_labels;  /* labels of one LDS tile (128, 64 or 32)                               */
    int32_t reruns;       /* list passes repeated because the candidate list was short            */
    float prep_ms;        /* hipEvent times of the steps (a repeated list pass included)          */
    float bound_ms;       /* the bound passes and the merges of their column maxima               */
    float screen_ms;      /* the list passes                                                      */
    float rescore_ms;
    float select_ms;
} pcv_assign_top_stats;
pcv_status pcv_searcher_last_assign_top_stats(pcv_searcher* s, pcv_assign_top_stats* out);

/* The integer sums of the unit rows of every label, reproducible bit for bit.  labels[n] names a label in [0, K) for every position of
 * the selected rows (as pcv_searcher_assign orders them; a negative value: none).  With rinv_r = (float)(1 / sqrt(|x_r|^2)) from the
 * canonical f64 |x_r|^2 and t(r, d) = rint((double)x[r][d] * (double)rinv_r * 2^32) as int64 — the product of two f32 is exact in
 * f64, so one rounding, half to even —
 *   out_sums[j][d] = sum of t(r, d) over the rows with labels[r] == j that have a cosine (squared norm in [2^-126, inf))
 *   out_counts[j]  = how many rows that were (may be NULL)
 * Integer addition is associative: whatever order the device adds in, the bits are the same, and three lines of numpy reproduce
 * them.  |t| <= 2^32 (1 + 2^-23), so a label with more than 2^30 members is refused (PCV_ERR_UNSUPPORTED).  A row that takes
 * no part in pcv_searcher_assign (hidden, or unsearchable: scale 0) adds nothing and is not counted, whatever label it is given, like
 * a row without a cosine.  Any dimension is accepted (the sums need no label tile).  n must be the n of pcv_searcher_assign for
 * the same filter, K in [1, PCV_MAX_LABELS], no label >= K (PCV_ERR_INVALID).  centroid[j][d] = (float)((double)out_sums[j][d] * 2^-32)
 * is the mean direction up to length, which a cosine ignores. */
pcv_status pcv_searcher_label_sums(pcv_searcher* s, const int64_t* source_ids, int n_sources, const int32_t* labels, int64_t n, int n_labels,
                                   int64_t* out_sums, int64_t* out_counts);

/* Spherical k-means (Lloyd) on the device, reproducible bit for bit.  It clusters by the canonical cosine for BOTH searcher metrics,
 * as pcv_searcher_find_duplicates does.  Starting from centroids = init[K][dim]:
 *   assignment i labels every row with the current centroids exactly as pcv_searcher_assign does under cosine; moved[i] is the
 *   number of rows whose label differs from the assignment before (before the first: every row has label -1);
 *   if moved[i] == 0, or max_iters updates have been made, the call ends; otherwise update: centroid[j] becomes
 *   (float)((double)S[j][d] * 2^-32) with S the sums of pcv_searcher_label_sums for these labels — not normalised; a label without a
 *   member keeps its vector — and the next assignment follows.
 *   out_centroids [K][dim] the centroids the LAST assignment used
 *   out_label, out_score, out_ids, out_counts, capacity, out_n   of the last assignment, as in pcv_searcher_assign (out_label may be
 *                 NULL here only together with capacity == 0, which reports n alone)
 *   out_iters     updates made (may be NULL);   out_moved  [max_iters + 1], entries 0 .. *out_iters filled (may be NULL)
 * max_iters = 0 is pcv_searcher_assign with the cosine metric.  The labels stay on the device between the steps; per update only the
 * K x dim sums come to the host, where the centroids are formed.  Errors as pcv_searcher_assign, plus max_iters < 0 and a NULL init
 * or out_centroids (PCV_ERR_INVALID) and a label with more than 2^30 members (PCV_ERR_UNSUPPORTED).  init comes from the caller, or from
 * pcv_searcher_seeds (k-means++) through pcv_searcher_like_queries.  Not in scope: a sharded form, device-resident output. */
pcv_status pcv_searcher_kmeans(pcv_searcher* s, const float* init, int n_labels, int max_iters, const int64_t* source_ids, int n_sources,
                               int64_t capacity, float* out_centroids, int32_t* out_label, float* out_score, int64_t* out_ids,
                               int64_t* out_counts, int32_t* out_iters, int64_t* out_moved, int64_t* out_n);

/* Counters of the most recent pcv_searcher_assign or pcv_searcher_kmeans on this handle (k-means: times summed over its
 * assignments, the other counters those of the last one). */
typedef struct pcv_assign_stats {
    int64_t rows;         /* rows of the selected segments (those taking no part included)       */
    int64_t candidates;   /* (row, label) pairs the bf16 screen listed                            */
    int32_t label_tiles;  /* label tiles = passes over the f32 rows                               */
    int32_t tile_labels;  /* labels of one LDS tile (128, 64 or 32)                               */
    int32_t reruns;       /* screens repeated because the candidate list was short                */
    float prep_ms;        /* hipEvent times of the three steps (a repeated screen included)       */
    float screen_ms;
    float rescore_ms;
} pcv_assign_stats;
pcv_status pcv_searcher_last_assign_stats(pcv_searcher* s, pcv_assign_stats* out);

/* Item neighbours: the k-nearest-neighbour table of the corpus — for EVERY stored item its exact k best other items, computed where
 * the rows live (a "related items" panel without a search at view time, the distance to the k-th neighbour as an outlier score,
 * label propagation, density and graph clustering, a 2-D map of a library).
 * The rows concerned are those of the selected segments in global position order, n of them, as in pcv_searcher_assign (hidden and
 * unsearchable rows included: they keep their place); source_ids == NULL means all sources, an empty list selects nothing (n = 0); a
 * view lists its own rows.  A row TAKES PART under exactly the rules of pcv_searcher_find_duplicates: a pcv_searcher_search with the
 * same filter could return it (scale != 0, not hidden) and it has a cosine (canonical |x|^2 in [2^-126, inf)).  For a participating
 * row r and every other participating row p (another position; the same item id is a neighbour like any other),
 * c(r, p) = the canonical cosine of the two stored f32 rows — f64, products exact, sums in feature order — for BOTH
 * metrics.  The neighbours of r are the k partners with the largest c, ties to the lower global position, ordered by (c descending,
 * position ascending).
 *   k                 1 .. PCV_MAX_NEIGHBORS
 *   capacity          rows the outputs have room for; capacity < n gives PCV_ERR_INVALID (out_rows is set)
 *   out_ids           [capacity] the item id of every position
 *   out_neighbor_ids  [capacity][k] the neighbours' item ids, best first; unused slots -1
 *   out_scores        [capacity][k] (float)c; unused slots NaN
 *   out_counts        [capacity] int32: min(k, participating rows - 1); 0 for a row that takes no part (it is nobody's neighbour)
 *   out_rows          n.  With all four arrays NULL and capacity == 0 the call only reports n and does no device work
 * A NULL out_rows or searcher, k out of range, a negative capacity or a NULL array with capacity != 0 give PCV_ERR_INVALID before the
 * handle is looked at; a searcher with pending rows fails as in pcv_searcher_search.  A dimension whose bf16 row tile does not fit the
 * LDS of a CU (above 2496) gives PCV_ERR_UNSUPPORTED, and so does a call whose screen lists more than 2^30 (row, partner) candidates
 * (more than a thousand near-identical rows per row across a million), before the larger list is allocated.  The result does not
 * depend on which screening copies exist, nor on pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity: the call reads the
 * f32 rows and touches no pass state (DESIGN.md §4 "Item neighbours").  Everything it allocates on the device is given back when it
 * returns.  Not in scope: a sharded searcher (pcv_searcher_set_shard_offset != 0 or a pcv_comm: a row's neighbours lie in every
 * shard) — PCV_ERR_INVALID — and device-resident output. */
enum { PCV_MAX_NEIGHBORS = 64 };
pcv_status pcv_searcher_neighbors(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, int64_t capacity, int64_t* out_ids,
                                  int64_t* out_neighbor_ids, float* out_scores, int32_t* out_counts, int64_t* out_rows);

/* Counters of the most recent pcv_searcher_neighbors on this handle. */
typedef struct pcv_neighbor_stats {
    int64_t rows;           /* rows of the selected segments (those taking no part included)                  */
    int64_t candidates;     /* directed (row, partner) pairs the bf16 list pass left and the f64 step scored  */
    int64_t listed;         /* neighbours written (the sum of out_counts)                                     */
    int32_t k;
    int32_t tile_rows;      /* rows of the LDS tile the screen kernel staged                                  */
    int32_t sample_stride;  /* the bound pass streamed every sample_stride-th block of partners               */
    int32_t spans;          /* disjoint partner sets whose maxima bound a row's k-th best score               */
    int32_t reruns;         /* list passes repeated because the candidate list was short                      */
    float prep_ms;          /* hipEvent times of the steps (a repeated list pass included in screen_ms)       */
    float bound_ms;
    float screen_ms;
    float rescore_ms;
    float select_ms;
} pcv_neighbor_stats;
pcv_status pcv_searcher_last_neighbor_stats(pcv_searcher* s, pcv_neighbor_stats* out);

/* Item matches: the join of two sets of stored items — for EVERY item of the sources A (`from`) its exact k best items of the
 * sources B (`to`), computed where the rows live (which newly imported items already exist elsewhere, with a score bound; the pages of
 * one source related to those of another; nearest-neighbour tagging from a tagged source).  The work is |A| x |B|: pcv_searcher_neighbors
 * over the union would also pay for A x A and B x B, and an item's own set would fill its k slots.
 * The rows concerned are those of the segments selected by from_source_ids in global position order, n of them, as in
 * pcv_searcher_neighbors (hidden and unsearchable rows included: they keep their place); from_source_ids == NULL means all sources,
 * an empty list selects nothing (n = 0); a view matches among its own rows.  The PARTNERS are the participating rows of the segments
 * selected by to_source_ids, with the same NULL and empty-list rules.  The two selections may overlap, fully or partly, and lie in any
 * position order.  A row TAKES PART under exactly the rules of pcv_searcher_neighbors: a pcv_searcher_search with the same filter could
 * return it (scale != 0, not hidden) and it has a cosine (canonical |x|^2 in [2^-126, inf)).  A row is never its own partner (the same
 * position); another row carrying the same item id is a partner like any other.  For a participating row r of A and a partner p,
 * c(r, p) = the canonical cosine of the two stored f32 rows — f64, products exact, sums in feature order — for BOTH
 * metrics.  The matches of r are, among the partners with c >= (double)min_score, the k with the largest c, ties to the lower global
 * position, ordered by (c descending, position ascending).  Fewer than k such partners is a result, not an error: the count says so.
 *   k               1 .. PCV_MAX_NEIGHBORS
 *   min_score       in [-1, 1].  Exactly -1.0f means no bound: the comparison is skipped, and a c that rounds below -1 is still listed
 *   capacity        rows the outputs have room for; capacity < n gives PCV_ERR_INVALID (out_rows is set)
 *   out_ids         [capacity] the item id of every position
 *   out_match_ids   [capacity][k] the matches' item ids, best first; unused slots -1
 *   out_scores      [capacity][k] (float)c; unused slots NaN
 *   out_counts      [capacity] int32: matches written; 0 for a row that takes no part
 *   out_rows        n.  With all four arrays NULL and capacity == 0 the call only reports n and does no device work
 * A NULL out_rows or searcher, k out of range, a min_score that is NaN or outside [-1, 1], a negative capacity or a NULL array with
 * capacity != 0 give PCV_ERR_INVALID before the handle is looked at; a searcher with pending rows and a sharded searcher fail as in
 * pcv_searcher_neighbors.  A dimension whose bf16 row tile does not fit the LDS of a CU (above 2496) gives PCV_ERR_UNSUPPORTED, and
 * so does a call whose screen lists more than 2^30 (row, partner) candidates, before the larger list is allocated.  The result does
 * not depend on which screening copies exist, nor on pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity: the call reads
 * the f32 rows and touches no pass state (DESIGN.md §4 "Item matches").  Everything it allocates on the device is given back when it
 * returns.  pcv_searcher_match(X, X, k, -1) returns bit for bit what pcv_searcher_neighbors(X, k) returns: the two calls run the same
 * steps.  Not in scope: a second searcher handle as B, a sharded searcher and device-resident output. */
pcv_status pcv_searcher_match(pcv_searcher* s, const int64_t* from_source_ids, int n_from, const int64_t* to_source_ids, int n_to, int k,
                              float min_score, int64_t capacity, int64_t* out_ids, int64_t* out_match_ids, float* out_scores,
                              int32_t* out_counts, int64_t* out_rows);

/* Counters of the most recent pcv_searcher_match on this handle. */
typedef struct pcv_match_stats {
    int64_t rows;            /* n: rows of the segments of `from` (those taking no part included)               */
    int64_t partner_rows;    /* rows of the segments of `to` (likewise)                                         */
    int32_t owner_blocks;    /* 32-row blocks the screen cut its tiles from: the segments of `from`             */
    int32_t partner_blocks;  /* 32-row blocks every tile was streamed against: the segments of `to`             */
    int64_t candidates;      /* directed (row, partner) pairs the bf16 list pass left and the f64 step scored   */
    int64_t listed;          /* matches written (the sum of out_counts)                                         */
    int32_t k;
    int32_t tile_rows;       /* rows of the LDS tile the screen kernel staged                                   */
    int32_t sample_stride;   /* the bound pass streamed every sample_stride-th partner block                    */
    int32_t spans;           /* disjoint partner sets whose maxima bound a row's k-th best score                */
    int32_t reruns;          /* list passes repeated because the candidate list was short                       */
    float prep_ms;           /* hipEvent times of the steps (a repeated list pass included in screen_ms)        */
    float bound_ms;
    float screen_ms;
    float rescore_ms;
    float select_ms;
} pcv_match_stats;
pcv_status pcv_searcher_last_match_stats(pcv_searcher* s, pcv_match_stats* out);

/* Group-aware pairs: pcv_searcher_neighbors, pcv_searcher_match and pcv_searcher_find_duplicates over a corpus of chunks, where the
 * group table (pcv_searcher_set_groups) says which rows are one document — "the k nearest rows of OTHER documents", "the k nearest
 * other documents", "duplicates across documents".  The plain calls ignore the table and stay as they are.
 * The existing rules of each call hold unchanged: which rows take part, the canonical f64 cosine, the order (c descending, position
 * ascending), every argument rule, refusal and limit.
 *   The GROUP of a row is the value its item id has in the table at call time (a view reads its parent's).  An id without an entry, or
 *   with PCV_NO_GROUP, makes the ROW a singleton, exactly as in pcv_searcher_search_grouped.  Two different rows are SIBLINGS iff both
 *   have a group >= 0 and the keys are equal: two ungrouped rows that share an id are not siblings, two rows that share an id with a
 *   group are.
 *   PCV_GROUPS_SKIP_OWN       a sibling of the owner is not a partner of it; the result is otherwise that of the plain call over the
 *                             remaining partners.
 *   PCV_GROUPS_ONE_PER_GROUP  the owner's partners are walked in order (after SKIP_OWN if set, after min_score for match); a partner is
 *                             KEPT iff no kept partner is its sibling, and the walk ends after the k-th kept partner.  A kept partner
 *                             is the best member of its group for this owner, the k kept are the k best groups by best member.
 *                             Singletons never collapse.
 *   flags == 0                the plain call, bit for bit (the partners' groups are still reported).
 * out_neighbor_groups / out_match_groups: [capacity][k] the group key of every reported partner, PCV_NO_GROUP for a singleton and in
 * unused slots; may be NULL.  Flags outside 0..3 give PCV_ERR_INVALID before the handle is looked at.  An empty or absent table is
 * legal: every row is a singleton and the result is the plain call's.  The grouped calls fill pcv_searcher_last_neighbor_stats /
 * _last_match_stats / _last_duplicate_stats as the plain ones do, and pcv_searcher_last_pair_group_stats beside them.
 * pcv_searcher_find_duplicates_grouped always skips sibling pairs and takes no flags: out_total counts the pairs of non-siblings only,
 * out_skipped (may be NULL) the sibling pairs with c >= threshold, which the plain call would report: out_total + out_skipped is the
 * plain call's total.
 * Exact (DESIGN.md §4 "Group-aware pairs"): the siblings are left out of the bound the screen's thresholds come from, and under
 * ONE_PER_GROUP that bound counts distinct groups; every exact decision compares the 64-bit keys.  Cost beside the plain call: 12
 * bytes per row for the rows' groups, 8 instead of 4 bytes per (row, span) of the bound pass, 8 bytes more per candidate.
 * Not in scope: density clusters, the linkage tree and the reach tree, pcv_searcher_search_like, a sharded form, device-resident
 * output. */
enum { PCV_GROUPS_SKIP_OWN = 1, PCV_GROUPS_ONE_PER_GROUP = 2 };
pcv_status pcv_searcher_neighbors_grouped(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, uint32_t flags, int64_t capacity,
                                          int64_t* out_ids, int64_t* out_neighbor_ids, float* out_scores, int64_t* out_neighbor_groups,
                                          int32_t* out_counts, int64_t* out_rows);
pcv_status pcv_searcher_match_grouped(pcv_searcher* s, const int64_t* from_source_ids, int n_from, const int64_t* to_source_ids, int n_to, int k,
                                      float min_score, uint32_t flags, int64_t capacity, int64_t* out_ids, int64_t* out_match_ids,
                                      float* out_scores, int64_t* out_match_groups, int32_t* out_counts, int64_t* out_rows);
pcv_status pcv_searcher_find_duplicates_grouped(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int64_t max_pairs,
                                                int64_t* out_id_a, int64_t* out_id_b, float* out_scores, int64_t* out_count,
                                                int64_t* out_total, int64_t* out_skipped);

/* Counters of the most recent grouped pair call on this handle (neighbors_grouped, match_grouped or find_duplicates_grouped). */
typedef struct pcv_pair_group_stats {
    int64_t grouped_rows;        /* launch rows that take part and have a group >= 0                                            */
    int64_t sibling_candidates;  /* listed candidates the f64 step dropped as siblings (find_duplicates_grouped: out_skipped)   */
    int64_t collapsed;           /* entries the select step passed over as members of a kept group (ONE_PER_GROUP)              */
    uint32_t flags;              /* the call's flags (find_duplicates_grouped: PCV_GROUPS_SKIP_OWN)                             */
    int32_t bound_tile_rows;     /* rows of the LDS tile of the bound pass: 64 at most in its grouped form (flags != 0)         */
    float groups_ms;             /* hipEvent time of the step that gathers the rows' groups from the table                      */
} pcv_pair_group_stats;
pcv_status pcv_searcher_last_pair_group_stats(pcv_searcher* s, pcv_pair_group_stats* out);

/* Density clusters: DBSCAN under the cosine over the stored items, exact, computed where the rows live — which topics a library
 * holds, how many, and which items belong to none, without the caller choosing a number of groups; degree(r) is a density and
 * outlier score of its own.
 * The rows concerned are those of the selected segments in global position order, n of them, exactly as in
 * pcv_searcher_find_duplicates and pcv_searcher_neighbors (hidden and unsearchable rows included: they keep their place);
 * source_ids == NULL means all sources, an empty list selects nothing (n = 0); a view clusters its own rows.  A row TAKES PART iff a
 * pcv_searcher_search with the same filter could return it (scale != 0, not hidden) and it has a cosine (canonical |x|^2 in
 * [2^-126, inf)).  For two different participating positions a, b: near(a, b) <=> c(a, b) >= (double)threshold, c the canonical
 * cosine of the two stored f32 rows — f64, products exact, sums in feature order — for BOTH metrics.
 *   degree(r)   the number of other participating rows p with near(r, p)
 *   core        r is a core row iff degree(r) + 1 >= min_items (min_items counts the item itself: DBSCAN's min_samples)
 *   clusters    the connected components of the graph on the core rows with the edges near; numbered 0, 1, ... in ascending order
 *               of the lowest global position among their core rows
 *   border      a participating row that is not core and has a core row near it; it takes the label of the core row near it with
 *               the LOWEST GLOBAL POSITION (no score enters this rule)
 *   noise       every other participating row
 *   threshold   in (-1, 1]
 *   min_items   >= 1
 *   capacity    rows the outputs have room for; capacity < n gives PCV_ERR_INVALID (out_rows is set)
 *   out_ids     [capacity] the item id of every position; may be NULL
 *   out_label   [capacity] the cluster, or -1 for noise and for rows that take no part
 *   out_kind    [capacity] PCV_DENSITY_CORE, _BORDER, _NOISE, or _NONE (the row takes no part)
 *   out_degree  [capacity] degree; 0 for _NONE rows; may be NULL
 *   out_rows    n.  With every array NULL and capacity == 0 the call only reports n and does no device work (out_clusters may be
 *               NULL then, and is not written)
 *   out_clusters the number of clusters
 * A NULL searcher or out_rows, a NaN or out-of-range threshold, min_items < 1, a negative capacity, a NULL out_label, out_kind or
 * out_clusters with the other arrays given or capacity != 0, capacity < n, and a sharded searcher (pcv_searcher_set_shard_offset
 * != 0 or a pcv_comm: a cluster lies in every shard) give PCV_ERR_INVALID before any device work; a searcher with pending rows fails
 * as in pcv_searcher_search.  PCV_ERR_UNSUPPORTED, with the searcher still usable: a dimension whose bf16 row tile does not fit the
 * LDS of a CU (above 2496); more than 2^30 rows; more than 2^28 pairs that the bf16 screen cannot decide (pairs within its certified
 * margin of the threshold, and every pair with a row whose length is outside [2^-20, 2^20]) — the message names the count, and the
 * error comes before the larger list is allocated.  Pairs the screen decides are counted and linked inside its kernel and never
 * listed, so the number of near pairs is not limited.  The result does not depend on which screening copies exist, nor on
 * pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity: the call reads the f32 rows and touches no pass state (DESIGN.md §4
 * "Density clusters").  Everything it allocates on the device is given back when it returns.  Not in scope: a sharded form and
 * device-resident output. */
enum { PCV_DENSITY_NONE = -1, PCV_DENSITY_NOISE = 0, PCV_DENSITY_BORDER = 1, PCV_DENSITY_CORE = 2 };
pcv_status pcv_searcher_density_clusters(pcv_searcher* s, const int64_t* source_ids, int n_sources, float threshold, int min_items,
                                         int64_t capacity, int64_t* out_ids, int32_t* out_label, int8_t* out_kind, int32_t* out_degree,
                                         int64_t* out_rows, int32_t* out_clusters);

/* Counters of the most recent pcv_searcher_density_clusters on this handle (all zero after a call that only reported n). */
typedef struct pcv_density_stats {
    int64_t rows;           /* rows of the selected segments (those taking no part included)                   */
    int64_t participating;  /* rows that take part                                                             */
    int64_t sure_pairs;     /* near pairs the bf16 screen decided alone (never listed, never rescored)         */
    int64_t candidates;     /* band pairs the screen listed for the f64 step                                   */
    int64_t confirmed;      /* band pairs with c >= threshold                                                  */
    int64_t core;
    int64_t border;
    int64_t noise;
    int32_t clusters;
    int32_t tile_rows;      /* rows of the LDS tile the screen kernel staged                                   */
    int32_t reruns;         /* degree passes repeated because the band list was short                          */
    float prep_ms;          /* hipEvent times of the steps (a repeated degree pass included in degree_ms)      */
    float degree_ms;
    float rescore_ms;
    float link_ms;
    float label_ms;
} pcv_density_stats;
pcv_status pcv_searcher_last_density_stats(pcv_searcher* s, pcv_density_stats* out);

/* Linkage tree: the exact single-linkage hierarchy of the stored items, computed where the rows live — the clusters of the corpus at
 * EVERY threshold at once.  It is the maximum-cosine spanning tree of the participating rows: cutting it at t gives exactly the
 * connected components of the graph c >= t (pcv_searcher_density_clusters with min_items = 1), dropping its K - 1 weakest edges gives
 * K clusters, and its edge list, best first, is the merge order of a dendrogram.
 * The rows concerned are those of the selected segments in global position order, n of them, exactly as in
 * pcv_searcher_density_clusters (hidden and unsearchable rows included: they keep their place); source_ids == NULL means all sources,
 * an empty list selects nothing (n = 0); a view uses its own rows.  A row TAKES PART iff a pcv_searcher_search with the same filter
 * could return it (scale != 0, not hidden) and it has a cosine (canonical |x|^2 in [2^-126, inf)); P is the number of such rows.
 *   weight      of the edge {a, b}, output positions a < b: c(a, b), the canonical cosine of the two stored f32 rows — f64, products
 *               exact, sums in feature order — for BOTH metrics.  Every participating pair has a finite c: the graph
 *               is complete
 *   edge order  strict and total: e is BETTER than e' iff its c is larger; on equal c the lower position a wins, then the lower b
 *   the tree    the unique spanning tree Kruskal builds when it takes the edges from best to worst: P - 1 edges (0 if P <= 1),
 *               returned from best to worst — the single-linkage merge order
 *   capacity    rows the outputs have room for; capacity < n gives PCV_ERR_INVALID (out_rows is set)
 *   out_ids     [capacity] the item id of every position; may be NULL
 *   out_part    [capacity] 1 iff the row takes part; may be NULL
 *   out_pos_a, out_pos_b  [capacity] the edges' output positions, pos_a < pos_b
 *   out_id_a, out_id_b    [capacity] their item ids; may be NULL (both or neither)
 *   out_c       [capacity] the canonical cosine, f64: a cut must compare what pcv_searcher_density_clusters compares with
 *               (double)threshold, and (float)c can land on the other side of it
 *   out_rows    n.  With every array NULL and capacity == 0 the call only reports n and does no device work (out_edges may be NULL
 *               then, and is not written)
 *   out_edges   the number of edges
 * A NULL searcher or out_rows, a negative capacity, a NULL out_pos_a, out_pos_b, out_c or out_edges with another array given or
 * capacity != 0, one of out_id_a / out_id_b without the other, capacity < n, and a sharded searcher (pcv_searcher_set_shard_offset
 * != 0 or a pcv_comm: the tree spans every shard) give PCV_ERR_INVALID before any device work; a searcher with pending rows fails as
 * in pcv_searcher_search.  PCV_ERR_UNSUPPORTED, with the searcher still usable: a dimension whose bf16 row tile does not fit the LDS
 * of a CU (above 2496); more than 2^30 rows; more than 2^28 candidate pairs in one round (the message names the count, and the error
 * comes before the larger list is allocated).  The result does not depend on which screening copies exist, nor on
 * pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity: the call reads the f32 rows and touches no pass state (DESIGN.md §4
 * "Linkage tree").  Everything it allocates on the device is given back when it returns.  Not in scope: a sharded form and
 * device-resident output. */
pcv_status pcv_searcher_linkage_tree(pcv_searcher* s, const int64_t* source_ids, int n_sources, int64_t capacity, int64_t* out_ids,
                                     int8_t* out_part, int64_t* out_pos_a, int64_t* out_pos_b, int64_t* out_id_a, int64_t* out_id_b,
                                     double* out_c, int64_t* out_rows, int64_t* out_edges);

/* Counters of the most recent pcv_searcher_linkage_tree on this handle (all zero after a call that only reported n). */
typedef struct pcv_linkage_stats {
    int64_t rows;           /* rows of the selected segments (those taking no part included)                   */
    int64_t participating;  /* rows that take part                                                             */
    int64_t edges;          /* edges of the tree: participating - 1, or 0                                      */
    int64_t candidates;     /* directed (row, partner) pairs rescored in f64, all rounds summed                */
    int32_t rounds;         /* Boruvka rounds: at most ceil(log2 participating)                                */
    int32_t tile_rows;      /* rows of the LDS tile the screen kernel staged                                   */
    int32_t reruns;         /* list passes repeated because the candidate list was short                       */
    float prep_ms;          /* hipEvent times of the steps, each summed over the rounds (a repeated list pass  */
    float bound_ms;         /* included in list_ms, a repeated bound pass and the wait for its count in        */
    float list_ms;          /* bound_ms)                                                                       */
    float rescore_ms;
    float merge_ms;
} pcv_linkage_stats;
pcv_status pcv_searcher_last_linkage_stats(pcv_searcher* s, pcv_linkage_stats* out);

/* Cuts a linkage tree (host only: no context, no GPU).  The edges are those pcv_searcher_linkage_tree returned, in its order: the
 * function checks 0 <= pos_a < pos_b < n_rows and that c is non-increasing (no NaN), PCV_ERR_INVALID otherwise.  Edge i is KEPT iff
 * c[i] >= threshold and i < n_edges - (min_clusters - 1): threshold = -inf with min_clusters = K gives K clusters (fewer edges than
 * K - 1: none is kept), min_clusters = 1 with threshold = t the cut at t.  The components of the kept edges are numbered 0, 1, ... in
 * ascending order of their lowest position; a participating row with no kept edge is a cluster of its own.
 *   part         [n_rows] as out_part; part[r] == 0 gives label -1.  NULL: every row takes part
 *   threshold    not NaN
 *   min_clusters >= 1
 *   out_label    [n_rows]
 *   out_clusters the number of clusters; may be NULL
 * An edge with an end that takes no part is PCV_ERR_INVALID. */
pcv_status pcv_linkage_cut(const int64_t* pos_a, const int64_t* pos_b, const double* c, int64_t n_edges, const int8_t* part, int64_t n_rows,
                           double threshold, int64_t min_clusters, int32_t* out_label, int32_t* out_clusters);

/* Reach tree: the spanning tree HDBSCAN starts from — the linkage tree under the MUTUAL-REACHABILITY weight, which a single stray
 * row cannot chain through — computed where the rows live.  Rows, participation (P participating rows), c(a, b), source selection,
 * views, the n-only form and the argument errors are exactly those of pcv_searcher_linkage_tree.
 *   min_items   1 .. PCV_MAX_NEIGHBORS + 1; it counts the item itself, as in pcv_searcher_density_clusters.  A value out of range
 *               gives PCV_ERR_INVALID before the handle is looked at
 *   core(r)     the j-th largest c(r, p) over the OTHER participating rows p, j = min(min_items - 1, P - 1): the f64 value, not its
 *               float rounding; j = 0 gives +inf
 *   weight      of the edge {a, b}, output positions a < b: w = min(core(a), core(b), c(a, b))
 *   edge order  strict and total: e is BETTER than e' iff its w is larger; on equal w the lower position a wins, then the lower b.
 *               c is not a key.  Ties are the normal case: every row's j nearest partners tie at its core score
 *   the tree    the unique spanning tree Kruskal builds when it takes the edges from best to worst: P - 1 edges (0 if P <= 1),
 *               returned from best to worst.  With min_items == 1 it is pcv_searcher_linkage_tree's output bit for bit (w == c)
 *   out_core    [capacity] core(r) of every position, NaN for a row that takes no part; may be NULL
 *   out_w       [capacity] the weight of every edge, f64
 *   out_c       [capacity] its canonical cosine, f64; may be NULL
 *   the others  as in pcv_searcher_linkage_tree (out_w in the place of its out_c among the arrays that must be given)
 * Cutting the tree at t (pcv_linkage_cut on out_w) and keeping the rows with core >= t gives the core rows of
 * pcv_searcher_density_clusters(t, min_items), cluster for cluster; pcv_linkage_select picks clusters without a threshold.
 * PCV_ERR_UNSUPPORTED, with the searcher still usable: a dimension above 2496; more than 2^30 rows; more than 2^30 candidate pairs
 * in the core step or 2^28 in one round (the message names the count, and the error comes before the larger list is allocated).
 * The result does not depend on which screening copies exist, nor on pcv_searcher_set_kernel, _set_tuning or
 * _set_candidate_capacity; nothing the call allocates on the device survives it and no pass state is touched (DESIGN.md §4 "Reach
 * tree"). */
pcv_status pcv_searcher_reach_tree(pcv_searcher* s, const int64_t* source_ids, int n_sources, int min_items, int64_t capacity,
                                   int64_t* out_ids, int8_t* out_part, double* out_core, int64_t* out_pos_a, int64_t* out_pos_b,
                                   int64_t* out_id_a, int64_t* out_id_b, double* out_w, double* out_c, int64_t* out_rows,
                                   int64_t* out_edges);

/* Counters of the most recent pcv_searcher_reach_tree on this handle (all zero after a call that only reported n). */
typedef struct pcv_reach_stats {
    int64_t rows;             /* rows of the selected segments (those taking no part included)                 */
    int64_t participating;    /* rows that take part                                                           */
    int64_t edges;            /* edges of the tree: participating - 1, or 0                                    */
    int64_t core_candidates;  /* directed (row, partner) pairs the core step rescored in f64                   */
    int64_t candidates;       /* directed (row, partner) pairs the rounds rescored in f64, all rounds summed   */
    int32_t rounds;           /* Boruvka rounds: at most ceil(log2 participating)                              */
    int32_t tile_rows;        /* rows of the LDS tile the screen kernels staged                                */
    int32_t reruns;           /* list passes repeated because the candidate list was short (core step included) */
    int32_t min_items;
    float core_ms;            /* the core step: the neighbours' bound, list and rescore, and the k-th best     */
    float prep_ms;            /* hipEvent times of the steps, each summed over the rounds, as in               */
    float bound_ms;           /* pcv_linkage_stats                                                             */
    float list_ms;
    float rescore_ms;
    float merge_ms;
} pcv_reach_stats;
pcv_status pcv_searcher_last_reach_stats(pcv_searcher* s, pcv_reach_stats* out);

/* Picks clusters from a reach tree without a threshold (host only: no context, no GPU): HDBSCAN's condensed tree and excess-of-mass
 * selection, with the cosine itself as the density level.  The edges are those of pcv_searcher_reach_tree in its order with w (or of
 * pcv_searcher_linkage_tree with its c).  The call checks the positions and the order as pcv_linkage_cut does, that the edges span
 * the participating rows (n_edges == P - 1, no cycle) and min_cluster_size >= 2: PCV_ERR_INVALID otherwise.
 *   dendrogram  edge i joins the two components Kruskal had before it; the last edge is the root
 *   condensing  from the root down, M = min_cluster_size.  At a node of weight w inside cluster C with child sizes nL, nR: both
 *               >= M: C ends at w, two clusters are born at w and all rows of C leave C at w; exactly one < M: that child's rows
 *               leave C at w and C goes on into the other child; both < M: all rows leave C at w.  The root cluster is born at the
 *               weight of the last edge
 *   stability   S(C) = the sum over C's leave events, in the order they are met walking down, of
 *               (double)size * (w_event - w_birth): f64, one subtraction, one multiplication, one addition per event, never
 *               contracted into an FMA
 *   selection   bottom-up.  A cluster without child clusters has T(C) = S(C); otherwise T_children = T(left) + T(right), left the
 *               child that holds the lower position; S(C) >= T_children: C replaces its descendants and T(C) = S(C), otherwise
 *               T(C) = T_children.  The root is a candidate only if allow_single != 0
 *   out_label   [n_rows] the selected cluster that is the cluster the row was in when it left, or an ancestor of it; -1 if there is
 *               none or the row takes no part.  Selected clusters are numbered 0, 1, ... by the lowest position of their labelled rows
 *   out_clusters      the number of selected clusters; may be NULL
 *   out_stability, out_size  [cluster_capacity] S and the labelled rows of the first cluster_capacity selected clusters; may be NULL */
pcv_status pcv_linkage_select(const int64_t* pos_a, const int64_t* pos_b, const double* w, int64_t n_edges, const int8_t* part,
                              int64_t n_rows, int64_t min_cluster_size, int allow_single, int32_t* out_label, int32_t* out_clusters,
                              double* out_stability, int64_t* out_size, int64_t cluster_capacity);

/* Seed items: k stored items that cover the corpus, picked one after the other where the rows live — the init pcv_searcher_kmeans
 * asks for (k-means++), or a representative sample whose covering radii tell how many topics a library holds (farthest first).
 * The rows concerned are those of the selected segments in global position order, as in pcv_searcher_neighbors; source_ids == NULL
 * means all sources, an empty list selects nothing; a view seeds its own rows (and numbers positions from 0, in its parent's
 * order).  A row TAKES PART under exactly the rules of pcv_searcher_neighbors / _find_duplicates: a pcv_searcher_search with the same
 * filter could return it (scale != 0, not hidden) and it has a cosine (canonical |x|^2 in [2^-126, inf)).  c(r, s) is the canonical
 * cosine of two stored f32 rows — f64, products exact, sums in feature order — for BOTH metrics.
 *   cover_j(r)   the largest c(r, s) over the seeds s_0 .. s_{j-1} picked so far (undefined before the first)
 *   w_0(r) = 1;  w_j(r) = (int64) rint(max(0, 1 - cover_j(r)) * 2^32), ties to even, for j >= 1: an integer in [0, 2^33]; a seed's own
 *                weight is 0 (c(r, r) is within 2^-51 of 1)
 *   T_j          the sum of w_j over the participating rows — exact, the addition is in integers, whatever its order
 * Step j = 0 .. k-1: if T_j == 0 the call stops with *out_count = j (every row left points the way of some seed, or there are no
 * rows).  Otherwise
 *   PCV_SEED_FARTHEST  picks the participating row with the largest w_j, ties to the lower global position (step 0: the first
 *                      participating row);
 *   PCV_SEED_KMEANSPP  draws t = pcv_seed_draw(seed, j, T_j) and picks the first row by global position whose inclusive prefix sum
 *                      of w_j exceeds t: row r with probability w_j(r) / T_j.
 * first_id (may be NULL): step 0 picks the first participating row by position that carries this item id instead; if none does the
 * call fails with PCV_ERR_INVALID and writes no output.
 *   k              1 .. PCV_MAX_SEEDS
 *   out_ids        [k] the seeds' item ids; unused slots -1
 *   out_positions  [k] their global positions; unused slots -1
 *   out_totals     [k] T_j, the potential before pick j in units of 2^-32; unused slots 0
 *   out_cover      [k] (float)cover_j(s_j), NaN at step 0 and in unused slots; under the farthest rule 1 - out_cover[j] is the covering
 *                  radius the first j seeds leave
 *   out_count      steps taken
 * The result is a pure function of rows, filter, k, method, seed and first id: it does not depend on which screening copies exist,
 * nor on pcv_searcher_set_kernel, _set_tuning or _set_candidate_capacity.  The call reads the f32 rows and touches no pass state
 * (DESIGN.md §4 "Seed items"); everything it allocates on the device — 20 bytes per row and 24 per 256 rows — is given back when it
 * returns.  A NULL searcher or output, k or method out of range give PCV_ERR_INVALID before the handle is looked at; a searcher with
 * pending rows fails as in pcv_searcher_search.  More than 2^30 participating rows give PCV_ERR_UNSUPPORTED (the int64 potential).
 * Not in scope: a sharded searcher (pcv_searcher_set_shard_offset != 0 or a pcv_comm) — PCV_ERR_INVALID — and device-resident output. */
enum { PCV_SEED_FARTHEST = 0, PCV_SEED_KMEANSPP = 1 };
enum { PCV_MAX_SEEDS = 4096 };
pcv_status pcv_searcher_seeds(pcv_searcher* s, const int64_t* source_ids, int n_sources, int k, int method, uint64_t seed,
                              const int64_t* first_id, int64_t* out_ids, int64_t* out_positions, int64_t* out_totals,
                              float* out_cover, int32_t* out_count);

/* Counters of the most recent pcv_searcher_seeds on this handle. */
typedef struct pcv_seed_stats {
    int64_t rows;           /* rows of the selected segments (those taking no part included)              */
    int64_t participating;  /* rows that take part (T_0)                                                  */
    int32_t steps;          /* seeds picked                                                               */
    int32_t method;
    float prep_ms;          /* hipEvent times: the norms (selfjoin_prep_kernel), then every cover and pick */
    float steps_ms;
} pcv_seed_stats;
pcv_status pcv_searcher_last_seed_stats(pcv_searcher* s, pcv_seed_stats* out);

/* The draw of step `step` (host only: needs no context and no GPU; the device calls the same function):
 * floor(z * total / 2^64) with z the splitmix64 finaliser of seed + (step + 1) * 0x9E3779B97F4A7C15 (mod 2^64):
 *   z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 * always below total.  total == 0, step < 0 or a NULL out_t give PCV_ERR_INVALID. */
pcv_status pcv_seed_draw(uint64_t seed, int step, uint64_t total, uint64_t* out_t);

/* Corpus moments and principal axes: the mean direction of a corpus, how its variance is spread over directions, and every row's
 * position along a handful of directions — a PCA where the rows live, without downloading N x dim floats and without a LAPACK.
 * Rules shared by pcv_searcher_moments, _principal_axes and _project: the rows concerned are those of the selected segments in global
 * position order, as in pcv_searcher_neighbors; source_ids == NULL means all sources, an empty list selects nothing; a view uses its
 * own rows.  A row TAKES PART under exactly the rules of pcv_searcher_neighbors / _label_sums: a pcv_searcher_search with the same
 * filter could return it (scale != 0, not hidden) and it has a cosine (canonical |x|^2 in [2^-126, inf)).  rinv_r =
 * (float)(1 / sqrt(|x_r|^2)) and t(r, d) = (int64) rint((double)x[r][d] * (double)rinv_r * 2^32) are those of pcv_searcher_label_sums:
 * both metrics work on unit rows, as k-means, neighbours and seeds do.  The calls read the f32 rows, touch no pass state and depend on
 * no screening copy, kernel or tuning setting; every device allocation is given back on return.  Argument errors are reported before
 * the handle is looked at; a searcher with pending rows fails as in pcv_searcher_search; a sharded searcher
 * (pcv_searcher_set_shard_offset != 0 or a pcv_comm) gives PCV_ERR_INVALID.  Not in scope: a sharded form, device-resident output,
 * incremental moments, partial eigen-solvers (DESIGN.md §4 "Corpus moments and principal axes").
 *
 * pcv_searcher_moments: the integer first and second moments of the unit rows, the same bits in any order of addition.
 *   out_n        n, the number of participating rows
 *   out_sums     [dim] int64: S_d = sum over the participating rows of t(r, d); the mean unit row is S_d * 2^-32 / n
 *   out_matrix   [dim][dim] f64, or NULL: then only the sums are computed and the rows are not streamed a second time.  With
 *                C_de = sum of t(r, d) * t(r, e), an exact integer of up to 94 bits,
 *                  centered == 0: (double)C_de * 2^-64                        n times the second moment
 *                  centered != 0: (double)(n * C_de - S_d * S_e) * 2^-64      n^2 times the covariance
 *                the one rounding is that of the exact integer to double, to nearest even; the power of two is exact
 * More than 2^30 participating rows, or dim > 2048, give PCV_ERR_UNSUPPORTED.  The device holds 12 bytes per row and three
 * Dp x Dp int64 matrices (Dp: dim rounded up to 64) for the call. */
pcv_status pcv_searcher_moments(pcv_searcher* s, const int64_t* source_ids, int n_sources, int centered, int64_t* out_sums,
                                double* out_matrix, int64_t* out_n);

/* The host finish of pcv_searcher_moments (host only: needs no context and no GPU; pcv_searcher_moments calls it).  hh, hl, ll are
 * [dim][dim] int64 limb sums over the participating rows with t = h * 2^16 + l, h = t >> 16 (arithmetic), l = t & 0xffff:
 * hh[d][e] = sum h_d h_e, hl[d][e] = sum h_d l_e, ll[d][e] = sum l_d l_e; hh and ll are read on and above the diagonal only.  In 128-bit
 * integers C_de = hh[d][e] * 2^32 + (hl[d][e] + hl[e][d]) * 2^16 + ll[d][e], then out_matrix[d][e] = out_matrix[e][d] as defined above
 * (sums [dim] and n are read only when centered != 0).  n in [0, 2^30], dim >= 1, else PCV_ERR_INVALID. */
pcv_status pcv_moments_finish(const int64_t* hh, const int64_t* hl, const int64_t* ll, const int64_t* sums, int64_t n, int dim,
                              int centered, double* out_matrix);

/* Counters of the most recent pcv_searcher_moments (or _principal_axes) on this handle. */
typedef struct pcv_moment_stats {
    int64_t rows;           /* rows of the selected segments (those taking no part included)                   */
    int64_t participating;  /* n                                                                               */
    int32_t tile_features;  /* a workgroup of the second-moment kernel owns tile_features x tile_features outputs */
    int32_t row_ranges;     /* row ranges the rows were cut in: one f64 accumulation chain each (0: no matrix)  */
    float prep_ms;          /* hipEvent times: the norms (selfjoin_prep_kernel), the sums, the second moments   */
    float sums_ms;
    float syrk_ms;
} pcv_moment_stats;
pcv_status pcv_searcher_last_moment_stats(pcv_searcher* s, pcv_moment_stats* out);

/* Eigenvalues and eigenvectors of a symmetric matrix by cyclic Jacobi rotations (host only: needs no context and no GPU, no LAPACK).
 * a is [n][n] f64, read from the upper triangle (a[i][j], i <= j); every value read must be finite.
 *   out_values   [n] descending
 *   out_vectors  [n][n]: out_vectors[i] is the unit eigenvector of out_values[i], its sign fixed so that its component of largest
 *                magnitude (the lowest index on ties) is positive
 * The sequence of rotations is deterministic, but no bit-for-bit promise is made across compilers (FMA contraction).  1 <= n <= 2048,
 * else PCV_ERR_INVALID.  An OFFLINE call: O(n^3) per sweep on one thread, seconds at n = 384. */
pcv_status pcv_symmetric_eigen(const double* a, int n, double* out_values, double* out_vectors);

/* The m leading principal axes of the unit rows: pcv_searcher_moments with centered = 1, then pcv_symmetric_eigen.
 *   out_axes      [m][dim] f32: (float) of eigenvector j of the covariance, j < m
 *   out_offsets   [m] f64: the feature-order f64 sum of (double)out_axes[j][d] * ((double)S_d * 2^-32 / (double)n) — the mean unit row
 *                 along axis j, what pcv_searcher_project subtracts
 *   out_variance  [m] f64: lambda_j / n^2, the variance of the unit rows along axis j
 *   out_n         n
 * 1 <= m <= PCV_MAX_AXES and m <= dim (PCV_ERR_INVALID); n == 0 gives PCV_ERR_INVALID (out_n is set). */
enum { PCV_MAX_AXES = 64 };
pcv_status pcv_searcher_principal_axes(pcv_searcher* s, const int64_t* source_ids, int n_sources, int m, float* out_axes,
                                       double* out_offsets, double* out_variance, int64_t* out_n);

/* The canonical score of every row against m vectors, written out in full: principal coordinates, linear probes, hand-made "topic
 * axes".  axes is host [m][dim] f32, every value finite; offsets host [m] f64 (finite), or NULL: zeros.  For a participating row
 *   coord(r, j) = (float)(a(r, j) * (double)rinv_r - offsets[j])
 * with a(r, j) the canonical f64 dot of axes[j] with the stored row — products exact, summed in feature order starting from +0
 *  — and the multiplication and the subtraction rounded separately (no fused multiply-add).  Rows that take no part
 * get NaN in all m slots.
 *   capacity     rows the outputs have room for; capacity < n gives PCV_ERR_INVALID (out_n is set)
 *   out_coords   [capacity][m] f32, in global position order
 *   out_ids      [capacity] the item id of every position (may be NULL)
 *   out_n        n, the rows of the selected segments.  With out_coords == NULL and capacity == 0 the call only reports n
 * 1 <= m <= PCV_MAX_AXES, else PCV_ERR_INVALID. */
pcv_status pcv_searcher_project(pcv_searcher* s, const float* axes, const double* offsets, int m, const int64_t* source_ids,
                                int n_sources, int64_t capacity, float* out_coords, int64_t* out_ids, int64_t* out_n);

/* Counters of the most recent pcv_searcher_project on this handle. */
typedef struct pcv_project_stats {
    int64_t rows;       /* rows of the selected segments (those taking no part included)      */
    int32_t axes;       /* m                                                                  */
    int32_t group;      /* axes scored per pass over a row's pieces (2 or 8)                  */
    float prep_ms;      /* hipEvent times: the norms (selfjoin_prep_kernel), the projection   */
    float project_ms;
} pcv_project_stats;
pcv_status pcv_searcher_last_project_stats(pcv_searcher* s, pcv_project_stats* out);

/* Groups of duplicates from a list of pairs (host only: needs no context and no GPU).  out_ids receives the distinct ids occurring
 * in the n_pairs pairs, ascending, and out_group[i] the smallest id of the connected component of out_ids[i]: an item is a candidate
 * for removal iff out_group[i] != out_ids[i].  out_n_ids receives the number of distinct ids; capacity < that gives PCV_ERR_INVALID
 * (out_n_ids is set, nothing else is written). */
pcv_status pcv_duplicate_groups(const int64_t* id_a, const int64_t* id_b, int64_t n_pairs, int64_t* out_ids, int64_t* out_group,
                                int64_t capacity, int64_t* out_n_ids);

/* Search by example (`perceive search --like <id>`, perceive-cli/cmd/search.rs:17-19, 64-86: the stored embedding of an item is
 * the query): query vectors are built on the device from rows the searcher already holds, found by item id.
 * Query q is built from the examples example_ids[offsets[q] .. offsets[q+1]) with the weights weights[...] (NULL: all 1);
 * offsets has n_queries + 1 entries, ascending from 0.
 *   - members: the members of a query are all rows carrying one of its example ids, in every source, explicit-id and implicit-id
 *     segments alike (ids == NULL rows: id0 + row).  Rows staged under PCV_STAGING_SOURCE are left out.  Hidden rows count (their
 *     f32 row is still stored).  An id listed twice in a group counts twice; the same id may appear in several groups;
 *   - vector: component c of query q is the f32 value of acc = fmaf(w_i, x_r[c], acc), starting from zero, over the examples i in
 *     the order given and, within an example, over that item's rows r in ascending global position; x is the stored f32 row, the
 *     value pcv_searcher_get_rows returns.  The order is part of the contract: one example of weight 1 with one row reproduces that
 *     row bit for bit (the sum starts from the zero that keeps the sign of a zero product, -0), and the same call gives the same
 *     bits every time.  Nothing is normalised: under PCV_METRIC_DOT one example gives exactly the reference's --like query;
 *   - not found: an example id that no row carries sets out_found[i] = 0 and contributes nothing; a query without any member is
 *     the zero vector (+0) in like_queries, and has count 0, ids -1 and NaN scores in search_like.  Neither is an error;
 *   - outputs of like_queries, each may be NULL: out_queries host [n_queries][dim], d_out_queries device [n_queries][dim] (both
 *     complete when the call returns), out_found [offsets[n_queries]], out_member_rows [n_queries] rows that went into each query;
 *   - search: search_like returns exactly what pcv_searcher_search returns for the vectors like_queries builds — same source
 *     filter, metric, order, ties, exactness, any k —, on host arrays shaped like pcv_searcher_search's outputs;
 *   - exclusion: with exclude_examples != 0 no row carrying one of query q's OWN example ids is a result of query q; the result is
 *     the exact top-k of the remaining rows (counts below k only when fewer remain) and does not depend on how it is computed:
 *     the call searches k + m, m = the most rows any query's example ids are carried by, and drops them by id — at most m rows of
 *     a query are dropped, and num_results is not limited.  exclude_examples == 0 is the reference's behaviour (the item itself is
 *     hit 1).  k + m may not pass 2^24;
 *   - views: both calls take a view.  The examples are looked up in the view's PARENT (an example need not be among the allowed
 *     items); the search runs over the view;
 *   - state: a finalized searcher (PCV_ERR_INVALID with pending rows) and no queued pass, as hide_ids.  NULL s, NULL offsets,
 *     NULL example_ids with examples, n_queries < 0, offsets[0] != 0, descending offsets or a non-finite weight give
 *     PCV_ERR_INVALID before anything touches the device.  n_queries == 0 succeeds and writes nothing;
 *   - read-only: rows, copies, the hidden set and the mid-copy statistics are as they were, apart from what a search books;
 *     pcv_searcher_last_stats afterwards describes the search of search_like.
 * A sharded host: an example lives on one rank; like_queries on each rank yields that rank's partial sums (no collective form). */
pcv_status pcv_searcher_like_queries(pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets,
                                     int n_queries, float* out_queries, void* d_out_queries, uint8_t* out_found,
                                     int64_t* out_member_rows);
pcv_status pcv_searcher_search_like(pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets,
                                    int n_queries, const int64_t* source_ids, int n_sources, int k, int exclude_examples,
                                    int64_t* out_ids, float* out_scores, int* out_counts, uint8_t* out_found);

/* One entry of a per-shard result list, the unit exchanged between GPUs (all-gather payload). */
typedef struct pcv_hit {
    double score;  /* canonical f64 score (cosine or dot)                 */
    int64_t pos;   /* global row position (shard offset already applied)  */
    int64_t id;    /* item id                                             */
} pcv_hit;

/* Row position offset of this searcher's shard inside the whole (multi-GPU) corpus. */
pcv_status pcv_searcher_set_shard_offset(pcv_searcher* s, int64_t first_global_pos);

/* Local (per-shard) exact top-k, results left on the device: `d_out` is a DEVICE pointer to
 * [n_queries][k] pcv_hit; unfilled entries have pos = -1.  Runs on the context stream; the call
 * returns after every pass has been collected (`async` is accepted for compatibility and ignored: use
 * the begin/end pair below to overlap an exchange with the host). */
pcv_status pcv_searcher_search_device(pcv_searcher* s, const float* queries, int n_queries,
                                      const int64_t* source_ids, int n_sources, int k, void* d_out,
                                      int async);

/* The same per-shard search split in two so that the exchange can be queued behind it without a host
 * round trip.  `begin` queues the whole pass on the context stream and returns at once; `d_out` then
 * holds n_queries*k hits followed by ONE extra pcv_hit whose `pos` is 1 if the pass must be repeated —
 * a candidate list overflowed, or a speculative start threshold did not hold (pcv_scan_stats) — and the
 * hits are then incomplete; else 0.  `end` waits for the stream, books the statistics and prepares the
 * repeat (larger lists; no guess).
 * No other call may use the searcher between the two.  PCV_ERR_UNSUPPORTED only when n_queries exceeds
 * one pass (use pcv_searcher_search_device then) — a condition every rank of a sharded search evaluates
 * alike, so all ranks exchange the same payload; a shard that holds none of the selected sources delivers
 * the same layout (empty lists, clear overflow record).  One launch takes any number of segments.
 * Typical step:
 *   begin -> all-gather of (n*k+1)*24 bytes -> pcv_merge_topk_flagged -> end -> repeat if any_overflow. */
pcv_status pcv_searcher_search_device_begin(pcv_searcher* s, const float* queries, int n_queries,
                                            const int64_t* source_ids, int n_sources, int k, void* d_out);
/* `begin` with the queries in DEVICE memory ([n_queries][dim] f32 at d_queries, valid until `end`): embeddings that
 * pcv_model_encode_tokens_device left on the GPU (and an all-gather put together) go into the scan without a host hop —
 * the chain of BASELINE configs[4], model.rs:176 -> search.rs:157 with nothing in between. */
pcv_status pcv_searcher_search_device_begin_dq(pcv_searcher* s, const void* d_queries, int n_queries,
                                               const int64_t* source_ids, int n_sources, int k, void* d_out);
pcv_status pcv_searcher_search_device_end(pcv_searcher* s, int* out_overflowed);
/* How many queries a pass takes is part of a sharded search's protocol (every rank must split a batch alike), so among ranks a pass
 * is what every searcher can take whatever copies it holds: 128 queries.  A host that KNOWS every rank's searcher keeps the int8
 * screening copy of all its rows (pcv_scan_stats.screening_copy == 2 on every rank, e.g. agreed with one all-reduce) may say so on
 * every rank: a pass among ranks then takes what the int8 scan takes — 256 queries up to 384-d, the 256 embeddings of BASELINE
 * configs[4] in one pass instead of two.  A rank for which it is not true fails pcv_searcher_search_device_begin* /
 * pcv_searcher_search_sharded* with PCV_ERR_UNSUPPORTED before queueing anything (the other ranks' exchange would wait for it:
 * check first). */
pcv_status pcv_searcher_allow_wide_sharded_pass(pcv_searcher* s, int on);
/* A step of a sharded search is about to be repeated because SOME rank's pass was incomplete (any_overflow of
 * pcv_merge_topk_flagged): the repeat on THIS rank runs without a speculative start threshold as well.  Every rank
 * keeps its own guess statistics; without this call guesses could fail on different ranks in different attempts and
 * every such failure would make all ranks repeat.  Call it on every rank between `end` and the next `begin`. */
pcv_status pcv_searcher_repeat_without_guess(pcv_searcher* s);

/* Cross-shard merge (replaces the rayon flat_map + sort + truncate of search.rs:163-181):
 * `d_lists` is a DEVICE pointer to [n_shards][n_queries][k] pcv_hit (the all-gather result),
 * written to host arrays shaped like pcv_searcher_search's outputs. */
pcv_status pcv_merge_topk(pcv_ctx* ctx, int metric, int dim, const void* d_lists, int n_shards, int n_queries,
                          int k, int64_t* out_ids, float* out_scores, int* out_counts);

/* pcv_merge_topk for lists produced by pcv_searcher_search_device_begin: shards are n_queries*k+1
 * records apart; *out_any_overflow = OR of the shards' overflow records (identical on every rank). */
pcv_status pcv_merge_topk_flagged(pcv_ctx* ctx, int metric, int dim, const void* d_lists, int n_shards,
                                  int n_queries, int k, int64_t* out_ids, float* out_scores, int* out_counts,
                                  int* out_any_overflow);

/* The same merge on host memory (`lists` = host pointer, same shape): the reference's own merge is
 * host code (search.rs:179-180 sort + truncate); used when the lists were gathered on the host and
 * by the CPU-side (gloo) tests of the multi-GPU protocol.  Needs no GPU. */
pcv_status pcv_merge_topk_host(int metric, int dim, const pcv_hit* lists, int n_shards, int n_queries, int k,
                               int64_t* out_ids, float* out_scores, int* out_counts);

/* ---- native RCCL exchange (no PyTorch in the data path) ----------------------------------------
 * One communicator per process/GPU.  RCCL (librccl.so.1) is loaded on first use; PCV_ERR_UNSUPPORTED if
 * it is not installed.  Bootstrap: rank 0 calls pcv_comm_unique_id and hands the 128 bytes to every rank
 * by whatever channel the host has (torchrun's store, MPI, a file); all ranks then call pcv_comm_create. */
typedef struct pcv_comm pcv_comm;
pcv_status pcv_comm_unique_id(uint8_t out_id[128]);
pcv_status pcv_comm_create(pcv_ctx* ctx, int world_size, int rank, const uint8_t id[128], pcv_comm** out);
pcv_status pcv_comm_destroy(pcv_comm* c);
/* Sharded Searcher::search_vector: local exact top-k on this rank's shard, ncclAllGather of the
 * [n_queries][k] pcv_hit lists over xGMI (on the context stream), merge on every rank.  Collective: every
 * rank of the communicator must call it with the same queries / k.  Outputs as pcv_searcher_search. */
pcv_status pcv_searcher_search_sharded(pcv_searcher* s, pcv_comm* c, const float* queries, int n_queries,
                                       const int64_t* source_ids, int n_sources, int k, int64_t* out_ids,
                                       float* out_scores, int* out_counts);
/* The same with the queries in DEVICE memory (the same on every rank), and the all-gather that puts them there: every rank
 * contributes bytes_per_rank bytes at d_send and receives world_size x bytes_per_rank at d_recv (rank order; d_send may be
 * this rank's slot of d_recv), on the context stream — data-parallel pcv_model_encode_tokens_device output -> all ranks hold
 * all embeddings -> pcv_searcher_search_sharded_dq, nothing passing through host memory. */
pcv_status pcv_searcher_search_sharded_dq(pcv_searcher* s, pcv_comm* c, const void* d_queries, int n_queries,
                                          const int64_t* source_ids, int n_sources, int k, int64_t* out_ids,
                                          float* out_scores, int* out_counts);
pcv_status pcv_comm_all_gather(pcv_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank);

/* Brute-force similarity matrices of lib.rs:63-77 for small inputs (tests, highlight.rs:109):
 *   out[b][n] = dot(a_b, m_n)                       pcv_dot_product            (lib.rs:63-65)
 *   out[b][n] = cos(a_b, m_n)                       pcv_cosine_similarity      (lib.rs:67-77)
 * a: [B][dim], m: [N][dim], out: [B][N], all host f32.  Computed on the GPU in f32. */
pcv_status pcv_dot_product(pcv_ctx* ctx, const float* a, int B, const float* m, int64_t N, int dim,
                           float* out);
pcv_status pcv_cosine_similarity(pcv_ctx* ctx, const float* a, int B, const float* m, int64_t N, int dim,
                                 float* out);

/* Counters of the most recent search on this handle (diagnostics + bench roofline). */
typedef struct pcv_scan_stats {
    int64_t rows_scanned;        /* rows streamed by the scan kernel(s), padding excluded        */
    int64_t bytes_algorithmic;   /* rows_scanned * dim * 4                                       */
    float scan_ms;               /* hipEvent time of the scan kernel launches only (a pass over <= 4M rows replayed as a
                                    hipGraph is timed as a whole: then total_ms times the share last measured) */
    float total_ms;              /* hipEvent time of the whole device pipeline                   */
    int64_t candidates;          /* rows rescored exactly, summed over queries                   */
    int32_t scan_launches;       /* scan kernel launches (reruns after overflow included)        */
    int32_t overflow_reruns;     /* passes repeated because a candidate list overflowed          */
    int32_t kernel_used;         /* PCV_KERNEL_WAVE or PCV_KERNEL_MFMA                           */
    int32_t screening_copy;      /* what the scan streamed (last pass): 0 f32 rows, 1 bf16 copy, 2 int8 copy or its 6-bit form (screen_bits) */
    float host_enqueue_ms;       /* host time spent queueing the passes (copies + launches)      */
    float host_wait_ms;          /* host time blocked until the stream had drained               */
    int64_t bytes_streamed;      /* bytes the scan kernel(s) had to read from HBM, layout padding included: per 32-row block
                                    the f32 pieces + 32 row scales, or the bf16 pieces, or the int8 pieces + the block's scale */
    int32_t speculation_reruns;  /* passes repeated because a speculative start threshold (a guess taken from the seed
                                    rows and checked at the end of the pass) did not hold; results are exact either way */
    int32_t mid_copy;            /* 1 if the last pass had the mid copy of every selected segment (pcv_searcher_set_mid_copy) */
    int64_t coarse_survivors;    /* MFMA scans: (row, query) pairs that passed the coarse screen and had their f32 row read
                                    by the fine screen, summed over queries and launches */
    int64_t mid_survivors;       /* ... and those of them that also passed the mid screen (= f32 rows read), when a mid copy exists */
    int64_t narrow_survivors;    /* passes that streamed the 6-bit copy: (row, query) pairs that passed its screen and had their int8
                                    row read (of them, coarse_survivors passed the int8 screen too), summed over queries and launches */
    int32_t screen_bits;         /* width of the copy the coarse screen streamed (last pass): 8 int8, 6 its 6-bit form, 0 none */
} pcv_scan_stats;
pcv_status pcv_searcher_last_stats(pcv_searcher* s, pcv_scan_stats* out);

/* ---- Model (model.rs:56-191, model/worker.rs:78-106) ---------------------------------------- */

/* Transformer description: what rust-bert reads from config.json / modules.json /
 * 1_Pooling/config.json (model.rs:84-151). */
typedef struct pcv_model_desc {
    int32_t vocab_size;          /* 30522 for all-MiniLM-L6-v2                                  */
    int32_t hidden;              /* 384                                                         */
    int32_t layers;              /* 6                                                           */
    int32_t heads;               /* 12                                                          */
    int32_t intermediate;        /* 1536                                                        */
    int32_t max_positions;       /* 512                                                         */
    int32_t type_vocab;          /* 2                                                           */
    float layer_norm_eps;        /* 1e-12                                                       */
    int32_t pooling;             /* PCV_POOL_*                                                  */
    int32_t normalize;           /* modules.has_normalization(), model.rs:151                   */
    int32_t dense_out;           /* 0 = no Dense module; else output width (model.rs:139-149)   */
    int32_t dense_activation;    /* PCV_ACT_* of the Dense module                               */
    int32_t max_seq_length;      /* sentence_bert_config.max_seq_length (tokenize.rs:66)        */
    int32_t compute;             /* PCV_COMPUTE_*                                               */
    /* ALBERT (ParaphraseAlbertSmallV2, configs.rs:35); all three 0 for the BERT-family models */
    int32_t embedding_size;      /* width of the embedding tables when they are factorised (0 = hidden): a Linear
                                    embedding_size -> hidden follows the embedding LayerNorm       */
    int32_t shared_layers;       /* != 0: every layer runs with the weights of layer 0              */
    int32_t hidden_act;          /* PCV_GELU_ERF (BERT's "gelu") or PCV_GELU_TANH ("gelu_new")      */
} pcv_model_desc;
enum { PCV_GELU_ERF = 0, PCV_GELU_TANH = 1 };
enum { PCV_POOL_MEAN = 0, PCV_POOL_CLS = 1, PCV_POOL_MAX = 2, PCV_POOL_MEAN_SQRT_LEN = 3 };
enum { PCV_ACT_IDENTITY = 0, PCV_ACT_TANH = 1 };
/* F32   : every GEMM on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32), the reference's dtype.
 * BF16X3: each f32 operand is split into three bf16 terms (hi + mid + lo = 24 significand bits) and
 *         a product is six bf16 MFMAs accumulated in f32 (the lo*mid, mid*lo, lo*lo terms, < 2^-24
 *         relative, are dropped): f32-level accuracy at 6/16 of the f32-MFMA cost.
 * F16X2 : each f32 operand is split into two f16 terms (11 + 11 significand bits, |x - hi - lo| <= 2^-24 |x|)
 *         and a product is three f16 MFMAs (lo*lo dropped): the same accuracy at half the matrix time of
 *         BF16X3.  Operands are rescaled by exact powers of two so the low terms stay normal; it needs
 *         |activation| < 4094 and |weight| < 255 (checked for weights when the model is built). */
enum { PCV_COMPUTE_F32 = 0, PCV_COMPUTE_BF16X3 = 1, PCV_COMPUTE_F16X2 = 2 };

/* Fill `d` with the all-MiniLM-L6-v2 shape. */
void pcv_model_desc_minilm_l6(pcv_model_desc* d);

/* Model::new_pretrained, transformer part (model.rs:117-151).  `weights_path` is a flat weight
 * file in this library's own format; NULL = seeded synthetic weights
 * (synth_weight(seed, tensor, index)), the only form available offline. */
pcv_status pcv_model_create(pcv_ctx* ctx, const pcv_model_desc* desc, const char* weights_path,
                            uint64_t synthetic_seed, pcv_model** out);
pcv_status pcv_model_destroy(pcv_model* m);
pcv_status pcv_model_output_dim(pcv_model* m, int* out_dim);
/* Overwrite one named tensor from host f32 data (tests load oracle weights through this). */
pcv_status pcv_model_set_tensor(pcv_model* m, const char* name, const float* data, int64_t n);
/* Copy one named tensor to the host (for oracles that must share the synthetic weights). */
pcv_status pcv_model_get_tensor(pcv_model* m, const char* name, float* out, int64_t cap, int64_t* out_n);

/* WorkerData::encode_tokens (worker.rs:78-106): ids/mask are [B][L] int64 row-major exactly as
 * generate_token_tensors lays them out (tokenize.rs:13-51: right-padded, mask = id != pad).
 * out: [B][output_dim] f32. */
pcv_status pcv_model_encode_tokens(pcv_model* m, const int64_t* ids, const int64_t* mask, int B, int L,
                                   float* out);
/* Same with the output left on the device (DEVICE pointer d_out, [B][output_dim] f32). */
pcv_status pcv_model_encode_tokens_device(pcv_model* m, const int64_t* ids, const int64_t* mask, int B,
                                          int L, void* d_out, int async);
/* Per-layer hidden states of the last encode (test hook): layer 0 = embedding output,
 * 1..layers = encoder layer outputs, [B][L][hidden] f32. */
pcv_status pcv_model_debug_hidden(pcv_model* m, int layer, float* out, int64_t cap);

typedef struct pcv_encode_stats {
    float total_ms;      /* hipEvent time of the whole forward                                  */
    double flops;        /* algorithmic FLOPs of the forward (SURVEY.md §8 row D formula)       */
    int32_t batch, seq_len;
} pcv_encode_stats;
pcv_status pcv_model_last_stats(pcv_model* m, pcv_encode_stats* out);

/* ---- Model, text side (model.rs:68-179, model/highlight.rs) -------------------------------------------
 * The host logic that sits between text and the device forward — model directories, tokenisation of a
 * batch, chunk planning and offset mapping of highlight — in the library, so that a Rust / C++ host gets
 * the whole of Model::{new_pretrained, encode, highlight} from this ABI. */

/* Directory name of a SentenceEmbeddingsModelType variant under model_data/ (configs.rs:30-69,121-141):
 * 0 AllMiniLmL6V2 .. 7 MsMarcoBertBaseDotV5, the enum order, which is also model_id() (configs.rs:72-83).
 * NULL for an unknown value. */
const char* pcv_model_type_dir_name(int model_type);

/* Model::new_pretrained (model.rs:68-174) from a sentence-transformers model directory: modules.json,
 * config.json, sentence_bert_config.json, tokenizer_config.json, vocab.txt (or vocab.json + merges.txt, or spiece.model),
 * <n>_Pooling/config.json, optional <n>_Dense/{config.json, weights}.  BERT, DistilBERT, RoBERTa and ALBERT
 * (spiece.model; one layer group) transformers: all eight variants of configs.rs:30-39.  The model owns its tokenizer.
 *   compute       PCV_COMPUTE_*
 *   load_weights  != 0: read the weights file of the directory — rust_model.ot (what the reference loads,
 *                 configs.rs:109,112), else model.safetensors, else pytorch_model.bin; see pcv_checkpoint_visit;
 *                 0: leave the weights to the caller — hand every checkpoint tensor to pcv_model_load_hf_tensor,
 *                 then pcv_model_check_loaded. */
pcv_status pcv_model_create_from_dir(pcv_ctx* ctx, const char* model_dir, int compute, int load_weights, pcv_model** out);
/* What pcv_model_create_from_dir would build, from the directory's JSON files alone (needs no GPU): the model
 * description, the transformer family (0 BERT, 1 DistilBERT, 2 RoBERTa, 3 ALBERT) and the tokenizer options
 * (strip_accents: -1 = follow lower_case).  Any output pointer may be NULL. */
pcv_status pcv_model_dir_describe(const char* model_dir, pcv_model_desc* out_desc, int* out_arch, int* out_lower_case,
                                  int* out_strip_accents);
/* Walk a checkpoint file: model.safetensors, or a libtorch zip archive — rust_model.ot as tch's
 * Tensor::save_multi writes it (VarStore::load, model.rs:117-124) or a torch.save state dict (pytorch_model.bin).
 * The archive's pickle is interpreted by a closed machine that knows only the tensor / dict / module records those
 * writers emit; nothing from the file is executed, an unknown record is PCV_ERR_UNSUPPORTED.
 * `visit` is called once per tensor in file order: shape[rank], dtype PCV_TENSOR_*, values = numel row-major f32
 * converted from the stored dtype (NULL for PCV_TENSOR_OTHER: integer tensors such as position_ids).  A non-zero
 * return from `visit` stops the walk with PCV_ERR_INVALID.  Needs no GPU. */
enum { PCV_TENSOR_F32 = 0, PCV_TENSOR_F16 = 1, PCV_TENSOR_BF16 = 2, PCV_TENSOR_F64 = 3, PCV_TENSOR_OTHER = 4 };
typedef int (*pcv_tensor_visitor)(void* user, const char* name, const int64_t* shape, int rank, int dtype, const float* values,
                                  int64_t numel);
pcv_status pcv_checkpoint_visit(const char* path, pcv_tensor_visitor visit, void* user);
/* One checkpoint tensor under its Hugging Face / rust-bert name ("bert.encoder.layer.0...", DistilBERT and
 * RoBERTa names included: they are mapped onto the encoder graph, the RoBERTa position table is shifted);
 * names the graph does not use are ignored.  `data`: numel f32, row-major. */
pcv_status pcv_model_load_hf_tensor(pcv_model* m, const char* hf_name, const float* data, int64_t numel);
/* PCV_ERR_IO naming a missing tensor unless every tensor of the graph has been provided. */
pcv_status pcv_model_check_loaded(pcv_model* m);
/* Give a model built by pcv_model_create its tokenizer (Model::tokenizer, model.rs:61).  take_ownership != 0:
 * the model destroys it. */
pcv_status pcv_model_set_tokenizer(pcv_model* m, pcv_tokenizer* t, int take_ownership);
/* The model's tokenizer (NULL if none); still owned as before. */
pcv_status pcv_model_tokenizer(pcv_model* m, pcv_tokenizer** out_tok);
/* The description the model was built from and the pad id its token tensors use (tokenize.rs:19). */
pcv_status pcv_model_get_desc(pcv_model* m, pcv_model_desc* out_desc, int64_t* out_pad_id);

/* Model::encode(&[S]) (model.rs:176-179): tokenize (encode_list, max_seq_length, LongestFirst; host threads),
 * pad to the batch maximum, forward.  texts[i] = n_bytes[i] bytes of UTF-8.  out: [n_texts][output_dim] f32. */
pcv_status pcv_model_encode_text(pcv_model* m, const char* const* texts, const size_t* n_bytes, int n_texts, float* out);

/* Model::highlight (model/highlight.rs:23-165): for every document the text of the chunk whose embedding has
 * the largest dot product with the query's.  Documents are tokenized without truncation, cut into chunks of
 * `chunk_size` tokens overlapping by `chunk_overlap` (<= 0 / < 0: the CHUNK_SIZE / CHUNK_OVERLAP environment
 * variables, defaults 20 / 4, highlight.rs:7-18), all chunks are encoded in batches and scored on the device.
 *   out_begin/out_end [n_docs]  byte range of the highlight inside docs[i];
 *                               -1/-1 = None (no chunk: the document is too short), begin == end = Some(""). */
pcv_status pcv_model_highlight(pcv_model* m, const char* query, size_t query_bytes, const char* const* docs, const size_t* doc_bytes,
                               int n_docs, int chunk_size, int chunk_overlap, int64_t* out_begin, int64_t* out_end);

/* ---- Tokenizer (model/tokenize.rs:60-77; rust_tokenizers BertTokenizer) -------------------------
 * Host code, like the reference's tokenizer: BERT BasicTokenizer (clean text, CJK spacing, lower-casing,
 * accent stripping, punctuation split) + greedy WordPiece over `vocab.txt` (one token per line, id =
 * line number).  Needs no GPU. */
/* TokenizerOption::from_file (model.rs:96-113).  strip_accents < 0: follow lower_case (the default of
 * rust_tokenizers / HF when tokenizer_config.strip_accents is absent). */
pcv_status pcv_tokenizer_create(const char* vocab_path, int lower_case, int strip_accents, pcv_tokenizer** out);
/* Byte-level BPE tokenizer of the RoBERTa-family models in the reference's list (AllDistilrobertaV1:
 * `RobertaTokenizer::from_file(vocab.json, merges.txt, lower_case, add_prefix_space)` in rust_tokenizers): GPT-2
 * pre-tokenization, bytes_to_unicode symbols, ranked merges, <s> ... </s> framing.  The handle works with
 * pcv_tokenizer_encode / _encode_batch / _special_ids (pad = <pad>, cls = <s>, sep = </s>). */
pcv_status pcv_tokenizer_create_bpe(const char* vocab_json_path, const char* merges_path, int add_prefix_space,
                                    pcv_tokenizer** out);
/* AlbertTokenizer::from_file(spiece.model, lower_case, strip_accents) of rust_tokenizers (what rust-bert builds for
 * ModelType::Albert, the ParaphraseAlbertSmallV2 variant of configs.rs:35): a SentencePiece unigram model file.
 * Text is cleaned, NFKC-normalised, lower-cased / stripped of accents as asked, whitespace becomes U+2581 and the
 * best-scoring segmentation is found by Viterbi; ALBERT's "<digit>," pieces are split again.  Framing is
 * [CLS] ... [SEP], padding <pad>.  strip_accents < 0 = follow lower_case. */
pcv_status pcv_tokenizer_create_sentencepiece(const char* model_path, int lower_case, int strip_accents, pcv_tokenizer** out);
/* Unicode NFKC (Unicode 13 tables) of UTF-8 `text`: what the SentencePiece path normalises with.  *out_n = bytes
 * of the result; out may be NULL to ask for the size. */
pcv_status pcv_unicode_nfkc(const char* text, size_t n_bytes, char* out, size_t cap, size_t* out_n);
pcv_status pcv_tokenizer_destroy(pcv_tokenizer* t);
pcv_status pcv_tokenizer_vocab_size(pcv_tokenizer* t, int* out_n);
/* ids of [PAD] (get_pad_id, tokenize.rs:19), [UNK], [CLS], [SEP]; -1 when the vocab lacks one */
pcv_status pcv_tokenizer_special_ids(pcv_tokenizer* t, int64_t* pad, int64_t* unk, int64_t* cls, int64_t* sep);

/* One element of encode_list(inputs, max_len, TruncationStrategy::LongestFirst, stride 0)
 * (tokenize.rs:64-75): [CLS] pieces... [SEP], truncated to max_len tokens in all.
 *   out_ids           token ids
 *   out_begin/out_end char (Unicode scalar) offsets of each token in `text`, -1 for special tokens
 *                     (TokenIdsWithOffsets::token_offsets, used by highlight.rs:129-147); may be NULL
 *   out_special       special_tokens_mask (highlight.rs:58-84); may be NULL
 *   cap               capacity of the output arrays; out_len receives the token count */
pcv_status pcv_tokenizer_encode(pcv_tokenizer* t, const char* text, size_t n_bytes, int max_len, int64_t* out_ids,
                                int32_t* out_begin, int32_t* out_end, uint8_t* out_special, int cap, int* out_len);
/* The batch form behind Model::tokenize (tokenize.rs:60-77) + generate_token_tensors (tokenize.rs:9-57):
 * text i -> row i of out_ids ([n_texts][max_len], right-padded with pad_id), out_lens[i] = token count
 * (truncated to max_len like pcv_tokenizer_encode).  Texts are spread over n_threads host threads
 * (0 = all hardware threads). */
pcv_status pcv_tokenizer_encode_batch(pcv_tokenizer* t, const char* const* texts, const size_t* n_bytes, int n_texts,
                                      int max_len, int64_t pad_id, int64_t* out_ids, int32_t* out_lens, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* PERCEIVE_HIP_H */
