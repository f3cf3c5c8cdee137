//! `Searcher` over libperceive_hip.so — replaces search.rs of the reference: the per-source HNSW graphs
//! become one exact, GPU-resident scan (recall 1.0), everything callers see stays:
//!   `SearchItem { id, score }`, `Searcher::{build, rebuild_source, search_vector, search,
//!   search_vector_and_retrieve, search_and_retrieve}`, pub field `hidden`, `encode_query`,
//!   `deserialize_embedding`, `serialize_embedding`                               (search.rs:18-294)
//! Scores keep the reference's convention: `max(0, 1 - dot/len)`, ascending (PCV_METRIC_DOT).
//! NOT COMPILED in this repository's build image (no Rust toolchain): see ../README.md.
use std::marker::PhantomData;
use std::ptr;
use std::rc::Rc;

use ahash::HashSet;
use time::OffsetDateTime;

use crate::{
    db::{Database, DbError},
    ffi,
    hip::{self, HipError},
    model::Model,
    Item, ItemMetadata,
};

#[derive(Debug, Copy, Clone)]
pub struct SearchItem {
    pub id: i64,
    pub score: f32,
}

pub struct Searcher {
    handle: *mut ffi::pcv_searcher,
    /// ids hidden after the index was built (`perceive hide`, cmd/hide.rs:17).  Kept as the pub field it
    /// is in the reference (search.rs:31-34), whose `search_vector` does not consult it either; `hide_items` /
    /// `unhide_items` keep it in step with the set the library does consult.
    pub hidden: HashSet<i64>,
}

// `&self` searches run concurrently from a thread pool in the callers (app_state.rs:52-57); the library
// serialises them on the handle
unsafe impl Send for Searcher {}
unsafe impl Sync for Searcher {}

/// rows per `pcv_searcher_add_blobs` call while streaming the build query
const BUILD_CHUNK_ROWS: usize = 8192;

impl Searcher {
    pub fn build(database: &Database, model_id: u32, model_version: u32) -> Result<Searcher, eyre::Report> {
        let conn = database.read_pool.get()?;

        let mut sources_stmt = conn.prepare("SELECT id FROM sources")?;
        let sources = sources_stmt
            .query_map([], |row| row.get::<_, i64>(0))?
            .collect::<Result<Vec<_>, _>>()?;

        let mut searcher = Searcher { handle: ptr::null_mut(), hidden: HashSet::default() };
        searcher.load_sources(&conn, model_id, model_version, &sources, None)?;
        Ok(searcher)
    }

    pub fn rebuild_source(
        &mut self,
        database: &Database,
        source_id: i64,
        model_id: u32,
        model_version: u32,
    ) -> Result<(), eyre::Report> {
        let conn = database.read_pool.get()?;
        if self.handle.is_null() {
            return self.load_sources(&conn, model_id, model_version, &[source_id], None);
        }
        // search.rs:57-79 builds the new SourceSearch first and swaps it in only on success: the replacement is staged
        // under PCV_STAGING_SOURCE; after a failure (a blob of the wrong size, an SQLite error) the old rows of the
        // source are still searchable.
        hip::check(unsafe { ffi::pcv_searcher_clear_source(self.handle, ffi::PCV_STAGING_SOURCE) })?;
        if let Err(e) = self.load_sources(&conn, model_id, model_version, &[source_id], Some(ffi::PCV_STAGING_SOURCE)) {
            unsafe {
                ffi::pcv_searcher_clear_source(self.handle, ffi::PCV_STAGING_SOURCE);
                ffi::pcv_searcher_finalize(self.handle);
            }
            return Err(e);
        }
        hip::check(unsafe { ffi::pcv_searcher_replace_source(self.handle, ffi::PCV_STAGING_SOURCE, source_id) })?;
        hip::check(unsafe { ffi::pcv_searcher_finalize(self.handle) })?;
        Ok(())
    }

    /// build_sources (search.rs:81-155): the same query, its blobs streamed into the device segments of
    /// their sources instead of into HNSW inserts.  The index is created at the first row, when the
    /// embedding width is known.
    fn load_sources(
        &mut self,
        conn: &rusqlite::Connection,
        model_id: u32,
        model_version: u32,
        sources: &[i64],
        into: Option<i64>, // Some(id): every row goes to that (staging) source instead of its own
    ) -> Result<(), eyre::Report> {
        let mut stmt = conn.prepare(
            r##"SELECT items.id, source_id, embedding
        FROM items
        JOIN item_embeddings ie ON model_id=? AND model_version=? AND ie.item_id=items.id
        WHERE skipped IS NULL AND hidden_at IS NULL"##,
        )?;

        // (ids, blob bytes) waiting to go up, per source
        let mut pending: Vec<(Vec<i64>, Vec<u8>)> = sources.iter().map(|_| (Vec::new(), Vec::new())).collect();
        let mut rows = stmt.query([model_id, model_version])?;
        while let Some(row) = rows.next()? {
            let id: i64 = row.get(0)?;
            let source_id: i64 = row.get(1)?;
            let Some(source_idx) = sources.iter().position(|&s| s == source_id) else {
                continue;
            };
            let blob = row.get_ref(2)?.as_blob().map_err(DbError::query)?;
            if self.handle.is_null() {
                let ctx = hip::context()?;
                hip::check(unsafe {
                    ffi::pcv_searcher_create(ctx.0, (blob.len() / 4) as i32, ffi::PCV_METRIC_DOT, &mut self.handle)
                })?;
                // ids hidden (hide_items) before there was an index: the library's set starts with them
                let ids: Vec<i64> = self.hidden.iter().copied().collect();
                hip::check(unsafe { ffi::pcv_searcher_hide_ids(self.handle, ids.as_ptr(), ids.len() as i64, ptr::null_mut()) })?;
            }
            let (ids, bytes) = &mut pending[source_idx];
            ids.push(id);
            bytes.extend_from_slice(blob);
            if ids.len() >= BUILD_CHUNK_ROWS {
                self.flush(into.unwrap_or(source_id), ids, bytes)?;
            }
        }
        for (source_idx, (ids, bytes)) in pending.iter_mut().enumerate() {
            self.flush(into.unwrap_or(sources[source_idx]), ids, bytes)?;
        }
        if !self.handle.is_null() {
            hip::check(unsafe { ffi::pcv_searcher_finalize(self.handle) })?;
        }
        Ok(())
    }

    fn flush(&self, source_id: i64, ids: &mut Vec<i64>, bytes: &mut Vec<u8>) -> Result<(), HipError> {
        if ids.is_empty() {
            return Ok(());
        }
        hip::check(unsafe {
            ffi::pcv_searcher_add_blobs(self.handle, source_id, ids.as_ptr(), bytes.as_ptr(), ids.len() as i64)
        })?;
        ids.clear();
        bytes.clear();
        Ok(())
    }

    pub fn search_vector(&self, sources: &[i64], num_results: usize, vector: Vec<f32>) -> Vec<SearchItem> {
        if self.handle.is_null() || num_results == 0 {
            return Vec::new();
        }
        // the C ABI reads `dim` floats from the pointer: a vector of another width must not reach it (the reference
        // works on slices and panics inside hnsw_rs on a width mismatch; so does this)
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector: the query has {} values, the index is {}-d", vector.len(), dim);
        // num_results is not limited (search.rs:157-182; perceive-cli's --num-results is user input): beyond the
        // PCV_MAX_RESULTS (128) hits one pass over the rows ranks, the library goes over them again for the next 128.
        let k = num_results;
        let mut ids = vec![-1i64; k];
        let mut scores = vec![f32::NAN; k];
        let mut count: i32 = 0;
        // `sources.as_ptr()` of an empty slice is non-null and n_sources = 0 matches nothing, like
        // `sources.contains(..)` at search.rs:166
        hip::check(unsafe {
            ffi::pcv_searcher_search(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                k as i32,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
            )
        })
        .expect("search failed"); // the reference unwraps here too (NaN scores panic at search.rs:179)
        (0..count as usize).map(|i| SearchItem { id: ids[i], score: scores[i] }).collect()
    }

    /// Hide every row carrying one of `ids` from every later search, in place (no rebuild; the library keeps the
    /// set, remembers ids no row has yet and hides rows added later with them).  `self.hidden` follows, so the pub field
    /// keeps meaning what it meant.  `perceive hide <id>` (cmd/hide.rs:16-17) would call this where it now inserts into
    /// `searcher.hidden`, right after setting `hidden_at`:
    ///     `searcher.hide_items(&[id])?;`
    pub fn hide_items(&mut self, ids: &[i64]) -> Result<(), HipError> {
        if !self.handle.is_null() {
            let mut rows: i64 = 0;
            hip::check(unsafe { ffi::pcv_searcher_hide_ids(self.handle, ids.as_ptr(), ids.len() as i64, &mut rows) })?;
        }
        self.hidden.extend(ids.iter().copied());
        Ok(())
    }

    /// The rows carrying one of `ids` are results again, exactly as before they were hidden.
    pub fn unhide_items(&mut self, ids: &[i64]) -> Result<(), HipError> {
        if !self.handle.is_null() {
            let mut rows: i64 = 0;
            hip::check(unsafe { ffi::pcv_searcher_unhide_ids(self.handle, ids.as_ptr(), ids.len() as i64, &mut rows) })?;
        }
        for id in ids {
            self.hidden.remove(id);
        }
        Ok(())
    }

    /// Remove every row carrying one of `ids`, in every source: the rows leave the device and the rows behind them move down
    /// in place (no rebuild, no upload; searches afterwards return what an index built fresh from the remaining rows
    /// returns).  Returns the rows removed.  The reference drops items by rebuilding: `Searcher::rebuild_source`
    /// (search.rs:58-79) reads the whole source from SQLite again without the rows that are gone, and `perceive source`
    /// (cmd/source.rs, `rebuild_search`) calls it after deleting items; that call becomes
    ///     `searcher.remove_items(&deleted_ids)?;`
    /// Unlike `hide_items` the ids are not remembered: an item added later with the same id is a new item.
    pub fn remove_items(&mut self, ids: &[i64]) -> Result<usize, HipError> {
        if self.handle.is_null() || ids.is_empty() {
            return Ok(0);
        }
        let mut rows: i64 = 0;
        hip::check(unsafe { ffi::pcv_searcher_remove_ids(self.handle, ids.as_ptr(), ids.len() as i64, &mut rows) })?;
        Ok(rows as usize)
    }

    /// Upsert the embeddings a source scan produced (update_db.rs:54-60,75-126 writes them to `item_embeddings` with
    /// `ON CONFLICT ... DO UPDATE`): items the index holds take their new vector in place, in every row carrying their id
    /// (no rebuild; searches afterwards return what an index built fresh from the new rows returns); the others are added
    /// to `source_id`.  Hidden items take the new vector and stay hidden.  `perceive source scan` (cmd/source.rs:313) would
    /// call this with the `New` / `Changed` embeddings of the scan where it now calls `rebuild_search`:
    ///     `searcher.update_items(source.id, &embeddings)?;`
    pub fn update_items(&mut self, source_id: i64, items: &[(i64, Vec<f32>)]) -> Result<(), HipError> {
        if items.is_empty() {
            return Ok(());
        }
        if self.handle.is_null() {
            let ctx = hip::context()?;
            hip::check(unsafe {
                ffi::pcv_searcher_create(ctx.0, items[0].1.len() as i32, ffi::PCV_METRIC_DOT, &mut self.handle)
            })?;
            let ids: Vec<i64> = self.hidden.iter().copied().collect();
            hip::check(unsafe { ffi::pcv_searcher_hide_ids(self.handle, ids.as_ptr(), ids.len() as i64, ptr::null_mut()) })?;
        }
        let ids: Vec<i64> = items.iter().map(|(id, _)| *id).collect();
        let rows: Vec<f32> = items.iter().flat_map(|(_, v)| v.iter().copied()).collect();
        let mut found = vec![0u8; items.len()];
        let mut changed: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_update_rows(self.handle, ids.as_ptr(), rows.as_ptr(), ids.len() as i64, found.as_mut_ptr(), &mut changed)
        })?;
        let (mut new_ids, mut new_rows) = (Vec::new(), Vec::new());
        for (i, (id, v)) in items.iter().enumerate() {
            if found[i] == 0 {
                new_ids.push(*id);
                new_rows.extend_from_slice(v);
            }
        }
        if !new_ids.is_empty() {
            hip::check(unsafe {
                ffi::pcv_searcher_add_rows(self.handle, source_id, new_ids.as_ptr(), new_rows.as_ptr(), new_ids.len() as i64)
            })?;
        }
        hip::check(unsafe { ffi::pcv_searcher_finalize(self.handle) })
    }

    /// A search restricted to `items` (the items of a tag, of an author, the results of an earlier search): a read-only view
    /// that searches like an index built from only the rows carrying those ids, with the hidden items left out, and follows
    /// every later change of this searcher (no rebuild).  The app turns its filter into ids with SQL first, e.g.
    ///     `SELECT item_id FROM item_tags WHERE tag_id = ?`
    pub fn view(&self, items: &[i64]) -> Result<SearcherView<'_>, HipError> {
        let mut handle: *mut ffi::pcv_searcher = ptr::null_mut();
        if !self.handle.is_null() {
            hip::check(unsafe { ffi::pcv_searcher_create_view(self.handle, items.as_ptr(), items.len() as i64, &mut handle) })?;
        }
        Ok(SearcherView { handle, _parent: PhantomData })
    }

    /// `perceive search --like <id>` (cmd/search.rs:64-86): search with the stored embedding of `item_id`.  The reference reads
    /// the blob from SQLite (`db.read_item_embedding`), deserializes it and calls `search_vector`; here the query is built on
    /// the device from the row the index already holds, so nothing is fetched or uploaded.  As in the reference the item
    /// itself is the first hit.  `None`: no row carries the id (cmd/search.rs:83 reports "Item not found").  The CLI's branch
    /// becomes
    ///     `searcher.search_like(&sources, args.num_results, id).ok_or_else(|| eyre!("Item not found"))?`
    pub fn search_like(&self, sources: &[i64], num_results: usize, item_id: i64) -> Option<Vec<SearchItem>> {
        if self.handle.is_null() || num_results == 0 {
            return None;
        }
        let k = num_results;
        let offsets: [i64; 2] = [0, 1];
        let mut ids = vec![-1i64; k];
        let mut scores = vec![f32::NAN; k];
        let mut count: i32 = 0;
        let mut found: u8 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_like(
                self.handle,
                &item_id,
                ptr::null(),
                offsets.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                k as i32,
                0,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
                &mut found,
            )
        })
        .expect("search_like failed");
        if found == 0 {
            return None;
        }
        Some((0..count as usize).map(|i| SearchItem { id: ids[i], score: scores[i] }).collect())
    }

    /// Range search (`pcv_searcher_search_range`): every item whose reported score passes `bound` — distance <= bound for the
    /// reference's dot metric — instead of the best `num_results`: near-duplicates of an item, a "related" list with a quality
    /// cut-off.  Best first, at most `max_results`; the flag says whether more items are in range than were returned.
    pub fn search_vector_range(&self, sources: &[i64], bound: f32, max_results: usize, vector: Vec<f32>) -> (Vec<SearchItem>, bool) {
        if self.handle.is_null() || max_results == 0 {
            return (Vec::new(), false);
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector_range: the query has {} values, the index is {}-d", vector.len(), dim);
        let mut ids = vec![-1i64; max_results];
        let mut scores = vec![f32::NAN; max_results];
        let mut count: i64 = 0;
        let mut more: u8 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_range(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                &bound,
                max_results as i64,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
                &mut more,
            )
        })
        .expect("search_range failed");
        ((0..count as usize).map(|i| SearchItem { id: ids[i], score: scores[i] }).collect(), more != 0)
    }

    /// Distinct results (`pcv_searcher_search_distinct`): the ranked list of `search_vector` walked best first on the device, an
    /// item kept only if its cosine with every item kept before it is below `threshold` — the same article under five URLs is one
    /// hit.  At most `pool` entries of the list are examined (`None`: min(PCV_MAX_DISTINCT_POOL, max(128, 8 * num_results))).
    /// Each hit comes with the number of examined items dropped in its favour.
    pub fn search_vector_distinct(
        &self,
        sources: &[i64],
        num_results: usize,
        vector: Vec<f32>,
        threshold: f32,
        pool: Option<usize>,
    ) -> Vec<(SearchItem, i32)> {
        if self.handle.is_null() || num_results == 0 {
            return Vec::new();
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector_distinct: the query has {} values, the index is {}-d", vector.len(), dim);
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_DISTINCT_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut scores = vec![f32::NAN; num_results];
        let mut similar = vec![0i32; num_results];
        let mut count: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_distinct(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                threshold,
                pool as i32,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
                similar.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        })
        .expect("search_distinct failed");
        (0..count as usize).map(|i| (SearchItem { id: ids[i], score: scores[i] }, similar[i])).collect()
    }

    /// Diverse results (`pcv_searcher_search_diverse`): exact greedy maximal marginal relevance on the device over the first `pool`
    /// entries of the ranked list of `search_vector` (`None`: min(PCV_MAX_DIVERSE_POOL, max(128, 8 * num_results))).  Each pick
    /// maximises lambda * relevance - (1 - lambda) * (largest cosine with an item already picked), ties to the better rank; lambda
    /// in [0, 1], 1 = the plain list.  The picks come in pick order, each with the marginal value it was picked at and its place
    /// in the ranked list.
    pub fn search_vector_diverse(
        &self,
        sources: &[i64],
        num_results: usize,
        vector: Vec<f32>,
        lambda: f32,
        pool: Option<usize>,
    ) -> Vec<(SearchItem, f64, i32)> {
        if self.handle.is_null() || num_results == 0 {
            return Vec::new();
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector_diverse: the query has {} values, the index is {}-d", vector.len(), dim);
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_DIVERSE_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut scores = vec![f32::NAN; num_results];
        let mut marginal = vec![f64::NAN; num_results];
        let mut ranks = vec![-1i32; num_results];
        let mut count: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_diverse(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                lambda,
                pool as i32,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                marginal.as_mut_ptr(),
                ranks.as_mut_ptr(),
                &mut count,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        })
        .expect("search_diverse failed");
        (0..count as usize).map(|i| (SearchItem { id: ids[i], score: scores[i] }, marginal[i], ranks[i])).collect()
    }

    /// The group table (`pcv_searcher_set_groups`): item `ids[i]` belongs to group `groups[i]` (any i64 >= 0; `ffi::PCV_NO_GROUP`
    /// ungroups the id); of an id that occurs more than once the last occurrence holds.  The table is keyed by item id and lives on
    /// the device: it survives `remove_items` and a rebuilt source.  A chunking ingester calls this after it has added the rows.
    pub fn set_groups(&mut self, ids: &[i64], groups: &[i64]) {
        assert_eq!(ids.len(), groups.len(), "set_groups: {} ids, {} groups", ids.len(), groups.len());
        if self.handle.is_null() || ids.is_empty() {
            return;
        }
        hip::check(unsafe { ffi::pcv_searcher_set_groups(self.handle, ids.as_ptr(), groups.as_ptr(), ids.len() as i64) })
            .expect("set_groups failed");
    }

    /// Grouped results (`pcv_searcher_search_grouped`): the ranked list of `search_vector` walked best first on the device, an item
    /// kept only if no kept item has its group (`set_groups`; an item without a group is a group of its own) — the k closest
    /// documents of an index of chunks.  At most `pool` entries of the list are examined (`None`: min(PCV_MAX_GROUPED_POOL,
    /// max(128, 8 * num_results))).  Each hit comes with its group key (`ffi::PCV_NO_GROUP`: none) and the number of examined
    /// items collapsed into it.
    pub fn search_vector_grouped(
        &self,
        sources: &[i64],
        num_results: usize,
        vector: Vec<f32>,
        pool: Option<usize>,
    ) -> Vec<(SearchItem, i64, i32)> {
        if self.handle.is_null() || num_results == 0 {
            return Vec::new();
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector_grouped: the query has {} values, the index is {}-d", vector.len(), dim);
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_GROUPED_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut scores = vec![f32::NAN; num_results];
        let mut groups = vec![ffi::PCV_NO_GROUP; num_results];
        let mut collapsed = vec![0i32; num_results];
        let mut count: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_grouped(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                pool as i32,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                groups.as_mut_ptr(),
                &mut count,
                collapsed.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        })
        .expect("search_grouped failed");
        (0..count as usize).map(|i| (SearchItem { id: ids[i], score: scores[i] }, groups[i], collapsed[i])).collect()
    }

    /// The value table (`pcv_searcher_set_values`): item `ids[i]` has value `values[i]` — `Item::modified` as a Unix time stamp, say —
    /// (any i64; `ffi::PCV_NO_VALUE` unsets the id); of an id that occurs more than once the last occurrence holds.  The table is
    /// keyed by item id and lives on the device: it survives `remove_items` and a rebuilt source.
    pub fn set_values(&mut self, ids: &[i64], values: &[i64]) {
        assert_eq!(ids.len(), values.len(), "set_values: {} ids, {} values", ids.len(), values.len());
        if self.handle.is_null() || ids.is_empty() {
            return;
        }
        hip::check(unsafe { ffi::pcv_searcher_set_values(self.handle, ids.as_ptr(), values.as_ptr(), ids.len() as i64) })
            .expect("set_values failed");
    }

    /// Filtered search (`pcv_searcher_search_where`): the ranked list of `search_vector` walked best first on the device, an item
    /// kept only if its value (`set_values`) lies in `lo ..= hi` — "the best matches among the items modified since last week".
    /// `flags`: `ffi::PCV_WHERE_UNSET_PASSES`, `ffi::PCV_WHERE_OUTSIDE` or 0.  At most `pool` entries of the list are examined
    /// (`None`: min(PCV_MAX_WHERE_POOL, max(128, 8 * num_results))): for a predicate that few items pass use `view_where`.  Each
    /// hit comes with its value (`ffi::PCV_NO_VALUE`: an item without one that passed).
    pub fn search_vector_where(
        &self,
        sources: &[i64],
        num_results: usize,
        vector: Vec<f32>,
        lo: i64,
        hi: i64,
        flags: u32,
        pool: Option<usize>,
    ) -> Vec<(SearchItem, i64)> {
        if self.handle.is_null() || num_results == 0 {
            return Vec::new();
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector_where: the query has {} values, the index is {}-d", vector.len(), dim);
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_WHERE_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut scores = vec![f32::NAN; num_results];
        let mut values = vec![ffi::PCV_NO_VALUE; num_results];
        let mut count: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_where(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                pool as i32,
                lo,
                hi,
                flags,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                values.as_mut_ptr(),
                &mut count,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        })
        .expect("search_where failed");
        (0..count as usize).map(|i| (SearchItem { id: ids[i], score: scores[i] }, values[i])).collect()
    }

    /// Boosted search (`pcv_searcher_search_boosted`): the top `num_results` under relevance plus a boost that is piecewise linear in
    /// the item's value (`set_values`) through `knots` — (value, boost) pairs, values strictly increasing, at most
    /// `ffi::PCV_MAX_BOOST_KNOTS` —, constant beyond both ends and `unset_boost` for an item without a value: "the best matches, with
    /// recent items ranked a little higher".  At most `pool` entries of the ranked list are examined (`None`:
    /// min(PCV_MAX_BOOST_POOL, max(128, 8 * num_results))).  Each hit comes with its boosted score and its value
    /// (`ffi::PCV_NO_VALUE`: none); the flag says whether the hits are provably the top of the whole list.
    pub fn search_vector_boosted(
        &self,
        sources: &[i64],
        num_results: usize,
        vector: Vec<f32>,
        knots: &[(i64, f64)],
        unset_boost: f64,
        pool: Option<usize>,
    ) -> (Vec<(SearchItem, f64, i64)>, bool) {
        if self.handle.is_null() || num_results == 0 {
            return (Vec::new(), true);
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector_boosted: the query has {} values, the index is {}-d", vector.len(), dim);
        assert!(knots.len() <= ffi::PCV_MAX_BOOST_KNOTS as usize, "search_vector_boosted: {} knots", knots.len());
        let mut boost = ffi::pcv_boost::default();
        boost.n_knots = knots.len() as i32;
        for (j, (v, b)) in knots.iter().enumerate() {
            boost.knot_values[j] = *v;
            boost.knot_boosts[j] = *b;
        }
        boost.unset_boost = unset_boost;
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_BOOST_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut scores = vec![f32::NAN; num_results];
        let mut boosted = vec![f64::NAN; num_results];
        let mut values = vec![ffi::PCV_NO_VALUE; num_results];
        let mut count: i32 = 0;
        let mut exact: u8 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_boosted(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                pool as i32,
                &boost,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                boosted.as_mut_ptr(),
                values.as_mut_ptr(),
                std::ptr::null_mut(),
                &mut count,
                std::ptr::null_mut(),
                &mut exact,
            )
        })
        .expect("search_boosted failed");
        ((0..count as usize).map(|i| (SearchItem { id: ids[i], score: scores[i] }, boosted[i], values[i])).collect(), exact != 0)
    }

    /// Compound search (`pcv_searcher_search_compound`): the top `num_results` under m = base - `avoid_weight` * max(0, max_n rel_n),
    /// where base is the minimum (`any == false`: relevant to ALL of `want`) or the maximum (`any == true`: to ANY of them) of the
    /// row's relevance under the wanted vectors and rel_n its relevance under the avoided ones — a hinge: only rows that resemble an
    /// avoided vector pay.  `want` holds 1 ..= `ffi::PCV_MAX_COMPOUND_PARTS` vectors, `avoid` up to as many.  At most `pool` entries
    /// of each wanted vector's ranked list are walked (`None`: min(PCV_MAX_COMPOUND_POOL, max(128, 8 * num_results))).  Each hit is
    /// (item id, m, the score `search_vector` reports under each wanted vector, penalty); the flag says whether the hits are provably
    /// the top of all rows.
    pub fn search_compound(
        &self,
        sources: &[i64],
        num_results: usize,
        want: &[Vec<f32>],
        avoid: &[Vec<f32>],
        any: bool,
        avoid_weight: f32,
        pool: Option<usize>,
    ) -> (Vec<(i64, f64, Vec<f32>, f64)>, bool) {
        if self.handle.is_null() || num_results == 0 {
            return (Vec::new(), true);
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        for v in want.iter().chain(avoid.iter()) {
            assert_eq!(v.len(), dim as usize, "search_compound: a vector has {} values, the index is {}-d", v.len(), dim);
        }
        let parts = ffi::PCV_MAX_COMPOUND_PARTS as usize;
        let want_flat: Vec<f32> = want.iter().flatten().copied().collect();
        let avoid_flat: Vec<f32> = avoid.iter().flatten().copied().collect();
        let want_off = [0i64, want.len() as i64];
        let avoid_off = [0i64, avoid.len() as i64];
        let mode = if any { ffi::PCV_COMPOUND_ANY } else { ffi::PCV_COMPOUND_ALL };
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_COMPOUND_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut combined = vec![f64::NAN; num_results];
        let mut scores = vec![f32::NAN; num_results * parts];
        let mut penalties = vec![f64::NAN; num_results];
        let mut count: i32 = 0;
        let mut exact: u8 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_compound(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                pool as i32,
                mode,
                avoid_weight,
                want_flat.as_ptr(),
                want_off.as_ptr(),
                if avoid_flat.is_empty() { std::ptr::null() } else { avoid_flat.as_ptr() },
                avoid_off.as_ptr(),
                1,
                ids.as_mut_ptr(),
                combined.as_mut_ptr(),
                scores.as_mut_ptr(),
                penalties.as_mut_ptr(),
                &mut count,
                std::ptr::null_mut(),
                &mut exact,
            )
        })
        .expect("search_compound failed");
        let hits = (0..count as usize).map(|i| (ids[i], combined[i], scores[i * parts..i * parts + want.len()].to_vec(), penalties[i])).collect();
        (hits, exact != 0)
    }

    /// `search_compound` with every vector built on the device from stored items (`pcv_searcher_search_compound_like`): part p of
    /// `want` / `avoid` is the sum of the rows that carry its item ids.  `exclude_examples`: no row that carries a wanted example id
    /// is returned.
    pub fn search_compound_like_items(
        &self,
        sources: &[i64],
        num_results: usize,
        want: &[Vec<i64>],
        avoid: &[Vec<i64>],
        any: bool,
        avoid_weight: f32,
        pool: Option<usize>,
        exclude_examples: bool,
    ) -> Result<(Vec<(i64, f64, Vec<f32>, f64)>, bool), HipError> {
        if self.handle.is_null() || num_results == 0 {
            return Ok((Vec::new(), true));
        }
        let parts = ffi::PCV_MAX_COMPOUND_PARTS as usize;
        let csr = |groups: &[Vec<i64>]| -> (Vec<i64>, Vec<i64>) {
            let mut ids = Vec::new();
            let mut off = vec![0i64];
            for g in groups {
                ids.extend_from_slice(g);
                off.push(ids.len() as i64);
            }
            (ids, off)
        };
        let (w_ids, w_ex) = csr(want);
        let (a_ids, a_ex) = csr(avoid);
        let want_off = [0i64, want.len() as i64];
        let avoid_off = [0i64, avoid.len() as i64];
        let mode = if any { ffi::PCV_COMPOUND_ANY } else { ffi::PCV_COMPOUND_ALL };
        let pool = pool.unwrap_or_else(|| (ffi::PCV_MAX_COMPOUND_POOL as usize).min((8 * num_results).max(128)));
        let mut ids = vec![-1i64; num_results];
        let mut combined = vec![f64::NAN; num_results];
        let mut scores = vec![f32::NAN; num_results * parts];
        let mut penalties = vec![f64::NAN; num_results];
        let mut count: i32 = 0;
        let mut exact: u8 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search_compound_like(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                num_results as i32,
                pool as i32,
                mode,
                avoid_weight,
                if w_ids.is_empty() { std::ptr::null() } else { w_ids.as_ptr() },
                std::ptr::null(),
                w_ex.as_ptr(),
                want_off.as_ptr(),
                if a_ids.is_empty() { std::ptr::null() } else { a_ids.as_ptr() },
                std::ptr::null(),
                a_ex.as_ptr(),
                avoid_off.as_ptr(),
                1,
                exclude_examples as i32,
                ids.as_mut_ptr(),
                combined.as_mut_ptr(),
                scores.as_mut_ptr(),
                penalties.as_mut_ptr(),
                &mut count,
                std::ptr::null_mut(),
                &mut exact,
            )
        })?;
        let hits = (0..count as usize).map(|i| (ids[i], combined[i], scores[i * parts..i * parts + want.len()].to_vec(), penalties[i])).collect();
        Ok((hits, exact != 0))
    }

    /// A search restricted to the items whose value passes a predicate (`pcv_searcher_create_view_where`): a view like `view`
    /// without an id list — the rows are selected on the device from the value table — that also follows every later `set_values`.
    pub fn view_where(&self, lo: i64, hi: i64, flags: u32) -> Result<SearcherView<'_>, HipError> {
        let mut handle: *mut ffi::pcv_searcher = ptr::null_mut();
        if !self.handle.is_null() {
            hip::check(unsafe { ffi::pcv_searcher_create_view_where(self.handle, lo, hi, flags, &mut handle) })?;
        }
        Ok(SearcherView { handle, _parent: PhantomData })
    }

    /// Duplicate pairs (`pcv_searcher_find_duplicates`): every pair of searchable items of `sources` whose cosine is at or above
    /// `threshold`, best first, at most `max_pairs` of them (clamped to PCV_MAX_DUPLICATE_PAIRS) — the same page under several
    /// URLs, found once for the whole index.  Returns the pairs as (id of the item stored first, id of the other, cosine) and the
    /// exact number of pairs there are.
    pub fn find_duplicates(&self, sources: &[i64], threshold: f32, max_pairs: usize) -> (Vec<(i64, i64, f32)>, i64) {
        if self.handle.is_null() || max_pairs == 0 {
            return (Vec::new(), 0);
        }
        let max_pairs = max_pairs.min(ffi::PCV_MAX_DUPLICATE_PAIRS as usize);
        let mut id_a = vec![-1i64; max_pairs];
        let mut id_b = vec![-1i64; max_pairs];
        let mut scores = vec![f32::NAN; max_pairs];
        let mut count: i64 = 0;
        let mut total: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_find_duplicates(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                threshold,
                max_pairs as i64,
                id_a.as_mut_ptr(),
                id_b.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
                &mut total,
            )
        })
        .expect("find_duplicates failed");
        ((0..count as usize).map(|i| (id_a[i], id_b[i], scores[i])).collect(), total)
    }

    /// Item labels (`pcv_searcher_assign`): the exact best of the `k` vectors `labels` (`k * dim` values) for every item of
    /// `sources`, by global position.  Returns (label, score as a search reports it, item id) per item — label -1 and a NaN
    /// score for an item no search could return — and the number of items per label.
    pub fn assign(&self, sources: &[i64], labels: &[f32], k: usize) -> (Vec<(i32, f32, i64)>, Vec<i64>) {
        let (_, rows, counts, _, _) = self.assign_or_kmeans(sources, labels, k, None);
        (rows, counts)
    }

    /// Spherical k-means by cosine (`pcv_searcher_kmeans`) from the `k` vectors `init`, at most `max_iters` updates; the same
    /// input gives the same bits.  Returns the centroids of the last assignment, that assignment as in `assign`, its counts,
    /// the updates made and the items that changed their label in each assignment.
    pub fn kmeans(&self, sources: &[i64], init: &[f32], k: usize, max_iters: usize) -> (Vec<f32>, Vec<(i32, f32, i64)>, Vec<i64>, usize, Vec<i64>) {
        self.assign_or_kmeans(sources, init, k, Some(max_iters))
    }

    fn assign_or_kmeans(&self, sources: &[i64], vectors: &[f32], k: usize, max_iters: Option<usize>) -> (Vec<f32>, Vec<(i32, f32, i64)>, Vec<i64>, usize, Vec<i64>) {
        let mut counts = vec![0i64; k];
        if self.handle.is_null() || k == 0 || sources.is_empty() {
            return (vectors.to_vec(), Vec::new(), counts, 0, vec![0]);
        }
        let iters = max_iters.unwrap_or(0) as i32;
        let mut n: i64 = 0;
        let null_i32 = std::ptr::null_mut::<i32>();
        let null_f32 = std::ptr::null_mut::<f32>();
        let null_i64 = std::ptr::null_mut::<i64>();
        hip::check(unsafe {
            ffi::pcv_searcher_assign(self.handle, vectors.as_ptr(), k as i32, sources.as_ptr(), sources.len() as i32, 0, null_i32, null_f32, null_i64, null_i64, &mut n)
        })
        .expect("assign failed");
        let room = (n.max(1)) as usize;
        let mut label = vec![-1i32; room];
        let mut score = vec![f32::NAN; room];
        let mut ids = vec![-1i64; room];
        let mut centroids = vectors.to_vec();
        let mut moved = vec![0i64; iters as usize + 1];
        let mut done: i32 = 0;
        hip::check(unsafe {
            match max_iters {
                Some(_) => ffi::pcv_searcher_kmeans(
                    self.handle,
                    vectors.as_ptr(),
                    k as i32,
                    iters,
                    sources.as_ptr(),
                    sources.len() as i32,
                    room as i64,
                    centroids.as_mut_ptr(),
                    label.as_mut_ptr(),
                    score.as_mut_ptr(),
                    ids.as_mut_ptr(),
                    counts.as_mut_ptr(),
                    &mut done,
                    moved.as_mut_ptr(),
                    &mut n,
                ),
                None => ffi::pcv_searcher_assign(
                    self.handle,
                    vectors.as_ptr(),
                    k as i32,
                    sources.as_ptr(),
                    sources.len() as i32,
                    room as i64,
                    label.as_mut_ptr(),
                    score.as_mut_ptr(),
                    ids.as_mut_ptr(),
                    counts.as_mut_ptr(),
                    &mut n,
                ),
            }
        })
        .expect("assign / kmeans failed");
        moved.truncate(done as usize + 1);
        ((centroids), (0..n as usize).map(|i| (label[i], score[i], ids[i])).collect(), counts, done as usize, moved)
    }

    /// Top-m labels (`pcv_searcher_assign_top`): for every item of `sources`, by global position, the exact `m` best of the `k`
    /// vectors `labels` (clamped to PCV_MAX_TOP_LABELS) with a score of at least `min_score` (`f32::NEG_INFINITY`: no bound),
    /// best first.  Returns (item id, its labels as (label, score as a search reports it)) per item — none for an item no search
    /// could return — and the number of items that list each label.
    pub fn assign_top(&self, sources: &[i64], labels: &[f32], k: usize, m: usize, min_score: f32) -> (Vec<(i64, Vec<(i32, f32)>)>, Vec<i64>) {
        let mut label_rows = vec![0i64; k];
        if self.handle.is_null() || k == 0 || m == 0 || sources.is_empty() {
            return (Vec::new(), label_rows);
        }
        let m = m.min(ffi::PCV_MAX_TOP_LABELS as usize);
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_assign_top(
                self.handle,
                labels.as_ptr(),
                k as i32,
                m as i32,
                min_score,
                sources.as_ptr(),
                sources.len() as i32,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
            )
        })
        .expect("assign_top failed");
        let room = n.max(1) as usize;
        let mut out = vec![-1i32; room * m];
        let mut score = vec![f32::NAN; room * m];
        let mut ids = vec![-1i64; room];
        let mut counts = vec![0i32; room];
        hip::check(unsafe {
            ffi::pcv_searcher_assign_top(
                self.handle,
                labels.as_ptr(),
                k as i32,
                m as i32,
                min_score,
                sources.as_ptr(),
                sources.len() as i32,
                room as i64,
                out.as_mut_ptr(),
                score.as_mut_ptr(),
                ids.as_mut_ptr(),
                counts.as_mut_ptr(),
                label_rows.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("assign_top failed");
        let rows = (0..n as usize).map(|i| (ids[i], (0..counts[i] as usize).map(|j| (out[i * m + j], score[i * m + j])).collect())).collect();
        (rows, label_rows)
    }

    /// Item neighbours (`pcv_searcher_neighbors`): for every item of `sources`, by global position, its exact `k` best other
    /// items by cosine (clamped to PCV_MAX_NEIGHBORS), best first — the table a "related items" panel reads without a search.
    /// Returns (item id, its neighbours as (id, cosine)) per item; an item no search could return has none.
    pub fn neighbors(&self, sources: &[i64], k: usize) -> Vec<(i64, Vec<(i64, f32)>)> {
        if self.handle.is_null() || k == 0 || sources.is_empty() {
            return Vec::new();
        }
        let k = k.min(ffi::PCV_MAX_NEIGHBORS as usize);
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_neighbors(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                k as i32,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
            )
        })
        .expect("neighbors failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut nbr = vec![-1i64; room * k];
        let mut scores = vec![f32::NAN; room * k];
        let mut counts = vec![0i32; room];
        hip::check(unsafe {
            ffi::pcv_searcher_neighbors(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                k as i32,
                room as i64,
                ids.as_mut_ptr(),
                nbr.as_mut_ptr(),
                scores.as_mut_ptr(),
                counts.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("neighbors failed");
        (0..n as usize).map(|i| (ids[i], (0..counts[i] as usize).map(|j| (nbr[i * k + j], scores[i * k + j])).collect())).collect()
    }

    /// Item matches (`pcv_searcher_match`; `match` is a keyword): for every item of the sources `from`, by global position, its
    /// exact `k` best items of the sources `to` by cosine (clamped to PCV_MAX_NEIGHBORS) among those with cosine >= `min_score`
    /// (-1.0: no bound), best first.  An item is never its own match; an empty `to` matches nothing.
    /// Returns (item id, its matches as (id, cosine)) per item of `from`.
    pub fn matches(&self, from: &[i64], to: &[i64], k: usize, min_score: f32) -> Vec<(i64, Vec<(i64, f32)>)> {
        if self.handle.is_null() || k == 0 || from.is_empty() {
            return Vec::new();
        }
        let k = k.min(ffi::PCV_MAX_NEIGHBORS as usize);
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_match(
                self.handle,
                from.as_ptr(),
                from.len() as i32,
                to.as_ptr(),
                to.len() as i32,
                k as i32,
                min_score,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
            )
        })
        .expect("match failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut mids = vec![-1i64; room * k];
        let mut scores = vec![f32::NAN; room * k];
        let mut counts = vec![0i32; room];
        hip::check(unsafe {
            ffi::pcv_searcher_match(
                self.handle,
                from.as_ptr(),
                from.len() as i32,
                to.as_ptr(),
                to.len() as i32,
                k as i32,
                min_score,
                room as i64,
                ids.as_mut_ptr(),
                mids.as_mut_ptr(),
                scores.as_mut_ptr(),
                counts.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("match failed");
        (0..n as usize).map(|i| (ids[i], (0..counts[i] as usize).map(|j| (mids[i * k + j], scores[i * k + j])).collect())).collect()
    }

    /// Group-aware neighbours (`pcv_searcher_neighbors_grouped`): `neighbors` with the group table (`set_groups`) consulted.  `flags`:
    /// ffi::PCV_GROUPS_SKIP_OWN — the items of the owner's own group are no partners of it; ffi::PCV_GROUPS_ONE_PER_GROUP — of every
    /// group only its best member is kept; both, or 0 for the plain table.
    /// Returns (item id, its neighbours as (id, cosine, group or -1)) per item of `sources`.
    pub fn neighbors_grouped(&self, sources: &[i64], k: usize, flags: u32) -> Vec<(i64, Vec<(i64, f32, i64)>)> {
        if self.handle.is_null() || k == 0 || sources.is_empty() {
            return Vec::new();
        }
        let k = k.min(ffi::PCV_MAX_NEIGHBORS as usize);
        let (src, nsrc) = (sources.as_ptr(), sources.len() as i32);
        let null = std::ptr::null_mut::<i64>();
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_neighbors_grouped(self.handle, src, nsrc, k as i32, flags, 0, null, null, std::ptr::null_mut(), null, std::ptr::null_mut(), &mut n)
        })
        .expect("neighbors_grouped failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut nbr = vec![-1i64; room * k];
        let mut scores = vec![f32::NAN; room * k];
        let mut groups = vec![-1i64; room * k];
        let mut counts = vec![0i32; room];
        hip::check(unsafe {
            ffi::pcv_searcher_neighbors_grouped(
                self.handle,
                src,
                nsrc,
                k as i32,
                flags,
                room as i64,
                ids.as_mut_ptr(),
                nbr.as_mut_ptr(),
                scores.as_mut_ptr(),
                groups.as_mut_ptr(),
                counts.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("neighbors_grouped failed");
        (0..n as usize)
            .map(|i| (ids[i], (0..counts[i] as usize).map(|j| (nbr[i * k + j], scores[i * k + j], groups[i * k + j])).collect()))
            .collect()
    }

    /// Group-aware matches (`pcv_searcher_match_grouped`): `matches` with the group table consulted, as `neighbors_grouped` does.
    /// Returns (item id, its matches as (id, cosine, group or -1)) per item of `from`.
    pub fn matches_grouped(&self, from: &[i64], to: &[i64], k: usize, min_score: f32, flags: u32) -> Vec<(i64, Vec<(i64, f32, i64)>)> {
        if self.handle.is_null() || k == 0 || from.is_empty() {
            return Vec::new();
        }
        let k = k.min(ffi::PCV_MAX_NEIGHBORS as usize);
        let (src, nsrc, dst, ndst) = (from.as_ptr(), from.len() as i32, to.as_ptr(), to.len() as i32);
        let null = std::ptr::null_mut::<i64>();
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_match_grouped(
                self.handle, src, nsrc, dst, ndst, k as i32, min_score, flags, 0, null, null, std::ptr::null_mut(), null, std::ptr::null_mut(), &mut n,
            )
        })
        .expect("match_grouped failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut mids = vec![-1i64; room * k];
        let mut scores = vec![f32::NAN; room * k];
        let mut groups = vec![-1i64; room * k];
        let mut counts = vec![0i32; room];
        hip::check(unsafe {
            ffi::pcv_searcher_match_grouped(
                self.handle,
                src,
                nsrc,
                dst,
                ndst,
                k as i32,
                min_score,
                flags,
                room as i64,
                ids.as_mut_ptr(),
                mids.as_mut_ptr(),
                scores.as_mut_ptr(),
                groups.as_mut_ptr(),
                counts.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("match_grouped failed");
        (0..n as usize)
            .map(|i| (ids[i], (0..counts[i] as usize).map(|j| (mids[i * k + j], scores[i * k + j], groups[i * k + j])).collect()))
            .collect()
    }

    /// Group-aware duplicate pairs (`pcv_searcher_find_duplicates_grouped`): `find_duplicates` without the pairs of items of one group.
    /// Returns ((id_a, id_b, cosine) best first, pairs of non-siblings in all, sibling pairs at or above the threshold that were skipped).
    pub fn find_duplicates_grouped(&self, sources: &[i64], threshold: f32, max_pairs: usize) -> (Vec<(i64, i64, f32)>, i64, i64) {
        if self.handle.is_null() || sources.is_empty() || max_pairs == 0 {
            return (Vec::new(), 0, 0);
        }
        let m = max_pairs.min(ffi::PCV_MAX_DUPLICATE_PAIRS as usize);
        let mut a = vec![-1i64; m];
        let mut b = vec![-1i64; m];
        let mut scores = vec![f32::NAN; m];
        let (mut count, mut total, mut skipped) = (0i64, 0i64, 0i64);
        hip::check(unsafe {
            ffi::pcv_searcher_find_duplicates_grouped(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                threshold,
                m as i64,
                a.as_mut_ptr(),
                b.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
                &mut total,
                &mut skipped,
            )
        })
        .expect("find_duplicates_grouped failed");
        ((0..count as usize).map(|i| (a[i], b[i], scores[i])).collect(), total, skipped)
    }

    /// Counters of the last grouped pair call (`pcv_searcher_last_pair_group_stats`).
    pub fn last_pair_group_stats(&self) -> ffi::pcv_pair_group_stats {
        let mut st: ffi::pcv_pair_group_stats = unsafe { std::mem::zeroed() };
        if !self.handle.is_null() {
            hip::check(unsafe { ffi::pcv_searcher_last_pair_group_stats(self.handle, &mut st) }).expect("last_pair_group_stats failed");
        }
        st
    }

    /// Density clusters (`pcv_searcher_density_clusters`): DBSCAN under the cosine over the items of `sources`, by global
    /// position.  Two items are near iff their cosine is at least `threshold`; an item with `min_items - 1` near items or more is a
    /// core item; clusters are the connected components of the core items, numbered by their first core item.
    /// Returns ((item id, cluster or -1, kind: ffi::PCV_DENSITY_CORE / _BORDER / _NOISE / _NONE, near items) per item, clusters).
    pub fn density_clusters(&self, sources: &[i64], threshold: f32, min_items: usize) -> (Vec<(i64, i32, i8, i32)>, usize) {
        if self.handle.is_null() || sources.is_empty() {
            return (Vec::new(), 0);
        }
        let min_items = min_items.clamp(1, i32::MAX as usize) as i32;
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_density_clusters(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                threshold,
                min_items,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
                std::ptr::null_mut(),
            )
        })
        .expect("density_clusters failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut labels = vec![-1i32; room];
        let mut kinds = vec![ffi::PCV_DENSITY_NONE as i8; room];
        let mut degrees = vec![0i32; room];
        let mut clusters: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_density_clusters(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                threshold,
                min_items,
                room as i64,
                ids.as_mut_ptr(),
                labels.as_mut_ptr(),
                kinds.as_mut_ptr(),
                degrees.as_mut_ptr(),
                &mut n,
                &mut clusters,
            )
        })
        .expect("density_clusters failed");
        ((0..n as usize).map(|i| (ids[i], labels[i], kinds[i], degrees[i])).collect(), clusters as usize)
    }

    /// Linkage tree (`pcv_searcher_linkage_tree`): the single-linkage hierarchy of the items of `sources` — their maximum spanning
    /// tree under the cosine, edges ordered by (cosine descending, lower position, higher position): the merge order.
    /// Returns ((item id, takes part) per item by global position, (position a, position b, cosine) per edge, a < b).
    /// `linkage_cut` cuts it.
    pub fn linkage_tree(&self, sources: &[i64]) -> (Vec<(i64, bool)>, Vec<(i64, i64, f64)>) {
        if self.handle.is_null() || sources.is_empty() {
            return (Vec::new(), Vec::new());
        }
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_linkage_tree(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
                std::ptr::null_mut(),
            )
        })
        .expect("linkage_tree failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut part = vec![0i8; room];
        let mut pos_a = vec![-1i64; room];
        let mut pos_b = vec![-1i64; room];
        let mut c = vec![f64::NAN; room];
        let mut edges: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_linkage_tree(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                room as i64,
                ids.as_mut_ptr(),
                part.as_mut_ptr(),
                pos_a.as_mut_ptr(),
                pos_b.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                c.as_mut_ptr(),
                &mut n,
                &mut edges,
            )
        })
        .expect("linkage_tree failed");
        (
            (0..n as usize).map(|i| (ids[i], part[i] != 0)).collect(),
            (0..edges as usize).map(|i| (pos_a[i], pos_b[i], c[i])).collect(),
        )
    }

    /// Reach tree (`pcv_searcher_reach_tree`): the spanning tree of the items of `sources` under the mutual-reachability weight
    /// w = min(core(a), core(b), cosine), core = the (min_items - 1)-th largest cosine of an item with another (min_items is clamped
    /// to 1 ..= PCV_MAX_NEIGHBORS + 1), edges ordered by (w descending, lower position, higher position): what HDBSCAN starts from.
    /// Returns ((item id, takes part, core) per item by global position, (position a, position b, w) per edge, a < b).
    /// `linkage_select` picks the clusters, `linkage_cut` cuts it at a threshold.
    pub fn reach_tree(&self, sources: &[i64], min_items: usize) -> (Vec<(i64, bool, f64)>, Vec<(i64, i64, f64)>) {
        if self.handle.is_null() || sources.is_empty() {
            return (Vec::new(), Vec::new());
        }
        let min_items = min_items.clamp(1, ffi::PCV_MAX_NEIGHBORS as usize + 1) as i32;
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_reach_tree(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                min_items,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
                std::ptr::null_mut(),
            )
        })
        .expect("reach_tree failed");
        let room = n.max(1) as usize;
        let mut ids = vec![-1i64; room];
        let mut part = vec![0i8; room];
        let mut core = vec![f64::NAN; room];
        let mut pos_a = vec![-1i64; room];
        let mut pos_b = vec![-1i64; room];
        let mut w = vec![f64::NAN; room];
        let mut edges: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_reach_tree(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                min_items,
                room as i64,
                ids.as_mut_ptr(),
                part.as_mut_ptr(),
                core.as_mut_ptr(),
                pos_a.as_mut_ptr(),
                pos_b.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                w.as_mut_ptr(),
                std::ptr::null_mut(),
                &mut n,
                &mut edges,
            )
        })
        .expect("reach_tree failed");
        (
            (0..n as usize).map(|i| (ids[i], part[i] != 0, core[i])).collect(),
            (0..edges as usize).map(|i| (pos_a[i], pos_b[i], w[i])).collect(),
        )
    }

    /// Seed items (`pcv_searcher_seeds`): up to `k` items (clamped to PCV_MAX_SEEDS) that cover `sources`, in the order they were
    /// picked — `kmeanspp`: the k-means++ draw of `seed`, else farthest first; `first_id`: the item step 0 picks instead.
    /// Returns (item id, global position, potential before the pick in units of 2^-32, largest cosine with the seeds before it:
    /// NaN at step 0) per pick; fewer than `k` when no row is left uncovered.
    pub fn seeds(&self, sources: &[i64], k: usize, kmeanspp: bool, seed: u64, first_id: Option<i64>) -> Vec<(i64, i64, i64, f32)> {
        if self.handle.is_null() || k == 0 || sources.is_empty() {
            return Vec::new();
        }
        let k = k.min(ffi::PCV_MAX_SEEDS as usize);
        let mut ids = vec![-1i64; k];
        let mut positions = vec![-1i64; k];
        let mut totals = vec![0i64; k];
        let mut cover = vec![f32::NAN; k];
        let mut n: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_seeds(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                k as i32,
                if kmeanspp { ffi::PCV_SEED_KMEANSPP } else { ffi::PCV_SEED_FARTHEST },
                seed,
                first_id.as_ref().map_or(std::ptr::null(), |id| id as *const i64),
                ids.as_mut_ptr(),
                positions.as_mut_ptr(),
                totals.as_mut_ptr(),
                cover.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("seeds failed");
        (0..n as usize).map(|i| (ids[i], positions[i], totals[i], cover[i])).collect()
    }

    /// Corpus moments (`pcv_searcher_moments`): the integer sums S_d of the fixed-point unit rows of `sources`, the participating
    /// rows n, and — with `matrix` — C * 2^-64 (`centered`: (n C - S S^T) * 2^-64) as [dim][dim] f64, C = T^T T in exact integers.
    pub fn moments(&self, sources: &[i64], centered: bool, matrix: bool) -> (Vec<i64>, Vec<f64>, i64) {
        if self.handle.is_null() {
            return (Vec::new(), Vec::new(), 0);
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("dim failed");
        let dim = dim as usize;
        let mut sums = vec![0i64; dim];
        let mut mat = vec![0f64; if matrix { dim * dim } else { 0 }];
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_moments(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                centered as i32,
                sums.as_mut_ptr(),
                if matrix { mat.as_mut_ptr() } else { std::ptr::null_mut() },
                &mut n,
            )
        })
        .expect("moments failed");
        (sums, mat, n)
    }

    /// Principal axes (`pcv_searcher_principal_axes`): the `m` leading axes (clamped to PCV_MAX_AXES) of the unit rows of
    /// `sources` as ([m][dim] axes, [m] offsets: the mean along each axis, [m] variances, participating rows).
    pub fn principal_axes(&self, sources: &[i64], m: usize) -> (Vec<f32>, Vec<f64>, Vec<f64>, i64) {
        if self.handle.is_null() || m == 0 || sources.is_empty() {
            return (Vec::new(), Vec::new(), Vec::new(), 0);
        }
        let m = m.min(ffi::PCV_MAX_AXES as usize);
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("dim failed");
        let mut axes = vec![0f32; m * dim as usize];
        let mut offsets = vec![0f64; m];
        let mut variance = vec![0f64; m];
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_principal_axes(
                self.handle,
                sources.as_ptr(),
                sources.len() as i32,
                m as i32,
                axes.as_mut_ptr(),
                offsets.as_mut_ptr(),
                variance.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("principal_axes failed");
        (axes, offsets, variance, n)
    }

    /// Projection (`pcv_searcher_project`): (float)(canonical dot(axes[j], row) * rinv - offsets[j]) for every item of `sources`, by
    /// global position, as (item id, its m coordinates); NaN for an item no search could return.  `axes` is [m][dim].
    pub fn project(&self, sources: &[i64], axes: &[f32], offsets: Option<&[f64]>, m: usize) -> Vec<(i64, Vec<f32>)> {
        if self.handle.is_null() || m == 0 || sources.is_empty() {
            return Vec::new();
        }
        assert!(m <= ffi::PCV_MAX_AXES as usize && axes.len() % m == 0 && offsets.map_or(true, |o| o.len() == m));
        let off = offsets.map_or(std::ptr::null(), |o| o.as_ptr());
        let mut n: i64 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_project(
                self.handle,
                axes.as_ptr(),
                off,
                m as i32,
                sources.as_ptr(),
                sources.len() as i32,
                0,
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                &mut n,
            )
        })
        .expect("project failed");
        let room = n.max(1) as usize;
        let mut coords = vec![f32::NAN; room * m];
        let mut ids = vec![-1i64; room];
        hip::check(unsafe {
            ffi::pcv_searcher_project(
                self.handle,
                axes.as_ptr(),
                off,
                m as i32,
                sources.as_ptr(),
                sources.len() as i32,
                room as i64,
                coords.as_mut_ptr(),
                ids.as_mut_ptr(),
                &mut n,
            )
        })
        .expect("project failed");
        (0..n as usize).map(|i| (ids[i], coords[i * m..(i + 1) * m].to_vec())).collect()
    }

    pub fn search(&self, model: &Model, sources: &[i64], num_results: usize, query: &str) -> Vec<SearchItem> {
        let term_embedding = encode_query(model, query);
        self.search_vector(sources, num_results, term_embedding)
    }

    /// search.rs:195-247: the hits of `search_vector`, each with its `Item` read back from the database.
    /// Items hidden or skipped since the index was built drop out here (the SQL filters them); the result
    /// keeps the order of the hits (ascending score).
    pub fn search_vector_and_retrieve(
        &self,
        database: &Database,
        sources: &[i64],
        num_results: usize,
        vector: Vec<f32>,
    ) -> Result<Vec<(Item, SearchItem)>, DbError> {
        let hits = self.search_vector(sources, num_results, vector);
        let wanted = Rc::new(hits.iter().map(|h| rusqlite::types::Value::from(h.id)).collect::<Vec<_>>());

        let conn = database.read_pool.get()?;
        let mut stmt = conn.prepare_cached(HYDRATE_SQL)?;
        let mut by_id: ahash::HashMap<i64, Item> = ahash::HashMap::default();
        for item in stmt.query_map([wanted], item_from_row)? {
            let item = item?;
            by_id.insert(item.id, item);
        }
        // `hits` is already sorted the way the caller wants it
        Ok(hits.into_iter().filter_map(|hit| by_id.remove(&hit.id).map(|item| (item, hit))).collect())
    }

    pub fn search_and_retrieve(
        &self,
        database: &Database,
        model: &Model,
        sources: &[i64],
        num_results: usize,
        query: &str,
    ) -> Result<Vec<(Item, SearchItem)>, DbError> {
        self.search_vector_and_retrieve(database, sources, num_results, encode_query(model, query))
    }
}

/// the read query of search.rs:209-211 (the `rarray` virtual table is registered on the read pool, db.rs:79-85)
const HYDRATE_SQL: &str = "SELECT id, source_id, external_id, content, name, author, description, modified, last_accessed \
     FROM items WHERE skipped is NULL AND hidden_at IS NULL AND id IN rarray(?)";

fn unix_time(seconds: Option<i64>) -> Option<OffsetDateTime> {
    seconds.map(|t| OffsetDateTime::from_unix_timestamp(t).unwrap())
}

fn item_from_row(row: &rusqlite::Row<'_>) -> rusqlite::Result<Item> {
    let metadata = ItemMetadata {
        name: row.get(4)?,
        author: row.get(5)?,
        description: row.get(6)?,
        mtime: unix_time(row.get(7)?),
        atime: unix_time(row.get(8)?),
    };
    Ok(Item {
        id: row.get(0)?,
        source_id: row.get(1)?,
        external_id: row.get(2)?,
        content: row.get(3)?,
        raw_content: None,
        hash: None,
        skipped: None,
        process_version: 0,
        metadata,
    })
}

impl Drop for Searcher {
    fn drop(&mut self) {
        if !self.handle.is_null() {
            unsafe { ffi::pcv_searcher_destroy(self.handle) };
        }
    }
}

/// `Searcher::view`: borrows its searcher, so it is dropped (destroyed) before the searcher is.
pub struct SearcherView<'a> {
    handle: *mut ffi::pcv_searcher,
    _parent: PhantomData<&'a Searcher>,
}

unsafe impl Send for SearcherView<'_> {}
unsafe impl Sync for SearcherView<'_> {}

impl SearcherView<'_> {
    /// `Searcher::search_vector` among the view's items.
    pub fn search_vector(&self, sources: &[i64], num_results: usize, vector: Vec<f32>) -> Vec<SearchItem> {
        if self.handle.is_null() || num_results == 0 {
            return Vec::new();
        }
        let mut dim: i32 = 0;
        hip::check(unsafe { ffi::pcv_searcher_dim(self.handle, &mut dim) }).expect("searcher_dim failed");
        assert_eq!(vector.len(), dim as usize, "search_vector: the query has {} values, the index is {}-d", vector.len(), dim);
        let k = num_results;
        let mut ids = vec![-1i64; k];
        let mut scores = vec![f32::NAN; k];
        let mut count: i32 = 0;
        hip::check(unsafe {
            ffi::pcv_searcher_search(
                self.handle,
                vector.as_ptr(),
                1,
                sources.as_ptr(),
                sources.len() as i32,
                k as i32,
                ids.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
            )
        })
        .expect("search failed");
        (0..count as usize).map(|i| SearchItem { id: ids[i], score: scores[i] }).collect()
    }
}

impl Drop for SearcherView<'_> {
    fn drop(&mut self) {
        if !self.handle.is_null() {
            unsafe { ffi::pcv_searcher_destroy(self.handle) };
        }
    }
}

pub fn encode_query(model: &Model, query: &str) -> Vec<f32> {
    Vec::<Vec<f32>>::from(model.encode(&[query]).unwrap()).pop().unwrap()
}

pub fn deserialize_embedding(value: &[u8]) -> Vec<f32> {
    let mut out = vec![0f32; value.len() / 4];
    let mut n: usize = 0;
    hip::check(unsafe { ffi::pcv_deserialize_embedding(value.as_ptr(), value.len(), out.as_mut_ptr(), out.len(), &mut n) })
        .expect("embedding blob is not a whole number of f32"); // the reference panics on a short chunk
    out.truncate(n);
    out
}

pub fn serialize_embedding(embedding: &[f32]) -> Vec<u8> {
    let mut bytes_vec = vec![0u8; embedding.len() * std::mem::size_of::<f32>()];
    hip::check(unsafe {
        ffi::pcv_serialize_embedding(embedding.as_ptr(), embedding.len(), bytes_vec.as_mut_ptr(), bytes_vec.len())
    })
    .expect("serialize_embedding");
    bytes_vec
}

/// Cuts the tree of `Searcher::linkage_tree` (`pcv_linkage_cut`, host only): edge i is kept iff its cosine is at least `threshold`
/// and i < edges - (min_clusters - 1).  Returns (cluster per item, numbered by lowest position, -1: the item takes no part; clusters).
pub fn linkage_cut(items: &[(i64, bool)], edges: &[(i64, i64, f64)], threshold: f64, min_clusters: usize) -> (Vec<i32>, usize) {
    let part: Vec<i8> = items.iter().map(|x| x.1 as i8).collect();
    let pos_a: Vec<i64> = edges.iter().map(|e| e.0).collect();
    let pos_b: Vec<i64> = edges.iter().map(|e| e.1).collect();
    let c: Vec<f64> = edges.iter().map(|e| e.2).collect();
    let mut labels = vec![-1i32; items.len().max(1)];
    let mut clusters: i32 = 0;
    hip::check(unsafe {
        ffi::pcv_linkage_cut(
            pos_a.as_ptr(),
            pos_b.as_ptr(),
            c.as_ptr(),
            edges.len() as i64,
            part.as_ptr(),
            items.len() as i64,
            threshold,
            min_clusters.max(1) as i64,
            labels.as_mut_ptr(),
            &mut clusters,
        )
    })
    .expect("linkage_cut failed");
    labels.truncate(items.len());
    (labels, clusters as usize)
}

/// Picks clusters from the tree of `Searcher::reach_tree` or `linkage_tree` without a threshold (`pcv_linkage_select`, host only):
/// HDBSCAN's condensed tree with `min_cluster_size` (at least 2) and excess-of-mass selection.  `part`: takes part, per item.
/// Returns (cluster per item, numbered by lowest position, -1: noise or no part; (stability, items) per cluster).
pub fn linkage_select(part: &[bool], edges: &[(i64, i64, f64)], min_cluster_size: usize, allow_single: bool) -> (Vec<i32>, Vec<(f64, i64)>) {
    let part8: Vec<i8> = part.iter().map(|&x| x as i8).collect();
    let pos_a: Vec<i64> = edges.iter().map(|e| e.0).collect();
    let pos_b: Vec<i64> = edges.iter().map(|e| e.1).collect();
    let w: Vec<f64> = edges.iter().map(|e| e.2).collect();
    let mut labels = vec![-1i32; part.len().max(1)];
    let room = (part.len() / min_cluster_size.max(2)).max(1);
    let mut stability = vec![0f64; room];
    let mut size = vec![0i64; room];
    let mut clusters: i32 = 0;
    hip::check(unsafe {
        ffi::pcv_linkage_select(
            pos_a.as_ptr(),
            pos_b.as_ptr(),
            w.as_ptr(),
            edges.len() as i64,
            part8.as_ptr(),
            part.len() as i64,
            min_cluster_size.max(2) as i64,
            allow_single as i32,
            labels.as_mut_ptr(),
            &mut clusters,
            stability.as_mut_ptr(),
            size.as_mut_ptr(),
            room as i64,
        )
    })
    .expect("linkage_select failed");
    labels.truncate(part.len());
    (labels, (0..clusters as usize).map(|k| (stability[k], size[k])).collect())
}
