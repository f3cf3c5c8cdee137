// searcher_calls.h — the search calls behind the C entry points (searcher_calls.cpp): plain, range, distinct, grouped, diverse,
// filtered, boosted and compound search, the id-keyed tables (groups, values), the begin half of the sharded protocol and search by example.  The entry point has checked its
// arguments, holds s->mu, has seen that no pass is pending and has brought a view up to date (sync_view).
#pragma once
#include "searcher_pass.h"

namespace pcv {

void search_hits(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, int k,
                 std::vector<pcv_hit_dev>& out);
void hits_to_outputs(int metric, int D, const pcv_hit_dev* hits, int n_queries, int k, int64_t* out_ids, float* out_scores, int* out_counts);
void search_range(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, const float* bounds,
                  int64_t max_results, int64_t* out_ids, float* out_scores, int64_t* out_counts, uint8_t* out_more);
void device_begin(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, int k, pcv_hit_dev* out,
                  bool queries_on_device = false);

// What the ranked calls (distinct, grouped, diverse) have in common: the queries, the selection, num_results and pool, and the
// columns each of them writes.  `out_last`: per query, `more` (distinct, grouped) or `exact` (diverse).
struct RankedCall {
    pcv_searcher* s;
    const float* queries;
    int n_queries;
    const int64_t* source_ids;
    int n_sources;
    int k, pool;
    int64_t* out_ids;
    float* out_scores;
    int32_t* out_counts;
    int32_t* out_examined;
    uint8_t* out_last;
};
void search_distinct(const RankedCall& c, float threshold, int32_t* out_similar);
void search_diverse(const RankedCall& c, float lambda, double* out_marginal, int32_t* out_ranks);
// `owner`: whose group table is read (s itself, or the parent of a view, locked by the caller around the whole call)
void search_grouped(const RankedCall& c, const pcv_searcher* owner, int64_t* out_groups, int32_t* out_collapsed);

// The id-keyed tables of a searcher (searcher_internal.h, IdTable: s->groups, s->values); `who` names the entry point in messages.
void set_table(pcv_searcher* s, pcv_searcher::IdTable& t, const char* who, const int64_t* ids, const int64_t* vals, int64_t n);
void clear_table(pcv_searcher* s, pcv_searcher::IdTable& t);
void get_table(pcv_searcher* owner, pcv_searcher::IdTable& t, const int64_t* ids, int64_t n, int64_t* out);

// Filtered search (DESIGN.md §4 "Item values and filtered search").  `owner`: whose value table is read, as in search_grouped.
ValueTable value_table_of(const pcv_searcher* owner);
void search_where(const RankedCall& c, const pcv_searcher* owner, const WherePred& w, int64_t* out_values);
// Boosted results (DESIGN.md §4 "Boosted results").  `owner` as above; c.out_last is the `exact` column.
void search_boosted(const RankedCall& c, const pcv_searcher* owner, const pcv_boost& boost, double* out_boosted, int64_t* out_values,
                    int32_t* out_ranks);
// Compound queries (DESIGN.md §4 "Compound queries"): n compounds, compound i with wanted vectors want[want_off[i] .. want_off[i + 1])
// and avoided vectors avoid[avoid_off[i] .. avoid_off[i + 1]) (avoid_off nullptr: none), [.][D] each; the entry point has checked
// the offsets, the values and the norms.  Outputs as pcv_searcher_search_compound declares them, all nullable.
struct CompoundCall {
    pcv_searcher* s;
    const int64_t* source_ids;
    int n_sources;
    int k, pool, mode;
    double lambda;
    const float* want;
    const int64_t* want_off;
    const float* avoid;
    const int64_t* avoid_off;
    int n;
    int64_t* out_ids;
    double* out_combined;
    float* out_part_scores;
    double* out_penalties;
    int32_t* out_counts;
    int32_t* out_examined;
    uint8_t* out_exact;
};
void search_compound(const CompoundCall& c);
// canonical |q|^2: f64, feature order (what the ranking pass and the compound select step divide by)
double query_norm2(const float* q, int D);
// rows of the selected sources of `s` that pass / those of them a search could return (s->mu and owner's lock held)
void count_where(pcv_searcher* s, const pcv_searcher* owner, const int64_t* source_ids, int n_sources, const WherePred& w,
                 int64_t* out_rows, int64_t* out_searchable);

int64_t check_like_args(const pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets, int n_queries,
                        const char* who);
std::unique_lock<std::mutex> lock_like_owner(pcv_searcher* s, pcv_searcher*& owner, const char* who);
// What the lookup of a call's examples gives back to the host.
struct LikeBuilt {
    std::vector<float> vectors;         // [n_queries][D], if asked for
    std::vector<int64_t> member_rows;   // [n_queries] rows that went into each query
    std::vector<int64_t> carrier_rows;  // [n_queries] ... plus the rows staged under PCV_STAGING_SOURCE that carry one of its ids
    std::vector<uint8_t> found;         // [examples]
};
void build_like_queries(pcv_searcher* p, const int64_t* example_ids, const float* weights, const int64_t* offsets, int n_queries,
                        bool want_host, void* d_out, LikeBuilt& out);

}  // namespace pcv
