// searcher_calls.cpp — the search calls: what each does with the passes of searcher_pass.cpp.  Called by the C entry points
// (searcher.cpp, searcher_exchange.cpp) under the conditions searcher_calls.h states.
#include <cfloat>
#include <cstring>
#include <numeric>

#include "searcher_calls.h"

namespace pcv {

// Full search: any number of queries / segments; result [n_queries][k] hits on the host.
void search_hits(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources,
                 int k, std::vector<pcv_hit_dev>& out) {
    check_search_args(s, queries, n_queries, k, "search", 1 << 24);
    const pcv_hit_dev none{NAN, -1, -1};
    out.assign((size_t)n_queries * k, none);
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    if (!open_search(s, plan)) return;
    const int qstep = plan.qstep;
    std::vector<CeilRec> ceil;
    std::vector<pcv_hit_dev> last;
    for (int q0 = 0; q0 < n_queries; q0 += qstep) {
        const int B = std::min(qstep, n_queries - q0);
        const float* qs = queries + (size_t)q0 * s->D;
        // One pass ranks up to kMaxK results.  More (search.rs:157-182 has no limit): the next kMaxK below the last hit of the
        // pass before, and so on — each pass exact among the rows that rank after its ceiling (the statistics add up over the passes).
        for (int got = 0; got < k; got += kMaxK) {
            const int kk = std::min(kMaxK, k - got);
            if (got > 0) {
                ceil.resize((size_t)B);
                next_ceilings(s, qs, B, last.data(), ceil.data());
            }
            run_pass(s, PassRequest(qs, B, plan.segs, plan.kernel).top_k(kk, nullptr, true, nullptr, got > 0 ? ceil.data() : nullptr));
            last.resize((size_t)B);
            bool more = false;
            for (int q = 0; q < B; ++q) {  // (the hits came down with the pass)
                std::memcpy(out.data() + (size_t)(q0 + q) * k + got, s->pin->hits + (size_t)q * kk, (size_t)kk * sizeof(pcv_hit_dev));
                last[(size_t)q] = s->pin->hits[(size_t)q * kk + kk - 1];  // pos < 0: fewer than kk rows counted — nothing is left
                more = more || last[(size_t)q].pos >= 0;
            }
            if (!more) break;
        }
    }
}

// hits -> the reference's result convention
void hits_to_outputs(int metric, int D, const pcv_hit_dev* hits, int n_queries, int k, int64_t* out_ids,
                     float* out_scores, int* out_counts) {
    for (int q = 0; q < n_queries; ++q) {
        int cnt = 0;
        for (int j = 0; j < k; ++j) {
            const pcv_hit_dev& h = hits[(size_t)q * k + j];
            const bool ok = h.pos >= 0;
            if (ok) ++cnt;
            if (out_ids) out_ids[(size_t)q * k + j] = ok ? h.id : -1;
            if (out_scores) {
                out_scores[(size_t)q * k + j] = ok ? reported_score(metric, D, h.score) : NAN;
            }
        }
        if (out_counts) out_counts[q] = cnt;
    }
}

// ---- range search (pcv_searcher_search_range; DESIGN.md §4 "Range search") ----
// The threshold of a range pass for one query: the canonical value of the bound, rounded towards "keeps more" — no row whose
// REPORTED score passes the bound has c < tau (scan.h, RangeRec).
//   cosine: (float)c >= b implies c > the f32 below b;
//   dot:    (float)max(0, 1 - c/D) <= b implies 1 - c/D < the f32 above b, i.e. c > D (1 - that), less the roundings of the f64
//           expression (1e-9 relative is generous); a negative bound admits nothing.
// Capped at a value no score reaches (cosine: 4; dot: 2 |q| max|x|), so that "nothing" is a finite threshold like any other.
static RangeRec range_rec(const pcv_searcher* s, const float* q, float bound) {
    RangeRec r{bound, -INFINITY};
    float most = 4.0f;
    if (s->metric == PCV_METRIC_DOT) {
        const double m = 2.0 * query_norm(q, s->D) * (double)s->max_norm + 1e-30;
        most = (m < (double)FLT_MAX) ? std::nextafterf((float)m, INFINITY) : FLT_MAX;  // (NaN: FLT_MAX)
        if (bound < 0.0f) {
            r.tau = most;
        } else if (bound < INFINITY) {
            const double T = (double)s->D * (1.0 - (double)std::nextafterf(bound, INFINITY));
            const double Tl = T - std::fabs(T) * 1e-9;
            r.tau = Tl > -(double)FLT_MAX ? std::nextafterf((float)Tl, -INFINITY) : -INFINITY;
        }
    } else if (bound > -INFINITY) {
        r.tau = std::nextafterf(bound, -INFINITY);
    }
    if (r.tau > most) r.tau = most;
    return r;
}

// What a range call leaves allocated for the next one.  Its lists and result blocks are sized from the data: up to kRangeBudget
// list entries per pass (0.4 GB of device lists) and, with max_results >= kRangeRun, as many pcv_hit_dev of pinned host memory
// (0.8 GB).  A searcher that once answered a wide bound does not hold that for good: whatever exceeds kRangeKeptBytes is given
// back when the call ends, and the lists start from cand_cap again (at the price of one repeated pass for the next wide bound).
constexpr size_t kRangeKeptBytes = (size_t)64 << 20;
static void trim_range_memory(pcv_searcher* s) {
    const bool pinned = s->pin_range.n * sizeof(pcv_hit_dev) > kRangeKeptBytes;
    const bool lists = s->d_cand.n * sizeof(*s->d_cand.p) > kRangeKeptBytes && s->d_cand.n > (size_t)kMfmaQueries * s->cand_cap;
    if (!pinned && !lists) return;
    (void)hipStreamSynchronize(s->ctx->stream);  // (a call that failed may have left its pass in flight)
    if (pinned) s->pin_range.release();
    if (lists) {  // (every pass sizes them again: ensure_workspace, fill_range_part)
        s->d_cand.release();
        s->d_cand_s.release();
        s->range_cap = 0;
    }
}

// Every searchable row of the selected sources whose reported score passes the query's bound, in the canonical order, at most
// max_results per query.  One pass per group of queries (a second one if a list was too short: the thresholds are fixed, so the
// uncapped counts of the first are exactly what the second needs); range_select_kernel leaves each list as sorted runs of
// kRangeRun in pinned memory, merged here.
void search_range(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, const float* bounds,
                  int64_t max_results, int64_t* out_ids, float* out_scores, int64_t* out_counts, uint8_t* out_more) {
    PCV_REQUIRE(!s->dirty, "search_range: rows were added or cleared without pcv_searcher_finalize");
    if (queries != nullptr && n_queries > 0) check_dot_envelope(s, queries, n_queries, "search_range");
    s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries);
    for (int q = 0; q < n_queries; ++q) {
        if (out_counts) out_counts[q] = 0;
        if (out_more) out_more[q] = 0;
    }
    auto blank = [&](int q, int64_t from) {
        for (int64_t j = from; j < max_results; ++j) {
            if (out_ids) out_ids[(size_t)q * max_results + j] = -1;
            if (out_scores) out_scores[(size_t)q * max_results + j] = NAN;
        }
    };
    if (!open_search(s, plan)) {
        for (int q = 0; q < n_queries; ++q) blank(q, 0);
        return;
    }
    struct Trim {
        pcv_searcher* s;
        ~Trim() { trim_range_memory(s); }
    } trim{s};
    std::vector<RangeRec> recs((size_t)n_queries);
    for (int q = 0; q < n_queries; ++q) recs[(size_t)q] = range_rec(s, queries + (size_t)q * s->D, bounds[q]);
    // the lists of one pass hold at most kRangeBudget entries (12 bytes each): long lists take fewer queries per pass
    constexpr uint64_t kRangeBudget = (uint64_t)1 << 25;
    const uint32_t keep = (uint32_t)std::min<int64_t>(kRangeRun, max_results);
    uint32_t cap = std::max(s->range_cap, s->cand_cap);
    const int qmost = plan.qstep;
    struct Head {
        const pcv_hit_dev* at;
        const pcv_hit_dev* end;
    };
    std::vector<Head> heads;
    for (int q0 = 0; q0 < n_queries;) {
        int B = (int)std::min<uint64_t>((uint64_t)std::min(qmost, n_queries - q0), std::max<uint64_t>(1, kRangeBudget / cap));
        const float* qs = queries + (size_t)q0 * s->D;
        PassRequest pass = PassRequest(qs, B, plan.segs, plan.kernel).in_range(recs.data() + q0, cap, keep);
        enqueue_pass(s, pass);
        if (finish_pass(s)) {
            uint32_t mx = 0;
            int worst = 0;
            for (int q = 0; q < B; ++q)
                if (s->pin->cnt[q] > mx) mx = s->pin->cnt[q], worst = q0 + q;
            if (mx > (uint32_t)PCV_MAX_RANGE_ROWS)
                PCV_FAIL(PCV_ERR_UNSUPPORTED,
                         "search_range: the pass of query %d lists %u rows, more than PCV_MAX_RANGE_ROWS (%d): use pcv_searcher_search for "
                         "such a bound",
                         worst, mx, (int)PCV_MAX_RANGE_ROWS);
            // what the pass needed plus a quarter, at least twice what they were
            const uint64_t want = std::max<uint64_t>(list_need(mx), (uint64_t)cap * 2);
            cap = (uint32_t)std::max<uint64_t>(mx, std::min<uint64_t>(want, (uint64_t)PCV_MAX_RANGE_ROWS));
            s->range_cap = cap;
            B = (int)std::min<uint64_t>((uint64_t)B, std::max<uint64_t>(1, kRangeBudget / cap));
            pass.B = B;
            pass.range.cap = cap;
            enqueue_pass(s, pass);
            PCV_REQUIRE(!finish_pass(s), "search_range: lists sized from the counts of a pass overflowed in its repeat");
        }
        const uint32_t runs = (cap + kRangeRun - 1) / kRangeRun;
        for (int q = 0; q < B; ++q) {
            const uint32_t listed = std::min(s->pin->cnt[q], cap);
            const uint32_t used = (listed + kRangeRun - 1) / kRangeRun;
            int64_t total = 0;
            heads.clear();
            for (uint32_t r = 0; r < used; ++r) {
                const uint32_t n = s->pin_range_cnt.p[(size_t)q * runs + r];
                total += n;
                const pcv_hit_dev* at = s->pin_range.p + ((size_t)q * runs + r) * keep;
                if (n > 0) heads.push_back({at, at + std::min(n, keep)});
            }
            const int64_t cnt = std::min(total, max_results);
            const size_t o = (size_t)(q0 + q) * (size_t)max_results;
            auto after = [](const Head& a, const Head& b) { return hit_better(*b.at, *a.at); };  // (heap: the best run on top)
            std::make_heap(heads.begin(), heads.end(), after);
            for (int64_t j = 0; j < cnt; ++j) {
                std::pop_heap(heads.begin(), heads.end(), after);
                Head& h = heads.back();
                if (out_ids) out_ids[o + j] = h.at->id;
                if (out_scores) out_scores[o + j] = reported_score(s->metric, s->D, h.at->score);
                if (++h.at == h.end)
                    heads.pop_back();
                else
                    std::push_heap(heads.begin(), heads.end(), after);
            }
            blank(q0 + q, cnt);
            if (out_counts) out_counts[q0 + q] = cnt;
            if (out_more) out_more[q0 + q] = total > max_results ? 1 : 0;
        }
        q0 += B;
    }
}

// ---- the ranked calls: distinct, grouped and diverse results (RankedCall, searcher_calls.h) ----
namespace {

// One query's answer: its n kept rows — hit(i) and the call's own columns, extra(at, &i), i the row's place in the state block
// of its group (`slot`: the query's) — with blanks behind them (extra(at, nullptr)), the counters and the call's last column.
template <class Hit, class Extra>
void write_ranked(const RankedCall& c, int q, int slot, int n, int32_t examined, uint8_t last, Hit hit, Extra extra) {
    for (int j = 0; j < c.k; ++j) {
        const size_t at = (size_t)q * c.k + j, i = (size_t)slot * kMaxK + j;
        const bool kept = j < n;
        const pcv_hit_dev h = kept ? hit(i) : pcv_hit_dev{NAN, -1, -1};
        if (c.out_ids) c.out_ids[at] = h.id;
        if (c.out_scores) c.out_scores[at] = kept ? reported_score(c.s->metric, c.s->D, h.score) : NAN;
        extra(at, kept ? &i : nullptr);
    }
    if (c.out_counts) c.out_counts[q] = n;
    if (c.out_examined) c.out_examined[q] = examined;
    if (c.out_last) c.out_last[q] = last;
}

// What a ranked call settles before its first pass, in this order: the argument check, fresh statistics, the plan, open_search.
// False: no selected rows, and the empty answer is written — every list blank, nothing kept or examined, `last` in the last column.
template <class Extra>
bool open_ranked(const RankedCall& c, const char* who, SearchPlan& plan, uint8_t last, Extra extra) {
    check_search_args(c.s, c.queries, c.n_queries, c.k, who);
    c.s->stats = pcv_scan_stats{};  // (also when the kernel is refused)
    c.s->select_ms = 0.0f;
    c.s->select_launches = 0;
    plan = plan_search(c.s, c.source_ids, c.n_sources, c.n_queries);
    if (open_search(c.s, plan)) return true;
    for (int q = 0; q < c.n_queries; ++q) write_ranked(c, q, 0, 0, 0, last, [](size_t) { return pcv_hit_dev{}; }, extra);
    return false;
}

// The call's queries in groups of up to `group`: f(q0, B, the group's queries).
template <class F>
void each_query_group(const RankedCall& c, int group, F f) {
    for (int q0 = 0; q0 < c.n_queries; q0 += group) f(q0, std::min(group, c.n_queries - q0), c.queries + (size_t)q0 * c.s->D);
}

// The walk of one group of B queries, shared by the ranked calls: passes of kMaxK hits until every query is finished or `pool`
// entries are walked, `select` (the call's select step, queued on the stream after each pass) keeping the records `rec` (pinned;
// `d_rec` on the device) up to date.  -> per query, whether its walk stopped at `pool` unfinished with more of its list to come
// (decided only if `want_more`).
template <class Select>
std::vector<uint8_t> walk_ranked_lists(pcv_searcher* s, const SearchPlan& plan, const float* qs, int B, int pool, DistinctRec* rec,
                                       DistinctRec* d_rec, bool want_more, Select select) {
    hipStream_t st = s->ctx->stream;
    std::vector<CeilRec> ceil((size_t)B);
    std::vector<pcv_hit_dev> last((size_t)B);
    // (the walk's own pair of events around every select step: pcv_searcher_last_select_stats)
    hipEvent_t ev[2] = {nullptr, nullptr};
    const auto drop_events = at_exit([&] {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    });
    for (hipEvent_t& e : ev) PCV_HIP(hipEventCreate(&e));
    // the ceilings behind the last hit each query has walked (a finished query: nothing ranks after it)
    auto ceilings = [&] {
        for (int q = 0; q < B; ++q) last[(size_t)q] = rec[q].flags ? pcv_hit_dev{NAN, -1, -1} : pcv_hit_dev{rec[q].last_score, rec[q].last_pos, -1};
        next_ceilings(s, qs, B, last.data(), ceil.data());
        return ceil.data();
    };
    for (int q = 0; q < B; ++q) rec[q] = DistinctRec{0, 0, 0, 0, INFINITY, -1};
    PCV_HIP(hipMemcpyAsync(d_rec, rec, (size_t)B * sizeof(DistinctRec), hipMemcpyHostToDevice, st));
    // A query still walking after a pass has walked every hit of every pass so far: `walked` is the same for all of them.
    bool pending = true;
    for (int walked = 0; pending && walked < pool; walked += kMaxK) {
        const int kk = std::min(kMaxK, pool - walked);
        run_pass(s, PassRequest(qs, B, plan.segs, plan.kernel).top_k(kk, nullptr, false, nullptr, walked > 0 ? ceilings() : nullptr));
        // (the pass block is the pass's to allocate and to grow: its device address is read after the pass, never before)
        PCV_HIP(hipEventRecord(ev[0], st));
        select();
        PCV_HIP(hipEventRecord(ev[1], st));
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        s->select_ms += ms;
        s->select_launches += 1;
        pending = false;
        for (int q = 0; q < B; ++q) pending = pending || rec[q].flags == 0;
    }
    // out_more: a walk that stopped at `pool` without its num_results and without seeing its list end.  Whether the list had
    // another row is one more, short pass under the same kind of ceiling: one hit per query.
    std::vector<uint8_t> more((size_t)B, 0);
    if (pending && want_more) {
        run_pass(s, PassRequest(qs, B, plan.segs, plan.kernel).top_k(1, nullptr, true, nullptr, ceilings()));
        for (int q = 0; q < B; ++q) more[(size_t)q] = (rec[q].flags == 0 && s->pin->hits[q].pos >= 0) ? 1 : 0;
    }
    return more;
}

// The state block of one group of up to kMfmaQueries queries of search_distinct and search_grouped (scan.h, DistinctArgs,
// GroupedArgs), the same layout on both sides ...
struct DistinctLayout {
    static constexpr size_t Q = kMfmaQueries;
    static constexpr size_t off_rec = 0;
    static constexpr size_t off_kept = off_rec + Q * sizeof(DistinctRec);
    static constexpr size_t off_sim = off_kept + Q * kMaxK * sizeof(pcv_hit_dev);
    static constexpr size_t off_norm = off_sim + Q * kMaxK * sizeof(int32_t);
    static constexpr size_t total = off_norm + Q * kMaxK * sizeof(double);
};
static_assert(sizeof(int64_t) == sizeof(double), "the group keys take the place of the norms");
// ... and the blocks of both sides as typed pointers (the searcher's own, made or grown here).
struct DistinctView {
    DistinctRec* rec;
    pcv_hit_dev* kept;  // [Q][kMaxK]
    int32_t* count;     // [Q][kMaxK] per kept row: the rows dropped in its favour (similar / collapsed)
    double* norm;       // [Q][kMaxK] distinct: the kept rows' norms (the device's alone: never downloaded) ...
    int64_t* group;     // ... grouped: their group keys, in the same place
};
struct DistinctViews {
    DistinctView dev{}, pin{};
};
DistinctViews distinct_views(pcv_searcher* s) {
    using L = DistinctLayout;
    s->d_distinct.ensure(L::total);
    s->pin_distinct.ensure(L::total);
    auto view = [](uint8_t* p) {
        return DistinctView{reinterpret_cast<DistinctRec*>(p + L::off_rec), reinterpret_cast<pcv_hit_dev*>(p + L::off_kept),
                            reinterpret_cast<int32_t*>(p + L::off_sim), reinterpret_cast<double*>(p + L::off_norm),
                            reinterpret_cast<int64_t*>(p + L::off_norm)};
    };
    return {view(s->d_distinct.p), view(s->pin_distinct.p)};
}

// What search_distinct and search_grouped do with the call's queries, qstep at a time: the walk, `select` after each of its
// passes; then the kept rows and what lies behind them in the block, up to `down_end`, come down once and the answers are written.
template <class Select, class Extra>
void collapse_ranked(const RankedCall& c, const SearchPlan& plan, const DistinctViews& v, size_t down_end, Select select, Extra extra) {
    using L = DistinctLayout;
    pcv_searcher* s = c.s;
    hipStream_t st = s->ctx->stream;
    const DistinctView& pin = v.pin;
    each_query_group(c, plan.qstep, [&](int q0, int B, const float* qs) {
        const std::vector<uint8_t> more = walk_ranked_lists(s, plan, qs, B, c.pool, pin.rec, v.dev.rec, c.out_last != nullptr, select);
        PCV_HIP(hipMemcpyAsync(s->pin_distinct.p + L::off_kept, s->d_distinct.p + L::off_kept, down_end - L::off_kept, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < B; ++q)
            write_ranked(c, q0 + q, q, (int)pin.rec[q].kept, (int32_t)pin.rec[q].examined, more[(size_t)q], [&](size_t i) { return pin.kept[i]; }, extra);
    });
}

}  // namespace

// ---- distinct results (pcv_searcher_search_distinct; DESIGN.md §4 "Distinct results") ----
// The ranked list of every query is walked kMaxK hits a pass: the first pass is a plain top-k pass, every later one ranks the rows
// behind the last hit walked (its ceiling, as in search_hits), and after each the select step (distinct_kernels.hip) walks the
// pass's lists on the device against the rows kept so far.  What comes back after a pass is one record per query — kept, examined,
// finished or not, the last hit walked —; the kept rows and their counters come down once, at the end.  A query that is finished
// (num_results kept, or its list at an end) gets the ceiling "nothing ranks after it" and the select step leaves it alone.
void search_distinct(const RankedCall& c, float threshold, int32_t* out_similar) {
    pcv_searcher* s = c.s;
    DistinctViews v;  // (set once the call has rows to search: the blanks of the empty answer read neither side)
    auto extra = [&](size_t at, const size_t* i) {
        if (out_similar) out_similar[at] = i ? v.pin.count[*i] : 0;
    };
    SearchPlan plan;
    if (!open_ranked(c, "search_distinct", plan, 0, extra)) return;
    v = distinct_views(s);
    DistinctArgs args{};
    args.rec = v.dev.rec;
    args.rec_host = v.pin.rec;
    args.kept = v.dev.kept;
    args.similar = v.dev.count;
    args.kept_norm = v.dev.norm;
    args.num_results = c.k;
    args.threshold = (double)threshold;
    collapse_ranked(c, plan, v, DistinctLayout::off_norm, [&] {
        launch_distinct_select(s->ctx->stream, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
    }, extra);
}

// ---- diverse results (pcv_searcher_search_diverse; DESIGN.md §4 "Diverse results") ----
// The state block of one group of up to kMfmaQueries queries: the walk's records and the result block, the same layout on both
// sides.  (The pool lists and the row scratch are sized by the call and live beside it: scan.h, DiverseArgs.)
namespace {
struct DiverseLayout {
    static constexpr size_t Q = kMfmaQueries;
    static constexpr size_t off_rec = 0;
    static constexpr size_t off_id = off_rec + Q * sizeof(DistinctRec);
    static constexpr size_t off_score = off_id + Q * kMaxK * sizeof(int64_t);
    static constexpr size_t off_marginal = off_score + Q * kMaxK * sizeof(double);
    static constexpr size_t off_rank = off_marginal + Q * kMaxK * sizeof(double);
    static constexpr size_t off_exact = off_rank + Q * kMaxK * sizeof(int32_t);
    static constexpr size_t total = off_exact + Q * sizeof(uint32_t);
};
// The rows of a group's pools are gathered into one compact scratch of at most kDiverseScratchBytes: a group is as many queries
// as fit (64 at 384-d and the largest pool), one at least.  What exceeds kDiverseKeptBytes is given back when the call ends.
constexpr size_t kDiverseScratchBytes = (size_t)512 << 20;
constexpr size_t kDiverseKeptBytes = (size_t)64 << 20;
}  // namespace

// The first `pool` entries of every query's ranked list are collected kMaxK hits a pass (walk_ranked_lists: nothing stops a query
// early but the end of its list), diverse_collect_kernel appending each pass's hits and their rows to the query's pool; then one
// launch of diverse_select_kernel makes the greedy walk of the whole group.  What comes back is one record per query after each
// pass and the result block once.
void search_diverse(const RankedCall& c, float lambda, double* out_marginal, int32_t* out_ranks) {
    using L = DiverseLayout;
    pcv_searcher* s = c.s;
    const double* r_marginal = nullptr;  // (of the pinned result block, once the call has rows to search)
    const int32_t* r_rank = nullptr;
    auto extra = [&](size_t at, const size_t* i) {
        if (out_marginal) out_marginal[at] = i ? r_marginal[*i] : NAN;
        if (out_ranks) out_ranks[at] = i ? r_rank[*i] : -1;
    };
    SearchPlan plan;
    if (!open_ranked(c, "search_diverse", plan, 1, extra)) return;  // (exact: the list ended inside the pool)
    hipStream_t st = s->ctx->stream;
    const size_t cap = ((size_t)c.pool + 63) / 64 * 64;
    const size_t row_bytes = cap * (size_t)s->D4 * sizeof(float4);  // of one query's pool
    const int group = (int)std::min<size_t>((size_t)std::min(plan.qstep, c.n_queries), std::max<size_t>(1, kDiverseScratchBytes / row_bytes));
    const auto trim = at_exit([&] {
        if (s->d_diverse_rows.n * sizeof(float4) <= kDiverseKeptBytes) return;
        (void)hipStreamSynchronize(st);  // (a call that failed may have left its kernels in flight)
        s->d_diverse_rows.release();
    });
    s->d_diverse.ensure(L::total);
    s->pin_diverse.ensure(L::total);
    s->d_diverse_entries.ensure((size_t)group * cap);
    s->d_diverse_rows.ensure((size_t)group * cap * (size_t)s->D4);
    DistinctRec* rec = reinterpret_cast<DistinctRec*>(s->pin_diverse.p + L::off_rec);
    DiverseArgs args{};
    args.rec = reinterpret_cast<DistinctRec*>(s->d_diverse.p + L::off_rec);
    args.rec_host = rec;
    args.entries = s->d_diverse_entries.p;
    args.rows = s->d_diverse_rows.p;
    args.out_id = reinterpret_cast<int64_t*>(s->d_diverse.p + L::off_id);
    args.out_score = reinterpret_cast<double*>(s->d_diverse.p + L::off_score);
    args.out_marginal = reinterpret_cast<double*>(s->d_diverse.p + L::off_marginal);
    args.out_rank = reinterpret_cast<int32_t*>(s->d_diverse.p + L::off_rank);
    args.out_exact = reinterpret_cast<uint32_t*>(s->d_diverse.p + L::off_exact);
    args.cap = (int)cap;
    args.pool = c.pool;
    args.num_results = c.k;
    args.lambda = (double)lambda;
    const int64_t* r_id = reinterpret_cast<const int64_t*>(s->pin_diverse.p + L::off_id);
    const double* r_score = reinterpret_cast<const double*>(s->pin_diverse.p + L::off_score);
    r_marginal = reinterpret_cast<const double*>(s->pin_diverse.p + L::off_marginal);
    r_rank = reinterpret_cast<const int32_t*>(s->pin_diverse.p + L::off_rank);
    const uint32_t* r_exact = reinterpret_cast<const uint32_t*>(s->pin_diverse.p + L::off_exact);
    each_query_group(c, group, [&](int q0, int B, const float* qs) {
        args.walked = 0;
        walk_ranked_lists(s, plan, qs, B, c.pool, rec, args.rec, false, [&] {
            launch_diverse_collect(st, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
            args.walked += kMaxK;
        });
        launch_diverse_select(st, B, s->D, s->D4, s->metric, args);
        PCV_HIP(hipMemcpyAsync(s->pin_diverse.p + L::off_id, s->d_diverse.p + L::off_id, L::total - L::off_id, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
        for (int q = 0; q < B; ++q)
            write_ranked(c, q0 + q, q, (int)rec[q].kept, (int32_t)rec[q].examined, r_exact[q] ? 1 : 0,
                         [&](size_t i) { return pcv_hit_dev{r_score[i], -1, r_id[i]}; }, extra);
    });
}

// ---- the id-keyed tables (pcv_searcher_set_groups / _set_values; DESIGN.md §4 "Grouped results", "Item values and filtered search") ----
constexpr int64_t kMaxGroupEntries = (int64_t)1 << 30;
constexpr uint64_t kMinGroupSlots = 1024;
constexpr size_t kGroupKeptBytes = (size_t)64 << 20;  // scratch of a set / get call beyond this is given back

// Table `t` of `s` gets `slots` slots (a power of two, more than it has): the entries move by a rehash on the device.  If the
// allocation fails the old table stays as it is.
static void grow_table(pcv_searcher* s, pcv_searcher::IdTable& t, const char* who, uint64_t slots) {
    hipStream_t st = s->ctx->stream;
    int64_t *keys = nullptr, *vals = nullptr;
    const hipError_t e = alloc_with_scales(s->fail_copy_alloc, &keys, slots * sizeof(int64_t), &vals, slots * sizeof(int64_t));
    if (e != hipSuccess)
        PCV_FAIL(PCV_ERR_DEVICE, "%s: hipMalloc of %.2f GB for a %s table of %llu slots failed: %s (the table is unchanged)", who,
                 slots * 16 / 1e9, t.what, (unsigned long long)slots, hipGetErrorString(e));
    try {
        launch_group_fill(st, keys, vals, slots, t.none);
        launch_group_rehash(st, t.keys, t.vals, t.slots, keys, vals, (uint32_t)(slots - 1));
        PCV_HIP(hipStreamSynchronize(st));
    } catch (...) {
        (void)hipFree(keys);
        (void)hipFree(vals);
        throw;
    }
    if (t.keys) (void)hipFree(t.keys);
    if (t.vals) (void)hipFree(t.vals);
    if (t.slots > 0) t.rehashes += 1;
    t.keys = keys;
    t.vals = vals;
    t.slots = slots;
}

static void trim_table_scratch(pcv_searcher::IdTable& t) {
    if (t.d_claim.n * sizeof(uint32_t) > kGroupKeptBytes) t.d_claim.release();
    if (t.d_slot.n * sizeof(uint32_t) > kGroupKeptBytes) t.d_slot.release();
    if (t.d_batch.n * sizeof(int64_t) > kGroupKeptBytes) t.d_batch.release();
}

// The upsert of a batch into table `t` of `s` (s->mu held, s no view, the arguments checked): one growth decision, then the batch
// kGroupBatch ids at a time, in order — a later occurrence of an id overrides an earlier one inside a launch (launch_group_upsert)
// and across launches.
void set_table(pcv_searcher* s, pcv_searcher::IdTable& t, const char* who, const int64_t* ids, const int64_t* vals, int64_t n) {
    if (n == 0) return;
    if (t.head.entries + n > kMaxGroupEntries)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "%s: %lld entries and %lld ids more exceed the table's limit of 2^30 entries", who,
                 (long long)t.head.entries, (long long)n);
    PCV_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (!t.d_head.p) {
        t.pin_head.ensure(1);
        t.d_head.ensure(1);
        *t.pin_head.p = t.head;
        PCV_HIP(hipMemcpyAsync(t.d_head.p, t.pin_head.p, sizeof(GroupHead), hipMemcpyHostToDevice, st));
    }
    hipEvent_t ev[2] = {nullptr, nullptr};  // (the call's own: a searcher without rows has none yet)
    const auto drop_events = at_exit([&] {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    });
    for (hipEvent_t& e : ev) PCV_HIP(hipEventCreate(&e));
    PCV_HIP(hipEventRecord(ev[0], st));
    uint64_t slots = std::max(t.slots, kMinGroupSlots);
    while (slots < 2 * (uint64_t)(t.head.entries + n)) slots *= 2;
    if (slots != t.slots) grow_table(s, t, who, slots);
    auto trim = at_exit([&] { trim_table_scratch(t); });
    t.d_claim.ensure(t.slots);
    PCV_HIP(hipMemsetAsync(t.d_claim.p, 0, t.slots * sizeof(uint32_t), st));
    const size_t m_most = (size_t)std::min<int64_t>(n, kGroupBatch);
    t.d_batch.ensure(2 * m_most);
    t.d_slot.ensure(m_most);
    for (int64_t i0 = 0; i0 < n; i0 += kGroupBatch) {
        const size_t m = (size_t)std::min<int64_t>(kGroupBatch, n - i0);
        PCV_HIP(hipMemcpyAsync(t.d_batch.p, ids + i0, m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemcpyAsync(t.d_batch.p + m_most, vals + i0, m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        launch_group_upsert(st, t.keys, t.vals, (uint32_t)(t.slots - 1), t.d_claim.p, t.d_head.p, t.d_batch.p, t.d_batch.p + m_most,
                            (uint32_t)m, t.d_slot.p, t.none);
    }
    PCV_HIP(hipMemcpyAsync(t.pin_head.p, t.d_head.p, sizeof(GroupHead), hipMemcpyDeviceToHost, st));
    PCV_HIP(hipEventRecord(ev[1], st));
    PCV_HIP(hipStreamSynchronize(st));
    t.head = *t.pin_head.p;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    t.last_set_ms = ms;
}

// The table is as created: no slots, every counter 0.
void clear_table(pcv_searcher* s, pcv_searcher::IdTable& t) {
    PCV_HIP(hipSetDevice(s->ctx->device));
    PCV_HIP(hipStreamSynchronize(s->ctx->stream));
    if (t.keys) (void)hipFree(t.keys);
    if (t.vals) (void)hipFree(t.vals);
    t.keys = t.vals = nullptr;
    t.slots = 0;
    t.head = GroupHead{0, 0, t.none, 0, 0};
    t.d_head.release();  // (the next upsert uploads a fresh one)
    t.d_claim.release();
    t.rehashes = 0;
    t.last_set_ms = 0.0f;
}

// out[i] = what table `t` of `owner` (locked by the caller) holds for ids[i]; the scratch is owner's too.
void get_table(pcv_searcher* owner, pcv_searcher::IdTable& t, const int64_t* ids, int64_t n, int64_t* out) {
    if (!t.d_head.p) {  // nothing was ever set
        for (int64_t i = 0; i < n; ++i) out[i] = t.none;
        return;
    }
    PCV_HIP(hipSetDevice(owner->ctx->device));
    hipStream_t st = owner->ctx->stream;
    auto trim = at_exit([&] { trim_table_scratch(t); });
    const size_t m_most = (size_t)std::min<int64_t>(n, kGroupBatch);
    t.d_batch.ensure(2 * m_most);
    for (int64_t i0 = 0; i0 < n; i0 += kGroupBatch) {
        const size_t m = (size_t)std::min<int64_t>(kGroupBatch, n - i0);
        PCV_HIP(hipMemcpyAsync(t.d_batch.p, ids + i0, m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        launch_group_lookup(st, t.keys, t.vals, (uint32_t)(t.slots ? t.slots - 1 : 0), t.d_head.p, t.d_batch.p, (uint32_t)m, t.d_batch.p + m_most,
                            t.none);
        PCV_HIP(hipMemcpyAsync(out + i0, t.d_batch.p + m_most, m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
    }
}

// ---- grouped results (pcv_searcher_search_grouped; DESIGN.md §4 "Grouped results") ----
// search_distinct's walk (walk_ranked_lists) with membership as the relation: after each pass grouped_select_kernel looks the
// hits' ids up in the group table of `owner` (s itself, or the parent of a view; locked by the caller), keeps the first row of
// every group not kept yet and counts the others for the kept row of their group.  The state block is the one search_distinct
// uses, with the kept rows' group keys where that call has their norms — and these come down with the kept rows.
void search_grouped(const RankedCall& c, const pcv_searcher* owner, int64_t* out_groups, int32_t* out_collapsed) {
    pcv_searcher* s = c.s;
    DistinctViews v;  // (as in search_distinct)
    auto extra = [&](size_t at, const size_t* i) {
        if (out_groups) out_groups[at] = i ? v.pin.group[*i] : PCV_NO_GROUP;
        if (out_collapsed) out_collapsed[at] = i ? v.pin.count[*i] : 0;
    };
    SearchPlan plan;
    if (!open_ranked(c, "search_grouped", plan, 0, extra)) return;
    v = distinct_views(s);
    GroupedArgs args{};
    args.rec = v.dev.rec;
    args.rec_host = v.pin.rec;
    args.kept = v.dev.kept;
    args.collapsed = v.dev.count;
    args.kept_group = v.dev.group;
    args.keys = owner->groups.slots ? owner->groups.keys : nullptr;
    args.vals = owner->groups.vals;
    args.mask = owner->groups.slots ? (uint32_t)(owner->groups.slots - 1) : 0;
    args.side_val = owner->groups.head.side_val;
    args.num_results = c.k;
    collapse_ranked(c, plan, v, DistinctLayout::total, [&] {
        launch_grouped_select(s->ctx->stream, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
    }, extra);
}

// ---- filtered search (pcv_searcher_search_where / _count_where; DESIGN.md §4 "Item values and filtered search") ----
ValueTable value_table_of(const pcv_searcher* owner) {
    const pcv_searcher::IdTable& t = owner->values;
    return ValueTable{t.slots ? t.keys : nullptr, t.vals, t.slots ? (uint32_t)(t.slots - 1) : 0u, t.head.side_val};
}

// The third client of the ranked-call frame: the walk of search_grouped with the predicate as the test.  After each pass
// where_select_kernel looks the hits' ids up in the value table of `owner` and keeps the hits that pass; the state block is
// DistinctLayout's, with the kept rows' values where search_grouped has their group keys (and no counters: nothing is collapsed).
void search_where(const RankedCall& c, const pcv_searcher* owner, const WherePred& w, int64_t* out_values) {
    pcv_searcher* s = c.s;
    DistinctViews v;  // (as in search_distinct)
    auto extra = [&](size_t at, const size_t* i) {
        if (out_values) out_values[at] = i ? v.pin.group[*i] : kNoValue;
    };
    SearchPlan plan;
    if (!open_ranked(c, "search_where", plan, 0, extra)) return;
    v = distinct_views(s);
    WhereArgs args{};
    args.rec = v.dev.rec;
    args.rec_host = v.pin.rec;
    args.kept = v.dev.kept;
    args.kept_value = v.dev.group;
    args.table = value_table_of(owner);
    args.where = w;
    args.num_results = c.k;
    collapse_ranked(c, plan, v, DistinctLayout::total, [&] {
        launch_where_select(s->ctx->stream, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
    }, extra);
}

// ---- boosted results (pcv_searcher_search_boosted; DESIGN.md §4 "Boosted results") ----
// The state block of one group of Q queries: the walk's records and, per kept row, the hit, its boosted score, its value and its
// rank — two 8-byte columns and one 4-byte column, so a layout of its own, the same on both sides.  The columns are packed for the
// group's own number of queries, so that what comes down at the end is one copy of what the group wrote and no more.
namespace {
struct BoostLayout {
    size_t off_kept, off_m, off_value, off_rank, total;
    explicit BoostLayout(size_t Q) {
        off_kept = (size_t)kMfmaQueries * sizeof(DistinctRec);
        off_m = off_kept + Q * kMaxK * sizeof(pcv_hit_dev);
        off_value = off_m + Q * kMaxK * sizeof(double);
        off_rank = off_value + Q * kMaxK * sizeof(int64_t);
        total = off_rank + Q * kMaxK * sizeof(int32_t);
    }
};
}  // namespace

// The fourth client of the ranked-call frame: the walk of search_where with a re-ranking in place of the test.  After each pass
// boost_select_kernel merges the pass's hits into the kept rows under m = fl(rel + boost(value)) and tests the certificate; a query
// is finished when the certificate holds or its list ended, and what stops at `pool` unfinished is not exact.  There is no "more"
// pass: the last column is the record's flag.
void search_boosted(const RankedCall& c, const pcv_searcher* owner, const pcv_boost& boost, double* out_boosted, int64_t* out_values,
                    int32_t* out_ranks) {
    pcv_searcher* s = c.s;
    const pcv_hit_dev* r_kept = nullptr;  // (of the pinned block, once the call has rows to search)
    const double* r_m = nullptr;
    const int64_t* r_value = nullptr;
    const int32_t* r_rank = nullptr;
    auto extra = [&](size_t at, const size_t* i) {
        if (out_boosted) out_boosted[at] = i ? r_m[*i] : NAN;
        if (out_values) out_values[at] = i ? r_value[*i] : kNoValue;
        if (out_ranks) out_ranks[at] = i ? r_rank[*i] : -1;
    };
    SearchPlan plan;
    if (!open_ranked(c, "search_boosted", plan, 1, extra)) return;  // (exact: the list ended before the pool did)
    hipStream_t st = s->ctx->stream;
    s->d_boost.ensure(BoostLayout(kMfmaQueries).total);
    s->pin_boost.ensure(BoostLayout(kMfmaQueries).total);
    uint8_t *dev = s->d_boost.p, *pin = s->pin_boost.p;
    DistinctRec* rec = reinterpret_cast<DistinctRec*>(pin);
    BoostArgs args{};
    args.rec = reinterpret_cast<DistinctRec*>(dev);
    args.rec_host = rec;
    args.table = value_table_of(owner);
    args.boost = boost;
    args.b_max = boost.unset_boost;
    for (int j = 0; j < boost.n_knots; ++j) args.b_max = std::max(args.b_max, boost.knot_boosts[j]);
    args.num_results = c.k;
    each_query_group(c, plan.qstep, [&](int q0, int B, const float* qs) {
        const BoostLayout L((size_t)B);
        args.kept = reinterpret_cast<pcv_hit_dev*>(dev + L.off_kept);
        args.kept_m = reinterpret_cast<double*>(dev + L.off_m);
        args.kept_value = reinterpret_cast<int64_t*>(dev + L.off_value);
        args.kept_rank = reinterpret_cast<int32_t*>(dev + L.off_rank);
        r_kept = reinterpret_cast<const pcv_hit_dev*>(pin + L.off_kept);
        r_m = reinterpret_cast<const double*>(pin + L.off_m);
        r_value = reinterpret_cast<const int64_t*>(pin + L.off_value);
        r_rank = reinterpret_cast<const int32_t*>(pin + L.off_rank);
        walk_ranked_lists(s, plan, qs, B, c.pool, rec, args.rec, false, [&] {
            launch_boost_select(st, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
        });
        PCV_HIP(hipMemcpyAsync(pin + L.off_kept, dev + L.off_kept, L.total - L.off_kept, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < B; ++q)
            write_ranked(c, q0 + q, q, (int)rec[q].kept, (int32_t)rec[q].examined, rec[q].flags != 0 ? 1 : 0, [&](size_t i) { return r_kept[i]; }, extra);
    });
}

// ---- compound queries (pcv_searcher_search_compound; DESIGN.md §4 "Compound queries") ----
// The state block of one group of compounds: the walk's records — one per PART query, as walk_ranked_lists wants them — and, per
// kept row of each of the group's C compounds, the hit (its score: m), its penalty and its canonical score under each wanted
// vector; the same layout on both sides, packed for the group's own number of compounds as BoostLayout is.
namespace {
struct CompoundLayout {
    size_t off_kept, off_pen, off_part, total;
    explicit CompoundLayout(size_t C) {
        off_kept = (size_t)kMfmaQueries * sizeof(DistinctRec);
        off_pen = off_kept + C * kMaxK * sizeof(pcv_hit_dev);
        off_part = off_pen + C * kMaxK * sizeof(double);
        total = off_part + C * kMaxK * kMaxCompoundParts * sizeof(double);
    }
};
}  // namespace

double query_norm2(const float* q, int D) {
    double nq = 0.0;
    for (int i = 0; i < D; ++i) nq += (double)q[i] * (double)q[i];
    return nq;
}

// The fifth client of the ranked-call frame: the wanted vectors of a compound are adjacent queries of one group, walked in lockstep,
// and after each pass compound_select_kernel scores the rows met for the first time under every vector of their compound, merges them
// into the kept rows and tests the certificate.  The avoided vectors are uploaded once, with the descriptors and the norms; a group
// takes whole compounds, as many as fit a pass.  The last column is the record's flag, as in search_boosted.
void search_compound(const CompoundCall& c) {
    pcv_searcher* s = c.s;
    const int D = s->D, Dp = s->D4 * 4;
    const int n_want = (int)c.want_off[c.n], n_avoid = c.avoid_off ? (int)c.avoid_off[c.n] : 0;
    auto width = [&](int i) { return (int)(c.want_off[i + 1] - c.want_off[i]); };
    auto blank = [&](int i, int from) {
        for (int j = from; j < c.k; ++j) {
            const size_t at = (size_t)i * c.k + j;
            if (c.out_ids) c.out_ids[at] = -1;
            if (c.out_combined) c.out_combined[at] = NAN;
            if (c.out_penalties) c.out_penalties[at] = NAN;
            if (c.out_part_scores)
                for (int u = 0; u < kMaxCompoundParts; ++u) c.out_part_scores[at * kMaxCompoundParts + u] = NAN;
        }
    };
    // (the frame's opening — argument check, statistics, plan, open_search — with the wanted vectors as the call's queries: the
    // kernel is picked for all of them; its blank answer is per query, so the compounds' is written here)
    const RankedCall frame{s, c.want, n_want, c.source_ids, c.n_sources, c.k, c.pool, nullptr, nullptr, nullptr, nullptr, nullptr};
    check_search_args(s, c.want, n_want, c.k, "search_compound");
    {
        const int qstep = pass_queries(s, pick_kernel(s, n_want));
        for (int i = 0; i < c.n; ++i)
            if (width(i) > qstep)
                PCV_FAIL(PCV_ERR_UNSUPPORTED,
                         "search_compound: compound %d has %d wanted vectors, but a pass of this searcher's kernel takes %d queries "
                         "(the wave kernel: use PCV_KERNEL_MFMA or PCV_KERNEL_AUTO)",
                         i, width(i), qstep);
    }
    SearchPlan plan;
    if (!open_ranked(frame, "search_compound", plan, 1, [](size_t, const size_t*) {})) {
        for (int i = 0; i < c.n; ++i) {  // (exact: there is nothing to miss)
            blank(i, 0);
            if (c.out_counts) c.out_counts[i] = 0;
            if (c.out_examined) c.out_examined[i] = 0;
            if (c.out_exact) c.out_exact[i] = 1;
        }
        return;
    }
    hipStream_t st = s->ctx->stream;
    // the call's tables: descriptors | norms of the wanted vectors | norms of the avoided vectors | the avoided vectors, zero padded
    const size_t off_wn = (size_t)c.n * sizeof(CompoundDesc), off_an = off_wn + (size_t)n_want * sizeof(double);
    const size_t off_av = off_an + (size_t)(n_avoid + 1) * sizeof(double), tab_bytes = off_av + (size_t)(n_avoid + 1) * Dp * sizeof(float);
    std::vector<uint8_t> tab(tab_bytes, 0);
    CompoundDesc* desc = reinterpret_cast<CompoundDesc*>(tab.data());
    double* wn = reinterpret_cast<double*>(tab.data() + off_wn);
    double* an = reinterpret_cast<double*>(tab.data() + off_an);
    float* av = reinterpret_cast<float*>(tab.data() + off_av);
    for (int q = 0; q < n_want; ++q) wn[q] = query_norm2(c.want + (size_t)q * D, D);
    for (int q = 0; q < n_avoid; ++q) {
        an[q] = query_norm2(c.avoid + (size_t)q * D, D);
        std::memcpy(av + (size_t)q * Dp, c.avoid + (size_t)q * D, (size_t)D * sizeof(float));
    }
    // groups of whole compounds: as many as a pass takes queries
    std::vector<int> first{0};  // first compound of every group, and the end
    for (int i = 0, used = 0; i < c.n; ++i) {
        if (used + width(i) > plan.qstep) first.push_back(i), used = 0;
        desc[i].first_query = used;
        desc[i].n_want = width(i);
        desc[i].first_avoid = c.avoid_off ? (int32_t)c.avoid_off[i] : 0;
        desc[i].n_avoid = c.avoid_off ? (int32_t)(c.avoid_off[i + 1] - c.avoid_off[i]) : 0;
        used += width(i);
    }
    first.push_back(c.n);
    size_t most = 0;
    for (size_t g = 0; g + 1 < first.size(); ++g) most = std::max(most, (size_t)(first[g + 1] - first[g]));
    s->d_compound.ensure(CompoundLayout(most).total);
    s->pin_compound.ensure(CompoundLayout(most).total);
    s->d_compound_tab.ensure(tab_bytes);
    PCV_HIP(hipMemcpyAsync(s->d_compound_tab.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
    PCV_HIP(hipStreamSynchronize(st));  // (`tab` is pageable and the call's own)
    uint8_t *dev = s->d_compound.p, *pin = s->pin_compound.p, *dtab = s->d_compound_tab.p;
    DistinctRec* rec = reinterpret_cast<DistinctRec*>(pin);
    CompoundArgs args{};
    args.rec = reinterpret_cast<DistinctRec*>(dev);
    args.rec_host = rec;
    args.avoid = reinterpret_cast<const float*>(dtab + off_av);
    args.avoid_norm = reinterpret_cast<const double*>(dtab + off_an);
    args.num_results = c.k;
    args.mode = c.mode;
    args.lambda = c.lambda;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int c0 = first[g], C = first[g + 1] - c0, q0 = (int)c.want_off[c0], B = (int)c.want_off[c0 + C] - q0;
        const CompoundLayout L((size_t)C);
        args.desc = reinterpret_cast<const CompoundDesc*>(dtab) + c0;
        args.want_norm = reinterpret_cast<const double*>(dtab + off_wn) + q0;
        args.kept = reinterpret_cast<pcv_hit_dev*>(dev + L.off_kept);
        args.kept_pen = reinterpret_cast<double*>(dev + L.off_pen);
        args.kept_part = reinterpret_cast<double*>(dev + L.off_part);
        args.n_compounds = C;
        args.max_want = args.max_vectors = 0;
        for (int i = c0; i < c0 + C; ++i) {
            args.max_want = std::max(args.max_want, desc[i].n_want);
            args.max_vectors = std::max(args.max_vectors, desc[i].n_want + desc[i].n_avoid);
        }
        walk_ranked_lists(s, plan, c.want + (size_t)q0 * D, B, c.pool, rec, args.rec, false, [&] {
            launch_compound_select(st, pass_params(s), reinterpret_cast<const ScanParams*>(s->d_pass.p), args);
        });
        PCV_HIP(hipMemcpyAsync(pin + L.off_kept, dev + L.off_kept, L.total - L.off_kept, hipMemcpyDeviceToHost, st));
        PCV_HIP(hipStreamSynchronize(st));
        const pcv_hit_dev* r_kept = reinterpret_cast<const pcv_hit_dev*>(pin + L.off_kept);
        const double* r_pen = reinterpret_cast<const double*>(pin + L.off_pen);
        const double* r_part = reinterpret_cast<const double*>(pin + L.off_part);
        for (int i = c0; i < c0 + C; ++i) {
            const DistinctRec& r = rec[desc[i].first_query];  // (every part's record carries the compound's counters and flags)
            const int n = (int)r.kept;
            for (int j = 0; j < n; ++j) {
                const size_t at = (size_t)i * c.k + j, from = (size_t)(i - c0) * kMaxK + j;
                if (c.out_ids) c.out_ids[at] = r_kept[from].id;
                if (c.out_combined) c.out_combined[at] = r_kept[from].score;
                if (c.out_penalties) c.out_penalties[at] = r_pen[from];
                if (c.out_part_scores)
                    for (int u = 0; u < kMaxCompoundParts; ++u)
                        c.out_part_scores[at * kMaxCompoundParts + u] =
                            u < desc[i].n_want ? reported_score(s->metric, D, r_part[from * kMaxCompoundParts + u]) : NAN;
            }
            blank(i, n);
            if (c.out_counts) c.out_counts[i] = n;
            if (c.out_examined) c.out_examined[i] = (int32_t)r.examined;
            if (c.out_exact) c.out_exact[i] = r.flags != 0 ? 1 : 0;
        }
    }
}

// The exact count: where_mark_kernel over every selected segment (the scratch of one segment at a time: launches of one stream
// follow each other), the tile counts summed on the device into two int64, which come down once.
void count_where(pcv_searcher* s, const pcv_searcher* owner, const int64_t* source_ids, int n_sources, const WherePred& w,
                 int64_t* out_rows, int64_t* out_searchable) {
    PCV_REQUIRE(!s->dirty, "count_where: rows were added or cleared without pcv_searcher_finalize");
    int64_t got[2] = {0, 0};
    const std::vector<SelSeg> segs = select_segments(s, source_ids, n_sources);
    if (!segs.empty()) {
        PCV_HIP(hipSetDevice(s->ctx->device));
        hipStream_t st = s->ctx->stream;
        uint32_t most = 0;
        for (const SelSeg& g : segs) most = std::max(most, view_tiles(g.g->nrows));
        // (the call's scratch is the searcher's, kept for the next call unless it is large)
        DevBuf<uint32_t>&flags4 = s->d_where_flags, &tiles = s->d_where_tiles;
        DevBuf<int64_t>& acc = s->d_where_acc;
        PinBuf<int64_t>& pin_acc = s->pin_where_acc;
        const auto trim = at_exit([&] {
            if (flags4.n * sizeof(uint32_t) > kGroupKeptBytes) flags4.release();
        });
        flags4.ensure((size_t)most * 256);
        tiles.ensure((size_t)most * 2);
        acc.ensure(2);
        pin_acc.ensure(2);
        const ValueTable t = value_table_of(owner);
        try {
            PCV_HIP(hipMemsetAsync(acc.p, 0, 2 * sizeof(int64_t), st));
            for (const SelSeg& g : segs) {
                const uint32_t nt = view_tiles(g.g->nrows);
                launch_where_mark(st, g.g->ids, g.g->id0, g.g->scale, g.g->nrows, t, w, flags4.p, tiles.p, tiles.p + most);
                launch_where_sum(st, tiles.p, tiles.p + most, nt, acc.p);
            }
            PCV_HIP(hipMemcpyAsync(pin_acc.p, acc.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            PCV_HIP(hipStreamSynchronize(st));
            PCV_HIP(hipGetLastError());
        } catch (...) {
            (void)hipStreamSynchronize(st);  // (the scratch may be released)
            throw;
        }
        got[0] = pin_acc.p[0];
        got[1] = pin_acc.p[1];
    }
    if (out_rows) *out_rows = got[0];
    if (out_searchable) *out_searchable = got[1];
}

// The per-shard pass of the begin/end protocol; the caller holds s->mu.
void device_begin(pcv_searcher* s, const float* queries, int n_queries, const int64_t* source_ids, int n_sources, int k,
                  pcv_hit_dev* out, bool queries_on_device) {
    // (a device pointer is not read on the host; host queries: only what every rank evaluates alike)
    check_search_args(s, queries, n_queries, k, "search_device_begin", kMaxK, queries_on_device ? kEnvelopeNone : kEnvelopeQuery);
    PCV_REQUIRE(!s->pending.active, "search_device_begin: the previous pass was not collected (search_device_end)");
    sync_view(s);
    const SearchPlan plan = plan_search(s, source_ids, n_sources, n_queries, true);
    // Only a condition every rank evaluates alike may refuse: the ranks of a sharded search must all
    // take the same protocol (the exchanged payload differs by the overflow record).
    if (n_queries > plan.qstep)
        PCV_FAIL(PCV_ERR_UNSUPPORTED, "search_device_begin: %d queries need more than one pass%s", n_queries,
                 s->wide_sharded ? " (wide sharded passes were allowed, but not every row of THIS rank has its int8 screening copy)" : "");
    const size_t n = (size_t)n_queries * k;
    if (!open_search(s, plan)) {  // (each rank builds mid copies by its own statistics: the copy changes no result and no protocol)
        // this shard holds none of the selected rows: hand over the same layout — empty lists and a clear
        // overflow record — from pinned memory; search_device_end waits for the copy like for a pass
        ensure_workspace(s);
        const pcv_hit_dev none{NAN, -1, -1};
        for (size_t i = 0; i < n; ++i) s->pin->hits[i] = none;
        s->pin->hits[n] = pcv_hit_dev{0.0, 0, 0};
        PCV_HIP(hipMemcpyAsync(out, s->pin->hits, (n + 1) * sizeof(pcv_hit_dev), hipMemcpyHostToDevice, s->ctx->stream));
        s->pending.active = true;
        s->pending.done = true;
        return;
    }
    PassRequest pass = PassRequest(queries, n_queries, plan.segs, plan.kernel).top_k(k, out, false, out + n);
    if (queries_on_device) pass.where = PassRequest::kDevice;
    enqueue_pass(s, pass);
    if (s->view_parent) launch_view_remap(s->ctx->stream, out, (int64_t)n, s->d_ppos.p, s->view_rows);  // (before any exchange)
}

// ---- search by example (pcv_searcher_like_queries / _search_like; DESIGN.md §3 "Search by example") ----
// What both entry points check before anything touches the searcher or the device; returns the number of examples.
int64_t check_like_args(const pcv_searcher* s, const int64_t* example_ids, const float* weights, const int64_t* offsets, int n_queries,
                        const char* who) {
    PCV_REQUIRE(s != nullptr, "%s: searcher is NULL", who);
    PCV_REQUIRE(n_queries >= 0, "%s: n_queries < 0", who);
    PCV_REQUIRE(offsets != nullptr, "%s: offsets is NULL", who);
    PCV_REQUIRE(offsets[0] == 0, "%s: offsets[0] must be 0", who);
    for (int q = 0; q < n_queries; ++q)
        PCV_REQUIRE(offsets[q + 1] >= offsets[q], "%s: offsets are not ascending (offsets[%d] < offsets[%d])", who, q + 1, q);
    const int64_t n = offsets[n_queries];
    PCV_REQUIRE(n <= 0x7fffffff, "%s: %lld examples in one call", who, (long long)n);
    PCV_REQUIRE(example_ids != nullptr || n == 0, "%s: example ids NULL with %lld examples", who, (long long)n);
    if (weights)
        for (int64_t i = 0; i < n; ++i) PCV_REQUIRE(std::isfinite(weights[i]), "%s: weight %lld is not finite", who, (long long)i);
    return n;
}

// The searcher the examples are looked up in (a view: its parent — an example need not be among the allowed items), locked, in
// the state both calls need.  The caller holds s->mu and has brought a view up to date.
std::unique_lock<std::mutex> lock_like_owner(pcv_searcher* s, pcv_searcher*& owner, const char* who) {
    PCV_REQUIRE(!s->pending.active, "%s: a queued pass has not been collected", who);
    owner = s->view_parent ? s->view_parent : s;
    std::unique_lock<std::mutex> lk;
    if (owner != s) lk = std::unique_lock<std::mutex>(owner->mu);
    PCV_REQUIRE(!owner->dirty, "%s: pending rows; call pcv_searcher_finalize first", who);
    PCV_REQUIRE(!owner->pending.active, "%s: a queued pass has not been collected", who);
    return lk;
}

// Query vectors from stored items (p->mu held, p no view): the distinct ids of the call are looked up once in every segment
// (find_slots: an id column is streamed against the batch's table, implicit ids are arithmetic), each id's rows listed in
// ascending global position, the lists expanded per query in the order the examples were given, and like_queries_kernel sums
// the rows.  Reads rows and ids only.
void build_like_queries(pcv_searcher* p, const int64_t* example_ids, const float* weights, const int64_t* offsets, int n_queries,
                        bool want_host, void* d_out, LikeBuilt& out) {
    const int64_t n = offsets[n_queries];
    out.member_rows.assign((size_t)n_queries, 0);
    out.carrier_rows.assign((size_t)n_queries, 0);
    out.found.assign((size_t)n, 0);
    if (want_host) out.vectors.assign((size_t)n_queries * p->D, 0.0f);
    if (n_queries == 0) return;
    PCV_HIP(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    // 1. one slot per distinct id
    std::vector<int64_t> uniq(example_ids, example_ids + n);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<uint32_t> slot_of(uniq.size());
    std::iota(slot_of.begin(), slot_of.end(), 0u);
    // 2. the rows of every slot: (segment of the table, row), ascending in global position — sources and segments are walked in
    //    the order assign_positions numbers them, rows ascending inside a segment
    std::vector<SegDesc> segs;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> rows_of(uniq.size());
    std::vector<int64_t> staged_of(uniq.size(), 0);
    if (!uniq.empty()) {
        IdBatch b;
        b.ids = &uniq;
        b.slots = &slot_of;
        for (const auto& src : p->sources)
            for (const auto& g : src.segs) {
                if (g.nrows == 0) continue;
                auto pr = find_slots(p, g, b);
                if (pr.empty()) continue;
                if (src.id == PCV_STAGING_SOURCE) {  // nobody's rows yet: no members, but a search that names the source may meet them
                    for (const auto& x : pr) staged_of[x.first] += 1;
                    continue;
                }
                std::sort(pr.begin(), pr.end(), [](const auto& a, const auto& c) { return a.second < c.second; });
                PCV_REQUIRE(segs.size() < 0x7fffffffu, "like_queries: too many segments");
                const uint32_t si = (uint32_t)segs.size();
                SegDesc d{};  // (like_queries_kernel reads the rows and their number; no copy is involved)
                d.blk = g.blk;
                d.scale = g.scale;
                d.ids = g.ids;
                d.id0 = g.id0;
                d.pos0 = g.pos0;
                d.nrows = g.nrows;
                d.nblocks = g.nblocks();
                segs.push_back(d);
                for (const auto& x : pr) rows_of[x.first].push_back({si, x.second});
            }
    }
    // 3. the member list, per query in the order given
    std::vector<LikeMember> members;
    std::vector<uint32_t> first((size_t)n_queries + 1, 0);
    for (int q = 0; q < n_queries; ++q) {
        for (int64_t i = offsets[q]; i < offsets[q + 1]; ++i) {
            const size_t slot = (size_t)(std::lower_bound(uniq.begin(), uniq.end(), example_ids[i]) - uniq.begin());
            const auto& rows = rows_of[slot];
            out.found[(size_t)i] = rows.empty() ? 0 : 1;
            out.carrier_rows[(size_t)q] += (int64_t)rows.size() + staged_of[slot];
            PCV_REQUIRE(members.size() + rows.size() <= 0x7fffffffu, "like_queries: more than 2^31 member rows in one call");
            for (const auto& r : rows) members.push_back(LikeMember{r.first, r.second, weights ? weights[i] : 1.0f});
        }
        first[(size_t)q + 1] = (uint32_t)members.size();
        out.member_rows[(size_t)q] = (int64_t)(first[(size_t)q + 1] - first[(size_t)q]);
    }
    // 4. the sums
    DevBuf<SegDesc> d_segs;
    DevBuf<LikeMember> d_members;
    DevBuf<uint32_t> d_first;
    DevBuf<float> d_vec;
    try {
        d_segs.ensure(segs.size() + 1);
        d_members.ensure(members.size() + 1);
        d_first.ensure(first.size());
        d_vec.ensure((size_t)n_queries * p->D);
        if (!segs.empty()) PCV_HIP(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, st));
        if (!members.empty())
            PCV_HIP(hipMemcpyAsync(d_members.p, members.data(), members.size() * sizeof(LikeMember), hipMemcpyHostToDevice, st));
        PCV_HIP(hipMemcpyAsync(d_first.p, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        launch_like_queries(st, d_segs.p, (int)segs.size(), d_members.p, d_first.p, n_queries, p->D, p->D4, d_vec.p);
        const size_t bytes = (size_t)n_queries * p->D * sizeof(float);
        if (want_host) PCV_HIP(hipMemcpyAsync(out.vectors.data(), d_vec.p, bytes, hipMemcpyDeviceToHost, st));
        if (d_out) PCV_HIP(hipMemcpyAsync(d_out, d_vec.p, bytes, hipMemcpyDeviceToDevice, st));
        PCV_HIP(hipStreamSynchronize(st));
        PCV_HIP(hipGetLastError());
    } catch (...) {
        (void)hipStreamSynchronize(st);  // (before the buffers queued work may still read are freed)
        throw;
    }
}

}  // namespace pcv
