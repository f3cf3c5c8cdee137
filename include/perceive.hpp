// perceive.hpp — C++ host-side mirror of perceive-core's public surface over the C ABI
// (include/perceive_hip.h).  Header-only.  The reference is a compiled (Rust) library; no Rust
// toolchain exists in the build image, so this is the compiled-language form of the shim in
// shim/perceive-core: same names, argument meaning and error behaviour as
//   crates/perceive-core/search.rs   (Searcher, SearchItem, serialize/deserialize_embedding)
//   crates/perceive-core/model.rs    (Model, ModelError, SentenceEmbeddingsModelType)
//   crates/perceive-core/lib.rs:63-77 (dot_product, cosine_similarity_*)
// Errors: the reference returns Result<_, ModelError/DbError/eyre::Report>; here a failing status
// throws perceive::Error carrying pcv_last_error().
#pragma once
#include <algorithm>
#include <cstdint>
#include <array>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_set>
#include <utility>
#include <vector>

#include "perceive_hip.h"

namespace perceive {

struct Error : std::runtime_error {
    pcv_status status;
    Error(pcv_status s, const std::string& what) : std::runtime_error(what), status(s) {}
};
struct ModelError : Error {  // model.rs:29-42
    using Error::Error;
};

inline void check(pcv_status s) {
    if (s != PCV_OK) throw Error(s, pcv_last_error());
}

// one process drives one GPU; replaces tch::Device::cuda_if_available() (model.rs:117)
class Context {
public:
    explicit Context(int device_index = 0) { check(pcv_init(device_index, &h_)); }
    ~Context() { pcv_shutdown(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    pcv_ctx* handle() const { return h_; }
    void synchronize() { check(pcv_synchronize(h_)); }

private:
    pcv_ctx* h_ = nullptr;
};

// search.rs:18-22
struct SearchItem {
    int64_t id;
    float score;
};

// search.rs:281-294
inline std::vector<float> deserialize_embedding(const std::vector<uint8_t>& value) {
    std::vector<float> out(value.size() / 4);
    size_t n = 0;
    check(pcv_deserialize_embedding(value.data(), value.size(), out.data(), out.size(), &n));
    out.resize(n);
    return out;
}
inline std::vector<uint8_t> serialize_embedding(const std::vector<float>& embedding) {
    std::vector<uint8_t> out(embedding.size() * 4);
    check(pcv_serialize_embedding(embedding.data(), embedding.size(), out.data(), out.size()));
    return out;
}

// One row of the query Searcher::build runs (search.rs:87-93): (items.id, source_id, embedding BLOB)
struct EmbeddingRow {
    int64_t item_id;
    int64_t source_id;
    std::vector<uint8_t> embedding;
};

enum class Metric { Cosine = PCV_METRIC_COSINE, Dot = PCV_METRIC_DOT };

// A persistent RCCL communicator for the row-sharded Searcher (one process per GPU).  Rank 0 makes the
// id and the host ships its 128 bytes to every rank by its own means; no reference counterpart (the
// reference is one process), it is the multi-GPU form of search.rs:163-181.
class Comm {
public:
    static std::array<uint8_t, 128> unique_id() {
        std::array<uint8_t, 128> id{};
        check(pcv_comm_unique_id(id.data()));
        return id;
    }
    Comm(Context& ctx, int world_size, int rank, const std::array<uint8_t, 128>& id) {
        check(pcv_comm_create(ctx.handle(), world_size, rank, id.data(), &h_));
    }
    ~Comm() { pcv_comm_destroy(h_); }  // before its Context
    Comm(const Comm&) = delete;
    Comm& operator=(const Comm&) = delete;
    pcv_comm* handle() const { return h_; }

private:
    pcv_comm* h_ = nullptr;
};

// `perceive search --like <id>` (cmd/search.rs:64-86) on a searcher or a view handle: the stored embedding of `item_id` is the
// query (pcv_searcher_search_like); nullopt when no row carries the id ("Item not found", cmd/search.rs:83).
inline std::optional<std::vector<SearchItem>> search_like_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                                 int64_t item_id, bool exclude) {
    const int64_t offsets[2] = {0, 1}, no_source = 0;
    std::vector<int64_t> ids(num_results);
    std::vector<float> scores(num_results);
    int count = 0;
    uint8_t found = 0;
    // (an empty filter matches nothing, like `sources.contains(..)`: the pointer stays non-NULL)
    check(pcv_searcher_search_like(h, &item_id, nullptr, offsets, 1, sources.empty() ? &no_source : sources.data(), (int)sources.size(),
                                   (int)num_results, exclude ? 1 : 0, ids.data(), scores.data(), &count, &found));
    if (!found) return std::nullopt;
    std::vector<SearchItem> out;
    for (int i = 0; i < count; ++i) out.push_back({ids[i], scores[i]});
    return out;
}

// Range search on a searcher or a view handle (pcv_searcher_search_range): the items whose reported score passes `bound` (cosine:
// score >= bound; Dot: distance <= bound), best first, at most max_results.  `more`, if given: more items are in range.
inline std::vector<SearchItem> search_range_handle(pcv_searcher* h, const std::vector<int64_t>& sources, float bound, size_t max_results,
                                                   const std::vector<float>& vector, bool* more) {
    if (more) *more = false;
    if (sources.empty() || max_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing (as the Rust twin)
    std::vector<int64_t> ids(max_results);
    std::vector<float> scores(max_results);
    int64_t count = 0;
    uint8_t m = 0;
    check(pcv_searcher_search_range(h, vector.data(), 1, sources.data(), (int)sources.size(), &bound, (int64_t)max_results, ids.data(),
                                    scores.data(), &count, &m));
    if (more) *more = m != 0;
    std::vector<SearchItem> out;
    for (int64_t i = 0; i < count; ++i) out.push_back({ids[(size_t)i], scores[(size_t)i]});
    return out;
}

// Distinct results on a searcher or a view handle (pcv_searcher_search_distinct): the ranked list of search_vector walked best first,
// an item kept iff its cosine with every item kept before it is below `threshold`; at most `pool` entries are examined (0: the
// default, min(PCV_MAX_DISTINCT_POOL, max(128, 8 * num_results))).  `similar`, if given: per hit, the examined items dropped in its favour.
inline std::vector<SearchItem> search_distinct_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                      const std::vector<float>& vector, float threshold, size_t pool,
                                                      std::vector<int32_t>* similar) {
    if (similar) similar->clear();
    if (sources.empty() || num_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_DISTINCT_POOL, std::max<size_t>(128, 8 * num_results));
    std::vector<int64_t> ids(num_results);
    std::vector<float> scores(num_results);
    std::vector<int32_t> sim(num_results);
    int32_t count = 0;
    check(pcv_searcher_search_distinct(h, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results, threshold, (int)pool,
                                       ids.data(), scores.data(), &count, sim.data(), nullptr, nullptr));
    std::vector<SearchItem> out;
    for (int i = 0; i < count; ++i) out.push_back({ids[(size_t)i], scores[(size_t)i]});
    if (similar) similar->assign(sim.begin(), sim.begin() + count);
    return out;
}

// One pick of search_vector_diverse: the item, the marginal value it was picked at and its place in the ranked list of search_vector.
struct DiverseItem {
    SearchItem item;
    double marginal;
    int32_t rank;
};
// Diverse results on a searcher or a view handle (pcv_searcher_search_diverse): exact greedy maximal marginal relevance over the
// first `pool` entries of the ranked list of search_vector (0: the default, min(PCV_MAX_DIVERSE_POOL, max(128, 8 * num_results))).
// Each pick maximises lambda * relevance - (1 - lambda) * (largest cosine with an item already picked), ties to the better rank;
// the picks come in pick order.  `exact`, if given: the picks are provably those of the same walk over the whole list.
inline std::vector<DiverseItem> search_diverse_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                      const std::vector<float>& vector, float lambda, size_t pool, bool* exact) {
    if (exact) *exact = true;
    if (sources.empty() || num_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_DIVERSE_POOL, std::max<size_t>(128, 8 * num_results));
    std::vector<int64_t> ids(num_results);
    std::vector<float> scores(num_results);
    std::vector<double> marginal(num_results);
    std::vector<int32_t> ranks(num_results);
    int32_t count = 0;
    uint8_t ex = 0;
    check(pcv_searcher_search_diverse(h, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results, lambda, (int)pool,
                                      ids.data(), scores.data(), marginal.data(), ranks.data(), &count, nullptr, &ex));
    std::vector<DiverseItem> out;
    for (int i = 0; i < count; ++i) out.push_back({{ids[(size_t)i], scores[(size_t)i]}, marginal[(size_t)i], ranks[(size_t)i]});
    if (exact) *exact = ex != 0;
    return out;
}

// One hit of search_vector_grouped: the best member of a group, the group's key (PCV_NO_GROUP: an item without a group, which is
// a group of its own) and the examined items collapsed into it.
struct GroupedItem {
    SearchItem item;
    int64_t group;
    int32_t collapsed;
};
// Grouped results on a searcher or a view handle (pcv_searcher_search_grouped): the ranked list of search_vector walked best first,
// an item kept iff no kept item has its group (Searcher::set_groups; a view reads its parent's); at most `pool` entries are
// examined (0: the default, min(PCV_MAX_GROUPED_POOL, max(128, 8 * num_results))).  `more`, if given: the walk stopped at `pool`
// short of num_results although the list went on.
inline std::vector<GroupedItem> search_grouped_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                      const std::vector<float>& vector, size_t pool, bool* more) {
    if (more) *more = false;
    if (sources.empty() || num_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_GROUPED_POOL, std::max<size_t>(128, 8 * num_results));
    std::vector<int64_t> ids(num_results), groups(num_results);
    std::vector<float> scores(num_results);
    std::vector<int32_t> collapsed(num_results);
    int32_t count = 0;
    uint8_t m = 0;
    check(pcv_searcher_search_grouped(h, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results, (int)pool, ids.data(),
                                      scores.data(), groups.data(), &count, collapsed.data(), nullptr, &m));
    if (more) *more = m != 0;
    std::vector<GroupedItem> out;
    for (int i = 0; i < count; ++i) out.push_back({{ids[(size_t)i], scores[(size_t)i]}, groups[(size_t)i], collapsed[(size_t)i]});
    return out;
}

// A predicate over the value of an item (Searcher::set_values): an item passes iff it has a value in [lo, hi] — `outside`: a value
// not in it —; `unset_passes`: items without a value pass too (pcv_searcher_count_where).
struct Where {
    int64_t lo = INT64_MIN + 1, hi = INT64_MAX;
    bool unset_passes = false, outside = false;
    uint32_t flags() const { return (unset_passes ? (uint32_t)PCV_WHERE_UNSET_PASSES : 0u) | (outside ? (uint32_t)PCV_WHERE_OUTSIDE : 0u); }
};
// One hit of search_vector_where: a passing item and its value (PCV_NO_VALUE: an item without one that passed).
struct ValuedItem {
    SearchItem item;
    int64_t value;
};
// Filtered search on a searcher or a view handle (pcv_searcher_search_where): the ranked list of search_vector walked best first,
// an item kept iff it passes `where` (a view reads its parent's values); at most `pool` entries are examined (0: the default,
// min(PCV_MAX_WHERE_POOL, max(128, 8 * num_results))).  `more`, if given: the walk stopped at `pool` short of num_results although
// the list went on — the predicate is too selective for this call: use Searcher::view_where.
inline std::vector<ValuedItem> search_where_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                   const std::vector<float>& vector, const Where& where, size_t pool, bool* more) {
    if (more) *more = false;
    if (sources.empty() || num_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_WHERE_POOL, std::max<size_t>(128, 8 * num_results));
    std::vector<int64_t> ids(num_results), values(num_results);
    std::vector<float> scores(num_results);
    int32_t count = 0;
    uint8_t m = 0;
    check(pcv_searcher_search_where(h, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results, (int)pool, where.lo, where.hi,
                                    where.flags(), ids.data(), scores.data(), values.data(), &count, nullptr, &m));
    if (more) *more = m != 0;
    std::vector<ValuedItem> out;
    for (int i = 0; i < count; ++i) out.push_back({{ids[(size_t)i], scores[(size_t)i]}, values[(size_t)i]});
    return out;
}
// The items of `sources` that pass `where`, and (`searchable`, if given) those of them a search could return.
inline int64_t count_where_handle(pcv_searcher* h, const std::vector<int64_t>& sources, const Where& where, int64_t* searchable) {
    int64_t rows = 0, live = 0;
    static const int64_t none = 0;  // (an empty list still needs a pointer: NULL means every source)
    check(pcv_searcher_count_where(h, sources.empty() ? &none : sources.data(), (int)sources.size(), where.lo, where.hi, where.flags(), &rows, &live));
    if (searchable) *searchable = live;
    return rows;
}

// A boost over the value of an item (Searcher::set_values): piecewise linear through (values[j], boosts[j]) — values strictly
// increasing, at most PCV_MAX_BOOST_KNOTS knots —, constant beyond both ends, `unset` for an item without a value
// (pcv_searcher_search_boosted).
struct Boost {
    std::vector<int64_t> values;
    std::vector<double> boosts;
    double unset = 0.0;
    pcv_boost raw() const {
        if (values.size() != boosts.size()) throw std::invalid_argument("Boost: values and boosts differ in length");
        pcv_boost b{};
        b.n_knots = (int32_t)std::min<size_t>(values.size(), (size_t)PCV_MAX_BOOST_KNOTS + 1);  // (none or too many: the library refuses)
        for (size_t j = 0; j < values.size() && j < (size_t)PCV_MAX_BOOST_KNOTS; ++j) b.knot_values[j] = values[j], b.knot_boosts[j] = boosts[j];
        b.unset_boost = unset;
        return b;
    }
};
// One hit of search_vector_boosted: the item, its boosted score m = relevance + boost(value), its value (PCV_NO_VALUE: none) and
// its rank in the list search_vector returns.
struct BoostedItem {
    SearchItem item;
    double boosted;
    int64_t value;
    int32_t rank;
};
// Boosted search on a searcher or a view handle (pcv_searcher_search_boosted): the top num_results under m, ties to the better
// rank; at most `pool` entries of the ranked list are examined (0: the default, min(PCV_MAX_BOOST_POOL, max(128, 8 * num_results))).
// `exact`, if given: the rows are provably the top num_results of the whole list.
inline std::vector<BoostedItem> search_boosted_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                      const std::vector<float>& vector, const Boost& boost, size_t pool, bool* exact) {
    if (exact) *exact = true;
    if (sources.empty() || num_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_BOOST_POOL, std::max<size_t>(128, 8 * num_results));
    const pcv_boost b = boost.raw();
    std::vector<int64_t> ids(num_results), values(num_results);
    std::vector<float> scores(num_results);
    std::vector<double> boosted(num_results);
    std::vector<int32_t> ranks(num_results);
    int32_t count = 0;
    uint8_t e = 0;
    check(pcv_searcher_search_boosted(h, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results, (int)pool, &b, ids.data(),
                                      scores.data(), boosted.data(), values.data(), ranks.data(), &count, nullptr, &e));
    if (exact) *exact = e != 0;
    std::vector<BoostedItem> out;
    for (int i = 0; i < count; ++i) out.push_back({{ids[(size_t)i], scores[(size_t)i]}, boosted[(size_t)i], values[(size_t)i], ranks[(size_t)i]});
    return out;
}

// A compound query (pcv_searcher_search_compound): the rows wanted under ALL or ANY of `want` (1 .. PCV_MAX_COMPOUND_PARTS vectors), less
// a hinge penalty for resembling one of `avoid` (0 .. PCV_MAX_COMPOUND_PARTS vectors).
struct Compound {
    std::vector<std::vector<float>> want, avoid;
};
enum class CompoundMode { All = PCV_COMPOUND_ALL, Any = PCV_COMPOUND_ANY };
// One hit of search_compound: the item's id, m = base - penalty, the score search_vector reports for it under each wanted vector,
// and the penalty.
struct CompoundItem {
    int64_t id;
    double combined;
    std::vector<float> part_scores;
    double penalty;
};
namespace detail {
inline std::vector<CompoundItem> compound_items(size_t parts, int32_t count, const std::vector<int64_t>& ids, const std::vector<double>& combined,
                                                const std::vector<float>& scores, const std::vector<double>& penalties) {
    std::vector<CompoundItem> out;
    for (int i = 0; i < count; ++i) {
        const float* p = scores.data() + (size_t)i * PCV_MAX_COMPOUND_PARTS;
        out.push_back({ids[(size_t)i], combined[(size_t)i], std::vector<float>(p, p + parts), penalties[(size_t)i]});
    }
    return out;
}
}  // namespace detail
// Compound search on a searcher or a view handle: the top num_results under m, ties to the lower position; at most `pool` entries of
// each wanted vector's ranked list are walked (0: the default, min(PCV_MAX_COMPOUND_POOL, max(128, 8 * num_results))).  `exact`, if
// given: the rows are provably the top num_results of all rows.
inline std::vector<CompoundItem> search_compound_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results, const Compound& c,
                                                        CompoundMode mode, float avoid_weight, size_t pool, bool* exact) {
    if (exact) *exact = true;
    if (sources.empty() || num_results == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_COMPOUND_POOL, std::max<size_t>(128, 8 * num_results));
    std::vector<float> want, avoid;
    for (const auto& v : c.want) want.insert(want.end(), v.begin(), v.end());
    for (const auto& v : c.avoid) avoid.insert(avoid.end(), v.begin(), v.end());
    const int64_t want_off[2] = {0, (int64_t)c.want.size()}, avoid_off[2] = {0, (int64_t)c.avoid.size()};
    std::vector<int64_t> ids(num_results);
    std::vector<double> combined(num_results), penalties(num_results);
    std::vector<float> scores(num_results * PCV_MAX_COMPOUND_PARTS);
    int32_t count = 0;
    uint8_t e = 0;
    check(pcv_searcher_search_compound(h, sources.data(), (int)sources.size(), (int)num_results, (int)pool, (int)mode, avoid_weight, want.data(),
                                       want_off, avoid.empty() ? nullptr : avoid.data(), avoid_off, 1, ids.data(), combined.data(), scores.data(),
                                       penalties.data(), &count, nullptr, &e));
    if (exact) *exact = e != 0;
    return detail::compound_items(c.want.size(), count, ids, combined, scores, penalties);
}
// ... with every vector built on the device from stored items (pcv_searcher_search_compound_like): want[p] / avoid[p] are the item ids
// whose rows are summed into part p.  exclude_examples: no row carrying a wanted example id is returned.
inline std::vector<CompoundItem> search_compound_like_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t num_results,
                                                             const std::vector<std::vector<int64_t>>& want, const std::vector<std::vector<int64_t>>& avoid,
                                                             CompoundMode mode, float avoid_weight, size_t pool, bool exclude_examples, bool* exact) {
    if (exact) *exact = true;
    if (sources.empty() || num_results == 0) return {};
    if (pool == 0) pool = std::min<size_t>(PCV_MAX_COMPOUND_POOL, std::max<size_t>(128, 8 * num_results));
    std::vector<int64_t> w_ids, w_ex{0}, a_ids, a_ex{0};
    for (const auto& part : want) w_ids.insert(w_ids.end(), part.begin(), part.end()), w_ex.push_back((int64_t)w_ids.size());
    for (const auto& part : avoid) a_ids.insert(a_ids.end(), part.begin(), part.end()), a_ex.push_back((int64_t)a_ids.size());
    const int64_t want_off[2] = {0, (int64_t)want.size()}, avoid_off[2] = {0, (int64_t)avoid.size()};
    std::vector<int64_t> ids(num_results);
    std::vector<double> combined(num_results), penalties(num_results);
    std::vector<float> scores(num_results * PCV_MAX_COMPOUND_PARTS);
    int32_t count = 0;
    uint8_t e = 0;
    check(pcv_searcher_search_compound_like(h, sources.data(), (int)sources.size(), (int)num_results, (int)pool, (int)mode, avoid_weight,
                                            w_ids.empty() ? nullptr : w_ids.data(), nullptr, w_ex.data(), want_off, a_ids.empty() ? nullptr : a_ids.data(),
                                            nullptr, a_ex.data(), avoid_off, 1, exclude_examples ? 1 : 0, ids.data(), combined.data(), scores.data(),
                                            penalties.data(), &count, nullptr, &e));
    if (exact) *exact = e != 0;
    return detail::compound_items(want.size(), count, ids, combined, scores, penalties);
}

// One duplicate pair of find_duplicates: the item stored first, the other one, their cosine.
struct DuplicatePair {
    int64_t id_a, id_b;
    float score;
};
// Searcher::find_duplicates / SearcherView::find_duplicates (pcv_searcher_find_duplicates): every pair of searchable items whose
// cosine is at or above the threshold, best first, at most max_pairs; `total` receives the exact number of pairs.
inline std::vector<DuplicatePair> find_duplicates_handle(pcv_searcher* h, const std::vector<int64_t>& sources, float threshold, size_t max_pairs,
                                                         int64_t* total) {
    if (total) *total = 0;
    if (sources.empty() || max_pairs == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    max_pairs = std::min<size_t>(max_pairs, PCV_MAX_DUPLICATE_PAIRS);
    std::vector<int64_t> a(max_pairs), b(max_pairs);
    std::vector<float> scores(max_pairs);
    int64_t count = 0;
    check(pcv_searcher_find_duplicates(h, sources.data(), (int)sources.size(), threshold, (int64_t)max_pairs, a.data(), b.data(), scores.data(),
                                       &count, total));
    std::vector<DuplicatePair> out;
    for (int64_t i = 0; i < count; ++i) out.push_back({a[(size_t)i], b[(size_t)i], scores[(size_t)i]});
    return out;
}

// Searcher::assign / kmeans and their SearcherView forms (pcv_searcher_assign, pcv_searcher_kmeans): the exact best of K label
// vectors for every item of `sources`, by global position; label -1 and a NaN score for an item no search could return.
struct Assignment {
    std::vector<int32_t> label;   // [n]
    std::vector<float> score;     // [n] as a search reports it
    std::vector<int64_t> ids;     // [n]
    std::vector<int64_t> counts;  // [K] items per label
};
struct KMeansResult {
    std::vector<float> centroids;  // [K][dim], those the last assignment used
    Assignment last;
    int iterations = 0;            // updates made
    std::vector<int64_t> moved;    // [iterations + 1] items that changed their label in each assignment
};
inline KMeansResult kmeans_handle(pcv_searcher* h, const std::vector<int64_t>& sources, const std::vector<float>& init, size_t k, int max_iters,
                                  bool cosine_kmeans) {
    KMeansResult r;
    r.last.counts.assign(k, 0);
    r.centroids = init;
    if (sources.empty() || k == 0) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    if (cosine_kmeans)
        check(pcv_searcher_kmeans(h, init.data(), (int)k, max_iters, sources.data(), (int)sources.size(), 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, &n));
    else
        check(pcv_searcher_assign(h, init.data(), (int)k, sources.data(), (int)sources.size(), 0, nullptr, nullptr, nullptr, nullptr, &n));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.last.label.resize(room);
    r.last.score.resize(room);
    r.last.ids.resize(room);
    r.moved.assign((size_t)std::max(max_iters, 0) + 1, 0);
    int32_t iters = 0;
    if (cosine_kmeans)
        check(pcv_searcher_kmeans(h, init.data(), (int)k, max_iters, sources.data(), (int)sources.size(), (int64_t)room, r.centroids.data(),
                                  r.last.label.data(), r.last.score.data(), r.last.ids.data(), r.last.counts.data(), &iters, r.moved.data(), &n));
    else
        check(pcv_searcher_assign(h, init.data(), (int)k, sources.data(), (int)sources.size(), (int64_t)room, r.last.label.data(),
                                  r.last.score.data(), r.last.ids.data(), r.last.counts.data(), &n));
    r.last.label.resize((size_t)n);
    r.last.score.resize((size_t)n);
    r.last.ids.resize((size_t)n);
    r.iterations = iters;
    r.moved.resize((size_t)iters + 1);
    return r;
}

// Searcher::assign_top / SearcherView::assign_top (pcv_searcher_assign_top): the exact m best of K label vectors for every item of
// `sources`, by global position, best first; only labels with a score >= min_score (-infinity: no bound) are listed.
struct TopLabels {
    size_t m = 0;
    std::vector<int32_t> labels;      // [n][m], unused slots -1
    std::vector<float> scores;        // [n][m] as a search reports them, unused slots NaN
    std::vector<int64_t> ids;         // [n]
    std::vector<int32_t> counts;      // [n] labels listed for the item
    std::vector<int64_t> label_rows;  // [K] items that list each label
};
inline TopLabels assign_top_handle(pcv_searcher* h, const std::vector<int64_t>& sources, const std::vector<float>& labels, size_t k, size_t m,
                                   float min_score) {
    TopLabels r;
    r.m = m;
    r.label_rows.assign(k, 0);
    if (sources.empty() || k == 0 || m == 0) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    check(pcv_searcher_assign_top(h, labels.data(), (int)k, (int)m, min_score, sources.data(), (int)sources.size(), 0, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, &n));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.labels.resize(room * m);
    r.scores.resize(room * m);
    r.ids.resize(room);
    r.counts.resize(room);
    check(pcv_searcher_assign_top(h, labels.data(), (int)k, (int)m, min_score, sources.data(), (int)sources.size(), (int64_t)room, r.labels.data(),
                                  r.scores.data(), r.ids.data(), r.counts.data(), r.label_rows.data(), &n));
    r.labels.resize((size_t)n * m);
    r.scores.resize((size_t)n * m);
    r.ids.resize((size_t)n);
    r.counts.resize((size_t)n);
    return r;
}

// Searcher::neighbors / SearcherView::neighbors (pcv_searcher_neighbors): for every item of `sources`, by global position, its
// exact k best other items by cosine, best first; an item no search could return has none.
struct NeighborTable {
    size_t k = 0;
    std::vector<int64_t> ids;           // [n]
    std::vector<int64_t> neighbor_ids;  // [n][k], unused slots -1
    std::vector<float> scores;          // [n][k], unused slots NaN
    std::vector<int32_t> counts;        // [n]
};
inline NeighborTable neighbors_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t k) {
    NeighborTable r;
    r.k = k;
    if (sources.empty() || k == 0) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    check(pcv_searcher_neighbors(h, sources.data(), (int)sources.size(), (int)k, 0, nullptr, nullptr, nullptr, nullptr, &n));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.neighbor_ids.resize(room * k);
    r.scores.resize(room * k);
    r.counts.resize(room);
    check(pcv_searcher_neighbors(h, sources.data(), (int)sources.size(), (int)k, (int64_t)room, r.ids.data(), r.neighbor_ids.data(), r.scores.data(),
                                 r.counts.data(), &n));
    r.ids.resize((size_t)n);
    r.neighbor_ids.resize((size_t)n * k);
    r.scores.resize((size_t)n * k);
    r.counts.resize((size_t)n);
    return r;
}

// Searcher::match / SearcherView::match (pcv_searcher_match): for every item of the sources `from`, by global position, its exact k
// best items of the sources `to` by cosine among those with cosine >= min_score (-1: no bound), best first; an item is never its own
// match; with `from` == `to` and no bound the table is the neighbours' (NeighborTable, neighbor_ids: the matches).  An empty `to`
// matches nothing: every count is 0.
inline NeighborTable match_handle(pcv_searcher* h, const std::vector<int64_t>& from, const std::vector<int64_t>& to, size_t k, float min_score) {
    NeighborTable r;
    r.k = k;
    if (from.empty() || k == 0) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    const int64_t none = 0;
    const int64_t* to_ids = to.empty() ? &none : to.data();  // (a NULL list would mean every source)
    check(pcv_searcher_match(h, from.data(), (int)from.size(), to_ids, (int)to.size(), (int)k, min_score, 0, nullptr, nullptr, nullptr, nullptr, &n));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.neighbor_ids.resize(room * k);
    r.scores.resize(room * k);
    r.counts.resize(room);
    check(pcv_searcher_match(h, from.data(), (int)from.size(), to_ids, (int)to.size(), (int)k, min_score, (int64_t)room, r.ids.data(),
                             r.neighbor_ids.data(), r.scores.data(), r.counts.data(), &n));
    r.ids.resize((size_t)n);
    r.neighbor_ids.resize((size_t)n * k);
    r.scores.resize((size_t)n * k);
    r.counts.resize((size_t)n);
    return r;
}

// Searcher::neighbors_grouped / match_grouped / find_duplicates_grouped and their SearcherView forms (pcv_searcher_neighbors_grouped,
// _match_grouped, _find_duplicates_grouped): neighbors, match and find_duplicates with the group table (set_groups) consulted.  flags:
// PCV_GROUPS_SKIP_OWN — the items of the owner's own group are no partners of it; PCV_GROUPS_ONE_PER_GROUP — of every group only its
// best member is kept; both, or 0 for the plain table.  `groups` holds the group of every reported partner, PCV_NO_GROUP for a
// singleton and in unused slots.
struct GroupedNeighborTable {
    NeighborTable table;
    std::vector<int64_t> groups;  // [n][k]
};
inline GroupedNeighborTable neighbors_grouped_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t k, uint32_t flags) {
    GroupedNeighborTable g;
    NeighborTable& r = g.table;
    r.k = k;
    if (sources.empty() || k == 0) return g;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    check(pcv_searcher_neighbors_grouped(h, sources.data(), (int)sources.size(), (int)k, flags, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.neighbor_ids.resize(room * k);
    r.scores.resize(room * k);
    g.groups.resize(room * k);
    r.counts.resize(room);
    check(pcv_searcher_neighbors_grouped(h, sources.data(), (int)sources.size(), (int)k, flags, (int64_t)room, r.ids.data(), r.neighbor_ids.data(),
                                         r.scores.data(), g.groups.data(), r.counts.data(), &n));
    r.ids.resize((size_t)n);
    r.neighbor_ids.resize((size_t)n * k);
    r.scores.resize((size_t)n * k);
    g.groups.resize((size_t)n * k);
    r.counts.resize((size_t)n);
    return g;
}
inline GroupedNeighborTable match_grouped_handle(pcv_searcher* h, const std::vector<int64_t>& from, const std::vector<int64_t>& to, size_t k,
                                                 float min_score, uint32_t flags) {
    GroupedNeighborTable g;
    NeighborTable& r = g.table;
    r.k = k;
    if (from.empty() || k == 0) return g;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    const int64_t none = 0;
    const int64_t* to_ids = to.empty() ? &none : to.data();  // (a NULL list would mean every source)
    check(pcv_searcher_match_grouped(h, from.data(), (int)from.size(), to_ids, (int)to.size(), (int)k, min_score, flags, 0, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, &n));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.neighbor_ids.resize(room * k);
    r.scores.resize(room * k);
    g.groups.resize(room * k);
    r.counts.resize(room);
    check(pcv_searcher_match_grouped(h, from.data(), (int)from.size(), to_ids, (int)to.size(), (int)k, min_score, flags, (int64_t)room, r.ids.data(),
                                     r.neighbor_ids.data(), r.scores.data(), g.groups.data(), r.counts.data(), &n));
    r.ids.resize((size_t)n);
    r.neighbor_ids.resize((size_t)n * k);
    r.scores.resize((size_t)n * k);
    g.groups.resize((size_t)n * k);
    r.counts.resize((size_t)n);
    return g;
}
// total: the pairs of non-siblings; skipped: the sibling pairs at or above the threshold, which find_duplicates would report
inline std::vector<DuplicatePair> find_duplicates_grouped_handle(pcv_searcher* h, const std::vector<int64_t>& sources, float threshold,
                                                                 size_t max_pairs, int64_t* total, int64_t* skipped) {
    if (total) *total = 0;
    if (skipped) *skipped = 0;
    if (sources.empty() || max_pairs == 0) return {};  // `sources.contains(..)` matches nothing; room for nothing
    max_pairs = std::min<size_t>(max_pairs, PCV_MAX_DUPLICATE_PAIRS);
    std::vector<int64_t> a(max_pairs), b(max_pairs);
    std::vector<float> scores(max_pairs);
    int64_t count = 0;
    check(pcv_searcher_find_duplicates_grouped(h, sources.data(), (int)sources.size(), threshold, (int64_t)max_pairs, a.data(), b.data(),
                                               scores.data(), &count, total, skipped));
    std::vector<DuplicatePair> out;
    for (int64_t i = 0; i < count; ++i) out.push_back({a[(size_t)i], b[(size_t)i], scores[(size_t)i]});
    return out;
}

// Searcher::density_clusters / SearcherView::density_clusters (pcv_searcher_density_clusters): DBSCAN under the cosine over the items
// of `sources`, by global position — the clusters, their number and the noise, with no number of groups to choose.
struct DensityClusters {
    std::vector<int64_t> ids;      // [n]
    std::vector<int32_t> labels;   // [n] the cluster; -1: noise, or the item takes no part
    std::vector<int8_t> kinds;     // [n] PCV_DENSITY_CORE, _BORDER, _NOISE or _NONE
    std::vector<int32_t> degrees;  // [n] the other items within the threshold
    int32_t clusters = 0;
};
inline DensityClusters density_clusters_handle(pcv_searcher* h, const std::vector<int64_t>& sources, float threshold, int min_items) {
    DensityClusters r;
    if (sources.empty()) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    check(pcv_searcher_density_clusters(h, sources.data(), (int)sources.size(), threshold, min_items, 0, nullptr, nullptr, nullptr, nullptr, &n, nullptr));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.labels.resize(room);
    r.kinds.resize(room);
    r.degrees.resize(room);
    check(pcv_searcher_density_clusters(h, sources.data(), (int)sources.size(), threshold, min_items, (int64_t)room, r.ids.data(), r.labels.data(),
                                        r.kinds.data(), r.degrees.data(), &n, &r.clusters));
    r.ids.resize((size_t)n);
    r.labels.resize((size_t)n);
    r.kinds.resize((size_t)n);
    r.degrees.resize((size_t)n);
    return r;
}

// Searcher::linkage_tree / SearcherView::linkage_tree (pcv_searcher_linkage_tree): the single-linkage hierarchy of the items of
// `sources` — their maximum spanning tree under the cosine, edges from best to worst — and linkage_cut, which cuts it (host only).
struct LinkageTree {
    std::vector<int64_t> ids;    // [n] by global position
    std::vector<int8_t> part;    // [n] 1 iff the item takes part
    std::vector<int64_t> pos_a;  // [e] positions into ids, pos_a < pos_b; e = participating items - 1 (or 0)
    std::vector<int64_t> pos_b;  // [e]
    std::vector<int64_t> id_a;   // [e]
    std::vector<int64_t> id_b;   // [e]
    std::vector<double> c;       // [e] the canonical cosine, descending
};
inline LinkageTree linkage_tree_handle(pcv_searcher* h, const std::vector<int64_t>& sources) {
    LinkageTree r;
    if (sources.empty()) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0, e = 0;
    check(pcv_searcher_linkage_tree(h, sources.data(), (int)sources.size(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, nullptr));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.part.resize(room);
    r.pos_a.resize(room);
    r.pos_b.resize(room);
    r.id_a.resize(room);
    r.id_b.resize(room);
    r.c.resize(room);
    check(pcv_searcher_linkage_tree(h, sources.data(), (int)sources.size(), (int64_t)room, r.ids.data(), r.part.data(), r.pos_a.data(), r.pos_b.data(),
                                    r.id_a.data(), r.id_b.data(), r.c.data(), &n, &e));
    r.ids.resize((size_t)n);
    r.part.resize((size_t)n);
    r.pos_a.resize((size_t)e);
    r.pos_b.resize((size_t)e);
    r.id_a.resize((size_t)e);
    r.id_b.resize((size_t)e);
    r.c.resize((size_t)e);
    return r;
}
struct LinkageCut {
    std::vector<int32_t> labels;  // [n] the cluster, numbered by its lowest position; -1: the item takes no part
    int32_t clusters = 0;
};
// edge i is kept iff c[i] >= threshold and i < e - (min_clusters - 1): a threshold alone gives the components of the graph c >= t
// (density_clusters with min_items 1), min_clusters K with threshold -infinity gives K clusters
inline LinkageCut linkage_cut(const LinkageTree& t, double threshold, int64_t min_clusters = 1) {
    LinkageCut r;
    r.labels.resize(std::max<size_t>(t.ids.size(), 1));
    check(pcv_linkage_cut(t.pos_a.data(), t.pos_b.data(), t.c.data(), (int64_t)t.c.size(), t.part.empty() ? nullptr : t.part.data(), (int64_t)t.ids.size(),
                          threshold, min_clusters, r.labels.data(), &r.clusters));
    r.labels.resize(t.ids.size());
    return r;
}

// Searcher::reach_tree / SearcherView::reach_tree (pcv_searcher_reach_tree): the spanning tree under the mutual-reachability weight
// w = min(core(a), core(b), c(a, b)), core the (min_items - 1)-th largest cosine of an item with another — what HDBSCAN starts from —
// and linkage_select, which picks clusters from it (or from a LinkageTree) without a threshold (host only).
struct ReachTree {
    std::vector<int64_t> ids;    // [n] by global position
    std::vector<int8_t> part;    // [n] 1 iff the item takes part
    std::vector<double> core;    // [n] the core score, +inf for min_items 1, NaN where part is 0
    std::vector<int64_t> pos_a;  // [e] positions into ids, pos_a < pos_b; e = participating items - 1 (or 0)
    std::vector<int64_t> pos_b;  // [e]
    std::vector<int64_t> id_a;   // [e]
    std::vector<int64_t> id_b;   // [e]
    std::vector<double> w;       // [e] the weight, descending
    std::vector<double> c;       // [e] the canonical cosine of the edge
};
inline ReachTree reach_tree_handle(pcv_searcher* h, const std::vector<int64_t>& sources, int min_items) {
    ReachTree r;
    if (sources.empty()) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0, e = 0;
    check(pcv_searcher_reach_tree(h, sources.data(), (int)sources.size(), min_items, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, &n, nullptr));
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    r.ids.resize(room);
    r.part.resize(room);
    r.core.resize(room);
    r.pos_a.resize(room);
    r.pos_b.resize(room);
    r.id_a.resize(room);
    r.id_b.resize(room);
    r.w.resize(room);
    r.c.resize(room);
    check(pcv_searcher_reach_tree(h, sources.data(), (int)sources.size(), min_items, (int64_t)room, r.ids.data(), r.part.data(), r.core.data(),
                                  r.pos_a.data(), r.pos_b.data(), r.id_a.data(), r.id_b.data(), r.w.data(), r.c.data(), &n, &e));
    r.ids.resize((size_t)n);
    r.part.resize((size_t)n);
    r.core.resize((size_t)n);
    r.pos_a.resize((size_t)e);
    r.pos_b.resize((size_t)e);
    r.id_a.resize((size_t)e);
    r.id_b.resize((size_t)e);
    r.w.resize((size_t)e);
    r.c.resize((size_t)e);
    return r;
}
struct LinkageSelection {
    std::vector<int32_t> labels;    // [n] the selected cluster, numbered by its lowest position; -1: noise, or the item takes no part
    std::vector<double> stability;  // [clusters]
    std::vector<int64_t> size;      // [clusters] items labelled with it
};
inline LinkageSelection linkage_select(const std::vector<int64_t>& pos_a, const std::vector<int64_t>& pos_b, const std::vector<double>& w,
                                       const std::vector<int8_t>& part, int64_t min_cluster_size, bool allow_single = false) {
    LinkageSelection r;
    const size_t n = part.size();
    const size_t room = std::max<size_t>(n / (size_t)std::max<int64_t>(min_cluster_size, 2), 1);
    int32_t clusters = 0;
    r.labels.resize(std::max<size_t>(n, 1));
    r.stability.resize(room);
    r.size.resize(room);
    check(pcv_linkage_select(pos_a.data(), pos_b.data(), w.data(), (int64_t)w.size(), part.empty() ? nullptr : part.data(), (int64_t)n, min_cluster_size,
                             allow_single ? 1 : 0, r.labels.data(), &clusters, r.stability.data(), r.size.data(), (int64_t)room));
    r.labels.resize(n);
    r.stability.resize((size_t)clusters);
    r.size.resize((size_t)clusters);
    return r;
}
inline LinkageSelection linkage_select(const ReachTree& t, int64_t min_cluster_size, bool allow_single = false) {
    return linkage_select(t.pos_a, t.pos_b, t.w, t.part, min_cluster_size, allow_single);
}
inline LinkageSelection linkage_select(const LinkageTree& t, int64_t min_cluster_size, bool allow_single = false) {
    return linkage_select(t.pos_a, t.pos_b, t.c, t.part, min_cluster_size, allow_single);
}

// Searcher::seeds / SearcherView::seeds (pcv_searcher_seeds): up to k items that cover `sources`, in the order they were picked —
// the init of kmeans (k-means++), or a representative sample with its covering radii (farthest first).
enum class SeedMethod { Farthest = PCV_SEED_FARTHEST, KMeansPP = PCV_SEED_KMEANSPP };
struct SeedItems {
    std::vector<int64_t> ids;        // [n], n <= k: the picks stop when no row is left uncovered
    std::vector<int64_t> positions;  // [n] global positions
    std::vector<int64_t> totals;     // [n] the potential before each pick, in units of 2^-32
    std::vector<float> cover;        // [n] the pick's largest cosine with the seeds before it; NaN at step 0
};
inline SeedItems seeds_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t k, SeedMethod method, uint64_t seed,
                              std::optional<int64_t> first_id) {
    SeedItems r;
    if (sources.empty() || k == 0) return r;  // `sources.contains(..)` matches nothing
    r.ids.resize(k);
    r.positions.resize(k);
    r.totals.resize(k);
    r.cover.resize(k);
    int32_t n = 0;
    const int64_t first = first_id.value_or(0);
    check(pcv_searcher_seeds(h, sources.data(), (int)sources.size(), (int)k, (int)method, seed, first_id ? &first : nullptr, r.ids.data(),
                             r.positions.data(), r.totals.data(), r.cover.data(), &n));
    r.ids.resize((size_t)n);
    r.positions.resize((size_t)n);
    r.totals.resize((size_t)n);
    r.cover.resize((size_t)n);
    return r;
}

// Searcher::moments / principal_axes / project (pcv_searcher_moments, _principal_axes, _project): a PCA where the rows live.
struct Moments {
    int64_t n = 0;                // participating rows
    std::vector<int64_t> sums;    // [dim] S_d, the sums of the fixed-point unit rows
    std::vector<double> matrix;   // [dim][dim] C * 2^-64, or centered (n C - S S^T) * 2^-64; empty when not asked for
};
struct PrincipalAxes {
    int64_t n = 0;
    std::vector<float> axes;       // [m][dim]
    std::vector<double> offsets;   // [m] the mean unit row along each axis
    std::vector<double> variance;  // [m]
};
struct Projection {
    std::vector<float> coords;  // [n][m]; NaN for a row that takes no part
    std::vector<int64_t> ids;   // [n]
};
inline size_t dim_of_handle(pcv_searcher* h) {
    int dim = 0;
    check(pcv_searcher_dim(h, &dim));
    return (size_t)dim;
}
inline Moments moments_handle(pcv_searcher* h, const std::vector<int64_t>& sources, bool centered, bool matrix) {
    Moments r;
    const size_t dim = dim_of_handle(h);
    r.sums.assign(dim, 0);
    if (matrix) r.matrix.assign(dim * dim, 0.0);
    if (sources.empty()) return r;  // `sources.contains(..)` matches nothing
    check(pcv_searcher_moments(h, sources.data(), (int)sources.size(), centered ? 1 : 0, r.sums.data(), matrix ? r.matrix.data() : nullptr, &r.n));
    return r;
}
inline PrincipalAxes principal_axes_handle(pcv_searcher* h, const std::vector<int64_t>& sources, size_t m) {
    PrincipalAxes r;
    const size_t dim = dim_of_handle(h);
    r.axes.assign(m * dim, 0.0f);
    r.offsets.assign(m, 0.0);
    r.variance.assign(m, 0.0);
    if (sources.empty()) throw Error(PCV_ERR_INVALID, "principal_axes: no source selected");
    check(pcv_searcher_principal_axes(h, sources.data(), (int)sources.size(), (int)m, r.axes.data(), r.offsets.data(), r.variance.data(), &r.n));
    return r;
}
inline Projection project_handle(pcv_searcher* h, const std::vector<int64_t>& sources, const std::vector<float>& axes, size_t m,
                                 const std::vector<double>* offsets) {
    Projection r;
    if (axes.size() != m * dim_of_handle(h) || (offsets && offsets->size() != m)) throw Error(PCV_ERR_INVALID, "project: axes must be [m][dim], offsets [m]");
    if (sources.empty()) return r;  // `sources.contains(..)` matches nothing
    int64_t n = 0;
    const double* off = offsets ? offsets->data() : nullptr;
    check(pcv_searcher_project(h, axes.data(), off, (int)m, sources.data(), (int)sources.size(), 0, nullptr, nullptr, &n));
    r.coords.resize((size_t)std::max<int64_t>(n, 1) * m);
    r.ids.resize((size_t)std::max<int64_t>(n, 1));
    check(pcv_searcher_project(h, axes.data(), off, (int)m, sources.data(), (int)sources.size(), std::max<int64_t>(n, 1), r.coords.data(), r.ids.data(), &n));
    r.coords.resize((size_t)n * m);
    r.ids.resize((size_t)n);
    return r;
}
// pcv_symmetric_eigen (host only, offline): values descending, vectors[i] the unit eigenvector of values[i]
struct Eigen {
    std::vector<double> values, vectors;
};
inline Eigen symmetric_eigen(const std::vector<double>& a, size_t n) {
    Eigen r;
    if (a.size() != n * n) throw Error(PCV_ERR_INVALID, "symmetric_eigen: a must be [n][n]");
    r.values.assign(n, 0.0);
    r.vectors.assign(n * n, 0.0);
    check(pcv_symmetric_eigen(a.data(), (int)n, r.values.data(), r.vectors.data()));
    return r;
}

// Searcher::view: a read-only searcher over the rows carrying one of a set of item ids (pcv_searcher_create_view).  It searches
// like a searcher built from only those rows and follows every later change of its parent; it must go before its parent does.
class SearcherView {
public:
    SearcherView(pcv_searcher* parent, const std::vector<int64_t>& ids) {
        check(pcv_searcher_create_view(parent, ids.data(), (int64_t)ids.size(), &h_));
    }
    // Searcher::view_where: the rows whose id passes the predicate, selected on the device (pcv_searcher_create_view_where)
    SearcherView(pcv_searcher* parent, const Where& where) { check(pcv_searcher_create_view_where(parent, where.lo, where.hi, where.flags(), &h_)); }
    ~SearcherView() {
        if (h_) pcv_searcher_destroy(h_);
    }
    SearcherView(SearcherView&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    SearcherView& operator=(SearcherView&& o) noexcept {
        if (this != &o) {
            if (h_) pcv_searcher_destroy(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    SearcherView(const SearcherView&) = delete;
    SearcherView& operator=(const SearcherView&) = delete;

    // Searcher::search_vector among the view's items
    std::vector<SearchItem> search_vector(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector) const {
        if (sources.empty()) return {};
        std::vector<int64_t> ids(num_results);
        std::vector<float> scores(num_results);
        int count = 0;
        check(pcv_searcher_search(h_, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results, ids.data(), scores.data(),
                                  &count));
        std::vector<SearchItem> out;
        for (int i = 0; i < count; ++i) out.push_back({ids[i], scores[i]});
        return out;
    }
    // every item of the view within a score bound (search_range_handle)
    std::vector<SearchItem> search_range(const std::vector<int64_t>& sources, float bound, size_t max_results, const std::vector<float>& vector,
                                         bool* more = nullptr) const {
        return search_range_handle(h_, sources, bound, max_results, vector, more);
    }
    // the view's best items with near-duplicates collapsed (search_distinct_handle)
    std::vector<SearchItem> search_vector_distinct(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   float threshold, size_t pool = 0, std::vector<int32_t>* similar = nullptr) const {
        return search_distinct_handle(h_, sources, num_results, vector, threshold, pool, similar);
    }
    // a diverse set of the view's best items: greedy MMR on the device (search_diverse_handle)
    std::vector<DiverseItem> search_vector_diverse(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   float lambda, size_t pool = 0, bool* exact = nullptr) const {
        return search_diverse_handle(h_, sources, num_results, vector, lambda, pool, exact);
    }
    // the view's best groups, one item each, by the parent's group table (search_grouped_handle)
    std::vector<GroupedItem> search_vector_grouped(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   size_t pool = 0, bool* more = nullptr) const {
        return search_grouped_handle(h_, sources, num_results, vector, pool, more);
    }
    // the view's best items that pass a predicate on the parent's values (search_where_handle), and how many pass at all
    std::vector<ValuedItem> search_vector_where(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                const Where& where, size_t pool = 0, bool* more = nullptr) const {
        return search_where_handle(h_, sources, num_results, vector, where, pool, more);
    }
    int64_t count_where(const std::vector<int64_t>& sources, const Where& where, int64_t* searchable = nullptr) const {
        return count_where_handle(h_, sources, where, searchable);
    }
    // the view's best items under score plus a boost from the parent's values (search_boosted_handle)
    std::vector<BoostedItem> search_vector_boosted(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   const Boost& boost, size_t pool = 0, bool* exact = nullptr) const {
        return search_boosted_handle(h_, sources, num_results, vector, boost, pool, exact);
    }
    // the view's best items under all / any of several vectors, less a penalty for resembling others (search_compound_handle)
    std::vector<CompoundItem> search_compound(const std::vector<int64_t>& sources, size_t num_results, const Compound& compound,
                                              CompoundMode mode = CompoundMode::All, float avoid_weight = 1.0f, size_t pool = 0,
                                              bool* exact = nullptr) const {
        return search_compound_handle(h_, sources, num_results, compound, mode, avoid_weight, pool, exact);
    }
    std::vector<CompoundItem> search_compound_like_items(const std::vector<int64_t>& sources, size_t num_results,
                                                         const std::vector<std::vector<int64_t>>& want,
                                                         const std::vector<std::vector<int64_t>>& avoid = {}, CompoundMode mode = CompoundMode::All,
                                                         float avoid_weight = 1.0f, size_t pool = 0, bool exclude_examples = true,
                                                         bool* exact = nullptr) const {
        return search_compound_like_handle(h_, sources, num_results, want, avoid, mode, avoid_weight, pool, exclude_examples, exact);
    }
    // the duplicate pairs among the view's items (find_duplicates_handle)
    std::vector<DuplicatePair> find_duplicates(const std::vector<int64_t>& sources, float threshold, size_t max_pairs = 1 << 20,
                                               int64_t* total = nullptr) const {
        return find_duplicates_handle(h_, sources, threshold, max_pairs, total);
    }
    // the best of the k label vectors `labels` [k][dim] for every item (kmeans_handle)
    Assignment assign(const std::vector<int64_t>& sources, const std::vector<float>& labels, size_t k) const {
        return kmeans_handle(h_, sources, labels, k, 0, false).last;
    }
    // spherical k-means by cosine from `init` [k][dim], at most max_iters updates (kmeans_handle)
    KMeansResult kmeans(const std::vector<int64_t>& sources, const std::vector<float>& init, size_t k, int max_iters = 20) const {
        return kmeans_handle(h_, sources, init, k, max_iters, true);
    }
    pcv_assign_stats last_assign_stats() const {
        pcv_assign_stats st;
        check(pcv_searcher_last_assign_stats(h_, &st));
        return st;
    }
    // the m best of the k label vectors `labels` [k][dim] for every item, with a score bound (assign_top_handle)
    TopLabels assign_top(const std::vector<int64_t>& sources, const std::vector<float>& labels, size_t k, size_t m,
                         float min_score = -std::numeric_limits<float>::infinity()) const {
        return assign_top_handle(h_, sources, labels, k, m, min_score);
    }
    pcv_assign_top_stats last_assign_top_stats() const {
        pcv_assign_top_stats st;
        check(pcv_searcher_last_assign_top_stats(h_, &st));
        return st;
    }
    // up to k seed items of the view (seeds_handle)
    SeedItems seeds(const std::vector<int64_t>& sources, size_t k, SeedMethod method = SeedMethod::KMeansPP, uint64_t seed = 0,
                    std::optional<int64_t> first_id = std::nullopt) const {
        return seeds_handle(h_, sources, k, method, seed, first_id);
    }
    pcv_seed_stats last_seed_stats() const {
        pcv_seed_stats st;
        check(pcv_searcher_last_seed_stats(h_, &st));
        return st;
    }
    // integer moments of the unit rows, their principal axes, and every row's coordinates along given axes (moments_handle, ...)
    Moments moments(const std::vector<int64_t>& sources, bool centered = false, bool matrix = true) const {
        return moments_handle(h_, sources, centered, matrix);
    }
    PrincipalAxes principal_axes(const std::vector<int64_t>& sources, size_t m) const { return principal_axes_handle(h_, sources, m); }
    Projection project(const std::vector<int64_t>& sources, const std::vector<float>& axes, size_t m, const std::vector<double>* offsets = nullptr) const {
        return project_handle(h_, sources, axes, m, offsets);
    }
    pcv_moment_stats last_moment_stats() const {
        pcv_moment_stats st;
        check(pcv_searcher_last_moment_stats(h_, &st));
        return st;
    }
    pcv_project_stats last_project_stats() const {
        pcv_project_stats st;
        check(pcv_searcher_last_project_stats(h_, &st));
        return st;
    }
    // density clusters of the view's items (density_clusters_handle)
    DensityClusters density_clusters(const std::vector<int64_t>& sources, float threshold, int min_items) const {
        return density_clusters_handle(h_, sources, threshold, min_items);
    }
    pcv_density_stats last_density_stats() const {
        pcv_density_stats st;
        check(pcv_searcher_last_density_stats(h_, &st));
        return st;
    }
    // the linkage tree of the view's items (linkage_tree_handle)
    LinkageTree linkage_tree(const std::vector<int64_t>& sources) const { return linkage_tree_handle(h_, sources); }
    pcv_linkage_stats last_linkage_stats() const {
        pcv_linkage_stats st;
        check(pcv_searcher_last_linkage_stats(h_, &st));
        return st;
    }
    // the reach tree of the view's items (reach_tree_handle)
    ReachTree reach_tree(const std::vector<int64_t>& sources, int min_items) const { return reach_tree_handle(h_, sources, min_items); }
    pcv_reach_stats last_reach_stats() const {
        pcv_reach_stats st;
        check(pcv_searcher_last_reach_stats(h_, &st));
        return st;
    }
    // the k nearest other items of every item of the view (neighbors_handle)
    NeighborTable neighbors(const std::vector<int64_t>& sources, size_t k) const { return neighbors_handle(h_, sources, k); }
    pcv_neighbor_stats last_neighbor_stats() const {
        pcv_neighbor_stats st;
        check(pcv_searcher_last_neighbor_stats(h_, &st));
        return st;
    }
    // the k best items of the sources `to` for every item of the sources `from` (match_handle)
    NeighborTable match(const std::vector<int64_t>& from, const std::vector<int64_t>& to, size_t k, float min_score = -1.0f) const {
        return match_handle(h_, from, to, k, min_score);
    }
    pcv_match_stats last_match_stats() const {
        pcv_match_stats st;
        check(pcv_searcher_last_match_stats(h_, &st));
        return st;
    }
    // neighbors, match and find_duplicates with the group table consulted (neighbors_grouped_handle, ...)
    GroupedNeighborTable neighbors_grouped(const std::vector<int64_t>& sources, size_t k, uint32_t flags = PCV_GROUPS_SKIP_OWN) const {
        return neighbors_grouped_handle(h_, sources, k, flags);
    }
    GroupedNeighborTable match_grouped(const std::vector<int64_t>& from, const std::vector<int64_t>& to, size_t k, float min_score = -1.0f,
                                       uint32_t flags = PCV_GROUPS_SKIP_OWN) const {
        return match_grouped_handle(h_, from, to, k, min_score, flags);
    }
    std::vector<DuplicatePair> find_duplicates_grouped(const std::vector<int64_t>& sources, float threshold, size_t max_pairs = 1 << 20,
                                                       int64_t* total = nullptr, int64_t* skipped = nullptr) const {
        return find_duplicates_grouped_handle(h_, sources, threshold, max_pairs, total, skipped);
    }
    pcv_pair_group_stats last_pair_group_stats() const {
        pcv_pair_group_stats st;
        check(pcv_searcher_last_pair_group_stats(h_, &st));
        return st;
    }
    // search by example among the view's items; the example is looked up in the parent (it need not be an allowed item)
    std::optional<std::vector<SearchItem>> search_like(const std::vector<int64_t>& sources, size_t num_results, int64_t item_id,
                                                       bool exclude = false) const {
        return search_like_handle(h_, sources, num_results, item_id, exclude);
    }
    int64_t num_rows() const {
        int64_t n = 0;
        check(pcv_searcher_num_rows(h_, &n));
        return n;
    }
    // copies of the parent's rows made since the view was created (one per parent change that a call of the view came after)
    int refreshes() const {
        int32_t r = 0;
        check(pcv_searcher_view_stats(h_, nullptr, nullptr, &r, nullptr));
        return r;
    }
    pcv_scan_stats last_stats() const {
        pcv_scan_stats st;
        check(pcv_searcher_last_stats(h_, &st));
        return st;
    }
    pcv_searcher* handle() const { return h_; }

private:
    pcv_searcher* h_ = nullptr;
};

// search.rs:29-260.  Metric::Dot reproduces the reference Searcher's scores exactly
// (max(0, 1 - dot/len), ascending); Metric::Cosine is lib.rs:67-77.
class Searcher {
public:
    std::unordered_set<int64_t> hidden;  // search.rs:31-34 (kept; search_vector does not consult it — hide_items keeps it in step)

    Searcher(Context& ctx, int dim, Metric metric = Metric::Dot) : dim_(dim) {
        check(pcv_searcher_create(ctx.handle(), dim, (int)metric, &h_));
    }
    ~Searcher() { pcv_searcher_destroy(h_); }
    Searcher(const Searcher&) = delete;
    Searcher& operator=(const Searcher&) = delete;

    // Searcher::build (search.rs:38-56) with the Database replaced by its row stream
    template <class Rows>
    static std::unique_ptr<Searcher> build(Context& ctx, const Rows& rows, int dim, Metric metric = Metric::Dot) {
        auto s = std::make_unique<Searcher>(ctx, dim, metric);
        for (const EmbeddingRow& r : rows) s->insert(r);
        check(pcv_searcher_finalize(s->h_));
        return s;
    }
    // Searcher::rebuild_source (search.rs:58-79)
    template <class Rows>
    void rebuild_source(const Rows& rows, int64_t source_id) {
        // the new index is built first and swapped in only once it exists (search.rs:57-79): staged under
        // PCV_STAGING_SOURCE, so a bad row leaves the source's old rows in place
        check(pcv_searcher_clear_source(h_, PCV_STAGING_SOURCE));
        try {
            for (const EmbeddingRow& r : rows)
                if (r.source_id == source_id) insert(r, PCV_STAGING_SOURCE);  // search.rs:106-109
            check(pcv_searcher_finalize(h_));
        } catch (...) {
            pcv_searcher_clear_source(h_, PCV_STAGING_SOURCE);
            pcv_searcher_finalize(h_);
            throw;
        }
        check(pcv_searcher_replace_source(h_, PCV_STAGING_SOURCE, source_id));
        check(pcv_searcher_finalize(h_));
    }
    // Searcher::search_vector (search.rs:157-182)
    std::vector<SearchItem> search_vector(const std::vector<int64_t>& sources, size_t num_results,
                                          const std::vector<float>& vector) const {
        if (sources.empty()) return {};  // `sources.contains(..)` matches nothing
        std::vector<int64_t> ids(num_results);
        std::vector<float> scores(num_results);
        int count = 0;
        check(pcv_searcher_search(h_, vector.data(), 1, sources.data(), (int)sources.size(), (int)num_results,
                                  ids.data(), scores.data(), &count));
        std::vector<SearchItem> out;
        for (int i = 0; i < count; ++i) out.push_back({ids[i], scores[i]});
        return out;
    }
    // every item within a score bound instead of the best k (search_range_handle)
    std::vector<SearchItem> search_range(const std::vector<int64_t>& sources, float bound, size_t max_results, const std::vector<float>& vector,
                                         bool* more = nullptr) const {
        return search_range_handle(h_, sources, bound, max_results, vector, more);
    }
    // the best items with near-duplicates collapsed on the device (search_distinct_handle)
    std::vector<SearchItem> search_vector_distinct(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   float threshold, size_t pool = 0, std::vector<int32_t>* similar = nullptr) const {
        return search_distinct_handle(h_, sources, num_results, vector, threshold, pool, similar);
    }
    // a diverse set of the best items: greedy MMR on the device (search_diverse_handle)
    std::vector<DiverseItem> search_vector_diverse(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   float lambda, size_t pool = 0, bool* exact = nullptr) const {
        return search_diverse_handle(h_, sources, num_results, vector, lambda, pool, exact);
    }
    // the group table (pcv_searcher_set_groups): item ids[i] belongs to group groups[i] (>= 0; PCV_NO_GROUP ungroups); the last
    // occurrence of an id holds.  Keyed by id: it survives remove_items and rebuild_source.
    void set_groups(const std::vector<int64_t>& ids, const std::vector<int64_t>& groups) {
        if (ids.size() != groups.size()) throw std::invalid_argument("set_groups: ids and groups differ in length");
        check(pcv_searcher_set_groups(h_, ids.data(), groups.data(), (int64_t)ids.size()));
    }
    void clear_groups() { check(pcv_searcher_clear_groups(h_)); }
    // the group of every id, PCV_NO_GROUP where it has none
    std::vector<int64_t> groups_of(const std::vector<int64_t>& ids) const {
        std::vector<int64_t> out(ids.size(), PCV_NO_GROUP);
        check(pcv_searcher_get_groups(h_, ids.data(), (int64_t)ids.size(), out.data()));
        return out;
    }
    // the best groups, one item each: "the k closest documents" over chunk rows (search_grouped_handle)
    std::vector<GroupedItem> search_vector_grouped(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   size_t pool = 0, bool* more = nullptr) const {
        return search_grouped_handle(h_, sources, num_results, vector, pool, more);
    }
    // the value table (pcv_searcher_set_values): item ids[i] has value values[i] (any int64; PCV_NO_VALUE unsets); the last occurrence
    // of an id holds.  Keyed by id: it survives remove_items and rebuild_source.
    void set_values(const std::vector<int64_t>& ids, const std::vector<int64_t>& values) {
        if (ids.size() != values.size()) throw std::invalid_argument("set_values: ids and values differ in length");
        check(pcv_searcher_set_values(h_, ids.data(), values.data(), (int64_t)ids.size()));
    }
    void clear_values() { check(pcv_searcher_clear_values(h_)); }
    // the value of every id, PCV_NO_VALUE where it has none
    std::vector<int64_t> values_of(const std::vector<int64_t>& ids) const {
        std::vector<int64_t> out(ids.size(), PCV_NO_VALUE);
        check(pcv_searcher_get_values(h_, ids.data(), (int64_t)ids.size(), out.data()));
        return out;
    }
    pcv_value_stats value_stats() const {
        pcv_value_stats st;
        check(pcv_searcher_value_stats(h_, &st));
        return st;
    }
    // the best items that pass a predicate on their value: "the best matches among the items modified since ..." (search_where_handle)
    std::vector<ValuedItem> search_vector_where(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                const Where& where, size_t pool = 0, bool* more = nullptr) const {
        return search_where_handle(h_, sources, num_results, vector, where, pool, more);
    }
    int64_t count_where(const std::vector<int64_t>& sources, const Where& where, int64_t* searchable = nullptr) const {
        return count_where_handle(h_, sources, where, searchable);
    }
    // the best items under score plus a boost from their value: "the best matches, recent items a little higher" (search_boosted_handle)
    std::vector<BoostedItem> search_vector_boosted(const std::vector<int64_t>& sources, size_t num_results, const std::vector<float>& vector,
                                                   const Boost& boost, size_t pool = 0, bool* exact = nullptr) const {
        return search_boosted_handle(h_, sources, num_results, vector, boost, pool, exact);
    }
    // the best items under all / any of several vectors, less a penalty for resembling others (search_compound_handle)
    std::vector<CompoundItem> search_compound(const std::vector<int64_t>& sources, size_t num_results, const Compound& compound,
                                              CompoundMode mode = CompoundMode::All, float avoid_weight = 1.0f, size_t pool = 0,
                                              bool* exact = nullptr) const {
        return search_compound_handle(h_, sources, num_results, compound, mode, avoid_weight, pool, exact);
    }
    std::vector<CompoundItem> search_compound_like_items(const std::vector<int64_t>& sources, size_t num_results,
                                                         const std::vector<std::vector<int64_t>>& want,
                                                         const std::vector<std::vector<int64_t>>& avoid = {}, CompoundMode mode = CompoundMode::All,
                                                         float avoid_weight = 1.0f, size_t pool = 0, bool exclude_examples = true,
                                                         bool* exact = nullptr) const {
        return search_compound_like_handle(h_, sources, num_results, want, avoid, mode, avoid_weight, pool, exclude_examples, exact);
    }
    // every pair of near-duplicate items, found once on the device (find_duplicates_handle)
    std::vector<DuplicatePair> find_duplicates(const std::vector<int64_t>& sources, float threshold, size_t max_pairs = 1 << 20,
                                               int64_t* total = nullptr) const {
        return find_duplicates_handle(h_, sources, threshold, max_pairs, total);
    }
    // the best of the k label vectors `labels` [k][dim] for every item (kmeans_handle)
    Assignment assign(const std::vector<int64_t>& sources, const std::vector<float>& labels, size_t k) const {
        return kmeans_handle(h_, sources, labels, k, 0, false).last;
    }
    // spherical k-means by cosine from `init` [k][dim], at most max_iters updates (kmeans_handle)
    KMeansResult kmeans(const std::vector<int64_t>& sources, const std::vector<float>& init, size_t k, int max_iters = 20) const {
        return kmeans_handle(h_, sources, init, k, max_iters, true);
    }
    pcv_assign_stats last_assign_stats() const {
        pcv_assign_stats st;
        check(pcv_searcher_last_assign_stats(h_, &st));
        return st;
    }
    // the m best of the k label vectors `labels` [k][dim] for every item, with a score bound (assign_top_handle)
    TopLabels assign_top(const std::vector<int64_t>& sources, const std::vector<float>& labels, size_t k, size_t m,
                         float min_score = -std::numeric_limits<float>::infinity()) const {
        return assign_top_handle(h_, sources, labels, k, m, min_score);
    }
    pcv_assign_top_stats last_assign_top_stats() const {
        pcv_assign_top_stats st;
        check(pcv_searcher_last_assign_top_stats(h_, &st));
        return st;
    }
    // up to k seed items, picked on the device (seeds_handle)
    SeedItems seeds(const std::vector<int64_t>& sources, size_t k, SeedMethod method = SeedMethod::KMeansPP, uint64_t seed = 0,
                    std::optional<int64_t> first_id = std::nullopt) const {
        return seeds_handle(h_, sources, k, method, seed, first_id);
    }
    pcv_seed_stats last_seed_stats() const {
        pcv_seed_stats st;
        check(pcv_searcher_last_seed_stats(h_, &st));
        return st;
    }
    // integer moments of the unit rows, their principal axes, and every row's coordinates along given axes (moments_handle, ...)
    Moments moments(const std::vector<int64_t>& sources, bool centered = false, bool matrix = true) const {
        return moments_handle(h_, sources, centered, matrix);
    }
    PrincipalAxes principal_axes(const std::vector<int64_t>& sources, size_t m) const { return principal_axes_handle(h_, sources, m); }
    Projection project(const std::vector<int64_t>& sources, const std::vector<float>& axes, size_t m, const std::vector<double>* offsets = nullptr) const {
        return project_handle(h_, sources, axes, m, offsets);
    }
    pcv_moment_stats last_moment_stats() const {
        pcv_moment_stats st;
        check(pcv_searcher_last_moment_stats(h_, &st));
        return st;
    }
    pcv_project_stats last_project_stats() const {
        pcv_project_stats st;
        check(pcv_searcher_last_project_stats(h_, &st));
        return st;
    }
    // density clusters (DBSCAN under the cosine) of the items, found on the device (density_clusters_handle)
    DensityClusters density_clusters(const std::vector<int64_t>& sources, float threshold, int min_items) const {
        return density_clusters_handle(h_, sources, threshold, min_items);
    }
    pcv_density_stats last_density_stats() const {
        pcv_density_stats st;
        check(pcv_searcher_last_density_stats(h_, &st));
        return st;
    }
    // the single-linkage hierarchy of the items, built on the device (linkage_tree_handle); linkage_cut cuts it
    LinkageTree linkage_tree(const std::vector<int64_t>& sources) const { return linkage_tree_handle(h_, sources); }
    pcv_linkage_stats last_linkage_stats() const {
        pcv_linkage_stats st;
        check(pcv_searcher_last_linkage_stats(h_, &st));
        return st;
    }
    // the spanning tree under the mutual-reachability weight, built on the device (reach_tree_handle); linkage_select picks its clusters
    ReachTree reach_tree(const std::vector<int64_t>& sources, int min_items) const { return reach_tree_handle(h_, sources, min_items); }
    pcv_reach_stats last_reach_stats() const {
        pcv_reach_stats st;
        check(pcv_searcher_last_reach_stats(h_, &st));
        return st;
    }
    // the k nearest other items of every item, found once on the device (neighbors_handle)
    NeighborTable neighbors(const std::vector<int64_t>& sources, size_t k) const { return neighbors_handle(h_, sources, k); }
    pcv_neighbor_stats last_neighbor_stats() const {
        pcv_neighbor_stats st;
        check(pcv_searcher_last_neighbor_stats(h_, &st));
        return st;
    }
    // the k best items of the sources `to` for every item of the sources `from` (match_handle)
    NeighborTable match(const std::vector<int64_t>& from, const std::vector<int64_t>& to, size_t k, float min_score = -1.0f) const {
        return match_handle(h_, from, to, k, min_score);
    }
    pcv_match_stats last_match_stats() const {
        pcv_match_stats st;
        check(pcv_searcher_last_match_stats(h_, &st));
        return st;
    }
    // neighbors, match and find_duplicates with the group table consulted (neighbors_grouped_handle, ...)
    GroupedNeighborTable neighbors_grouped(const std::vector<int64_t>& sources, size_t k, uint32_t flags = PCV_GROUPS_SKIP_OWN) const {
        return neighbors_grouped_handle(h_, sources, k, flags);
    }
    GroupedNeighborTable match_grouped(const std::vector<int64_t>& from, const std::vector<int64_t>& to, size_t k, float min_score = -1.0f,
                                       uint32_t flags = PCV_GROUPS_SKIP_OWN) const {
        return match_grouped_handle(h_, from, to, k, min_score, flags);
    }
    std::vector<DuplicatePair> find_duplicates_grouped(const std::vector<int64_t>& sources, float threshold, size_t max_pairs = 1 << 20,
                                                       int64_t* total = nullptr, int64_t* skipped = nullptr) const {
        return find_duplicates_grouped_handle(h_, sources, threshold, max_pairs, total, skipped);
    }
    pcv_pair_group_stats last_pair_group_stats() const {
        pcv_pair_group_stats st;
        check(pcv_searcher_last_pair_group_stats(h_, &st));
        return st;
    }
    // `perceive search --like <id>`: search with the stored embedding of an item, built on the device; as in the reference the
    // item itself is the first hit unless `exclude`.  nullopt: no row carries the id.
    std::optional<std::vector<SearchItem>> search_like(const std::vector<int64_t>& sources, size_t num_results, int64_t item_id,
                                                       bool exclude = false) const {
        return search_like_handle(h_, sources, num_results, item_id, exclude);
    }
    // search_vector over every rank's shard: a collective, same arguments on all ranks; this rank's rows
    // start at global position `set_shard_offset`
    void set_shard_offset(int64_t first_global_pos) { check(pcv_searcher_set_shard_offset(h_, first_global_pos)); }
    std::vector<SearchItem> search_vector_sharded(Comm& comm, const std::vector<int64_t>& sources, size_t num_results,
                                                  const std::vector<float>& vector) const {
        if (sources.empty()) return {};
        std::vector<int64_t> ids(num_results);
        std::vector<float> scores(num_results);
        int count = 0;
        check(pcv_searcher_search_sharded(h_, comm.handle(), vector.data(), 1, sources.data(), (int)sources.size(),
                                          (int)num_results, ids.data(), scores.data(), &count));
        std::vector<SearchItem> out;
        for (int i = 0; i < count; ++i) out.push_back({ids[i], scores[i]});
        return out;
    }
    int64_t num_rows() const {
        int64_t n = 0;
        check(pcv_searcher_num_rows(h_, &n));
        return n;
    }
    // Searcher::build / rebuild_source against the reference's SQLite file itself (search.rs:38-155): the SQL
    // runs inside the library.  `only_source` empty = every source of the database.
    int64_t load_sqlite(const std::string& db_path, uint32_t model_id, uint32_t model_version,
                        std::optional<int64_t> only_source = std::nullopt) {
        int64_t rows = 0;
        const int64_t src = only_source.value_or(0);
        check(pcv_searcher_load_sqlite(h_, db_path.c_str(), model_id, model_version, only_source ? &src : nullptr, &rows));
        return rows;
    }
    // hidden items (pcv_searcher_hide_ids): rows carrying one of `ids` are no result of any search until unhidden (no
    // rebuild; the library's set persists across finalize and rebuild_source).  `hidden` follows.  Returns the rows changed.
    int64_t hide_items(const std::vector<int64_t>& ids) {
        int64_t rows = 0;
        check(pcv_searcher_hide_ids(h_, ids.data(), (int64_t)ids.size(), &rows));
        hidden.insert(ids.begin(), ids.end());
        return rows;
    }
    int64_t unhide_items(const std::vector<int64_t>& ids) {
        int64_t rows = 0;
        check(pcv_searcher_unhide_ids(h_, ids.data(), (int64_t)ids.size(), &rows));
        for (int64_t id : ids) hidden.erase(id);
        return rows;
    }
    // removed items (pcv_searcher_remove_ids): rows carrying one of `ids` leave the searcher, in every source; the rows behind
    // them move down on the device (no rebuild, no upload; positions shift; the ids are not remembered).  Returns the rows
    // removed.  A SearcherView has no such call: a view is read-only.
    int64_t remove_items(const std::vector<int64_t>& ids) {
        int64_t rows = 0;
        check(pcv_searcher_remove_ids(h_, ids.data(), (int64_t)ids.size(), &rows));
        return rows;
    }
    // updated items (pcv_searcher_update_rows): rows carrying ids[i] take the vector rows[i*dim .. (i+1)*dim) in place (no
    // rebuild).  `found` (if given) gets, per id, whether some row carries it.  Returns the rows rewritten.
    int64_t update_items(const std::vector<int64_t>& ids, const std::vector<float>& rows, std::vector<bool>* found = nullptr) {
        if (rows.size() != ids.size() * (size_t)dim_) throw Error(PCV_ERR_INVALID, "update_items: rows must be ids.size() x dim");
        std::vector<uint8_t> f(ids.size());
        int64_t changed = 0;
        check(pcv_searcher_update_rows(h_, ids.data(), rows.data(), (int64_t)ids.size(), f.data(), &changed));
        if (found) found->assign(f.begin(), f.end());
        return changed;
    }
    // what a source scan produces: ids some row carries take their new vector, the others are added to `source_id`; then
    // finalize.  Returns (rows replaced, rows appended).
    std::pair<int64_t, int64_t> upsert_items(int64_t source_id, const std::vector<int64_t>& ids, const std::vector<float>& rows) {
        std::vector<bool> found;
        const int64_t replaced = update_items(ids, rows, &found);
        std::vector<int64_t> new_ids;
        std::vector<float> new_rows;
        for (size_t i = 0; i < ids.size(); ++i)
            if (!found[i]) {
                new_ids.push_back(ids[i]);
                new_rows.insert(new_rows.end(), rows.begin() + i * dim_, rows.begin() + (i + 1) * dim_);
            }
        if (!new_ids.empty())
            check(pcv_searcher_add_rows(h_, source_id, new_ids.data(), new_rows.data(), (int64_t)new_ids.size()));
        check(pcv_searcher_finalize(h_));
        return {replaced, (int64_t)new_ids.size()};
    }
    // a search restricted to `ids` (the items of a tag, of an author, earlier results): SQL gives the ids, the view searches them
    SearcherView view(const std::vector<int64_t>& ids) const { return SearcherView(h_, ids); }
    // ... over the items that pass a predicate on their value: for predicates too selective for search_vector_where
    SearcherView view_where(const Where& where) const { return SearcherView(h_, where); }
    // capacity hint: the rows about to be added to `source_id` land in one device segment
    void reserve(int64_t source_id, int64_t n_rows) { check(pcv_searcher_reserve(h_, source_id, n_rows)); }
    // narrow screening copy of the rows next to the f32 rows (a half / a quarter of the bytes per scan, same results):
    // PCV_SCREEN_COPY_{OFF, BF16, INT8, AUTO}; built by the next rebuild / finalize
    void set_screening_copy(int mode) { check(pcv_searcher_set_screening_copy(h_, mode)); }
    pcv_scan_stats last_stats() const {
        pcv_scan_stats st;
        check(pcv_searcher_last_stats(h_, &st));
        return st;
    }
    pcv_searcher* handle() const { return h_; }

private:
    void insert(const EmbeddingRow& r) { insert(r, r.source_id); }
    void insert(const EmbeddingRow& r, int64_t into_source) {
        if ((int)r.embedding.size() != dim_ * 4)
            throw Error(PCV_ERR_INVALID, "embedding blob of item " + std::to_string(r.item_id) + " has the wrong size");
        check(pcv_searcher_add_blobs(h_, into_source, &r.item_id, r.embedding.data(), 1));
    }
    pcv_searcher* h_ = nullptr;
    int dim_;
};

// configs.rs:30-39, model_id() of configs.rs:72-83
enum class SentenceEmbeddingsModelType {
    AllMiniLmL6V2 = 0,
    AllMiniLmL12V2 = 1,
    DistiluseBaseMultilingualCased = 2,
    AllDistilrobertaV1 = 3,
    ParaphraseAlbertSmallV2 = 4,
    MsMarcoDistilbertDotV5 = 5,
    MsMarcoDistilbertBaseTasB = 6,
    MsMarcoBertBaseDotV5 = 7,
};
inline uint32_t model_id(SentenceEmbeddingsModelType t) { return (uint32_t)t; }

// One tensor of a checkpoint file (model.safetensors, rust_model.ot, pytorch_model.bin) as pcv_checkpoint_visit reports it
struct CheckpointTensor {
    std::string name;
    std::vector<int64_t> shape;
    int dtype = PCV_TENSOR_OTHER;
    std::vector<float> values;  // empty for integer tensors
};
inline std::vector<CheckpointTensor> read_checkpoint(const std::string& path) {
    std::vector<CheckpointTensor> out;
    auto visit = [](void* user, const char* name, const int64_t* shape, int rank, int dtype, const float* values, int64_t numel) -> int {
        auto* v = static_cast<std::vector<CheckpointTensor>*>(user);
        CheckpointTensor t;
        t.name = name;
        t.shape.assign(shape, shape + rank);
        t.dtype = dtype;
        if (values) t.values.assign(values, values + numel);
        v->push_back(std::move(t));
        return 0;
    };
    const pcv_status st = pcv_checkpoint_visit(path.c_str(), visit, &out);
    if (st != PCV_OK) throw ModelError(st, pcv_last_error());
    return out;
}

// SentenceEmbeddingsTokenizerOuput of tokenize.rs:9-57: right-padded ids, mask = id != pad
struct TokenTensors {
    std::vector<int64_t> tokens_ids, tokens_masks;
    int batch = 0, len = 0;
};
inline TokenTensors generate_token_tensors(const std::vector<std::vector<int64_t>>& token_ids, int64_t pad_token_id = 0) {
    TokenTensors t;
    t.batch = (int)token_ids.size();
    for (auto& v : token_ids) t.len = std::max<int>(t.len, (int)v.size());
    t.tokens_ids.assign((size_t)t.batch * t.len, pad_token_id);
    for (int b = 0; b < t.batch; ++b)
        for (size_t i = 0; i < token_ids[b].size(); ++i) t.tokens_ids[(size_t)b * t.len + i] = token_ids[b][i];
    t.tokens_masks.resize(t.tokens_ids.size());
    for (size_t i = 0; i < t.tokens_ids.size(); ++i) t.tokens_masks[i] = t.tokens_ids[i] != pad_token_id;
    return t;
}

// model.rs:56-191
class Model {
public:
    SentenceEmbeddingsModelType model_type;  // pub field, model.rs:57

    Model(Context& ctx, const pcv_model_desc& desc, const char* weights_path, uint64_t synthetic_seed = 0,
          SentenceEmbeddingsModelType type = SentenceEmbeddingsModelType::AllMiniLmL6V2)
        : model_type(type) {
        pcv_status s = pcv_model_create(ctx.handle(), &desc, weights_path, synthetic_seed, &h_);
        if (s != PCV_OK) throw ModelError(s, pcv_last_error());
        check(pcv_model_output_dim(h_, &dim_));
    }
    // Model::new_pretrained (model.rs:68-174) from a sentence-transformers directory: configs, tokenizer and
    // model.safetensors are read by the library; the model owns its tokenizer
    Model(Context& ctx, const std::string& model_dir, SentenceEmbeddingsModelType type = SentenceEmbeddingsModelType::AllMiniLmL6V2,
          int compute = PCV_COMPUTE_F32, bool load_weights = true)
        : model_type(type) {
        pcv_status s = pcv_model_create_from_dir(ctx.handle(), model_dir.c_str(), compute, load_weights ? 1 : 0, &h_);
        if (s != PCV_OK) throw ModelError(s, pcv_last_error());
        check(pcv_model_output_dim(h_, &dim_));
    }
    ~Model() { pcv_model_destroy(h_); }
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;

    // Model::encode(&[S]) (model.rs:176-179): tokenize + forward in one call
    std::vector<std::vector<float>> encode(const std::vector<std::string>& inputs) const {
        std::vector<const char*> ptrs;
        std::vector<size_t> lens;
        for (const auto& t : inputs) {
            ptrs.push_back(t.data());
            lens.push_back(t.size());
        }
        std::vector<float> flat(inputs.size() * (size_t)dim_);
        pcv_status s = pcv_model_encode_text(h_, ptrs.data(), lens.data(), (int)inputs.size(), flat.data());
        if (s != PCV_OK) throw ModelError(s, pcv_last_error());
        std::vector<std::vector<float>> out(inputs.size());
        for (size_t b = 0; b < inputs.size(); ++b) out[b].assign(flat.begin() + b * dim_, flat.begin() + (b + 1) * dim_);
        return out;
    }
    // Model::highlight (highlight.rs:23-165): views into `documents` (nullopt: the document gave no chunk)
    std::vector<std::optional<std::string_view>> highlight(const std::string& query, const std::vector<std::string>& documents) const {
        std::vector<const char*> ptrs;
        std::vector<size_t> lens;
        for (const auto& d : documents) {
            ptrs.push_back(d.data());
            lens.push_back(d.size());
        }
        std::vector<int64_t> b(documents.size(), -1), e(documents.size(), -1);
        pcv_status s = pcv_model_highlight(h_, query.data(), query.size(), ptrs.data(), lens.data(), (int)documents.size(), 0, -1,
                                           b.data(), e.data());
        if (s != PCV_OK) throw ModelError(s, pcv_last_error());
        std::vector<std::optional<std::string_view>> out(documents.size());
        for (size_t i = 0; i < documents.size(); ++i)
            if (b[i] >= 0) out[i] = std::string_view(documents[i]).substr((size_t)b[i], (size_t)(e[i] - b[i]));
        return out;
    }

    // Model::encode_tokens (model.rs:181-190 -> worker.rs:78-106); result rows = Vec<Vec<f32>>::from(Tensor)
    std::vector<std::vector<float>> encode_tokens(const TokenTensors& t) const {
        std::vector<float> flat((size_t)t.batch * dim_);
        pcv_status s = pcv_model_encode_tokens(h_, t.tokens_ids.data(), t.tokens_masks.data(), t.batch, t.len, flat.data());
        if (s != PCV_OK) throw ModelError(s, pcv_last_error());
        std::vector<std::vector<float>> out(t.batch);
        for (int b = 0; b < t.batch; ++b) out[b].assign(flat.begin() + (size_t)b * dim_, flat.begin() + (size_t)(b + 1) * dim_);
        return out;
    }
    int output_dim() const { return dim_; }

private:
    pcv_model* h_ = nullptr;
    int dim_ = 0;
};

// lib.rs:63-77, row-major [B][N] result
inline std::vector<float> dot_product(Context& ctx, const std::vector<float>& set1, int B, const std::vector<float>& set2,
                                      int64_t N, int dim) {
    std::vector<float> out((size_t)B * N);
    check(pcv_dot_product(ctx.handle(), set1.data(), B, set2.data(), N, dim, out.data()));
    return out;
}
inline std::vector<float> cosine_similarity_multi_query(Context& ctx, const std::vector<float>& set1, int B,
                                                        const std::vector<float>& set2, int64_t N, int dim) {
    std::vector<float> out((size_t)B * N);
    check(pcv_cosine_similarity(ctx.handle(), set1.data(), B, set2.data(), N, dim, out.data()));
    return out;
}
inline std::vector<float> cosine_similarity_single_query(Context& ctx, const std::vector<float>& query,
                                                         const std::vector<float>& matches, int64_t N, int dim) {
    return cosine_similarity_multi_query(ctx, query, 1, matches, N, dim);
}

}  // namespace perceive
