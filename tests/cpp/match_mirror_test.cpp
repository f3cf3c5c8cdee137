// Drives Searcher::match and SearcherView::match of the C++ host mirror (include/perceive.hpp) on the GPU: 200 items of 64 features in
// four planted clusters, the even items in source 1 and the odd ones in source 2 — every item's three best items of the other source
// belong to its own cluster, best first; the square is the neighbours' table; an empty `to` matches nothing, an empty `from` selects
// nothing; a score bound no pair reaches leaves every list empty; and a view matches among its own items.
#include <cmath>
#include <cstdio>
#include <random>

#include "perceive.hpp"

using namespace perceive;

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// every item has k matches of its cluster whose parity is `to_parity`
static void check_table(const NeighborTable& t, size_t n, size_t k, int from_parity, int to_parity) {
    EXPECT(t.k == k && t.ids.size() == n && t.counts.size() == n && t.neighbor_ids.size() == n * k && t.scores.size() == n * k);
    for (size_t r = 0; r < t.ids.size(); ++r) {
        EXPECT(t.counts[r] == (int32_t)k);
        EXPECT((t.ids[r] - 9000) % 2 == from_parity);
        for (size_t j = 0; j < k; ++j) {
            const int64_t m = t.neighbor_ids[r * k + j];
            EXPECT(m != t.ids[r] && (m - 9000) % 4 == (t.ids[r] - 9000) % 4 && (m - 9000) % 2 == to_parity);
            EXPECT(t.scores[r * k + j] > 0.8f && t.scores[r * k + j] <= 1.0f);
            EXPECT(j == 0 || t.scores[r * k + j] <= t.scores[r * k + j - 1]);
        }
    }
}

int main() {
    Context ctx(0);
    const int D = 64, N = 200, K = 2;  // (two clusters a parity: cluster = i % 4, source = 1 + i % 2)
    std::mt19937 rng(54);
    std::normal_distribution<float> nd;
    std::vector<float> centres((size_t)2 * K * D);
    for (auto& v : centres) v = nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> some;
    for (int i = 0; i < N; ++i) {
        std::vector<float> e(D);
        for (int f = 0; f < D; ++f) e[f] = (centres[(size_t)(i % 4) * D + f] + 0.2f * nd(rng)) * (1.0f + 0.25f * (i % 3));
        rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(e)});
        if (i < 120) some.push_back(9000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    // clusters 0 and 2 are even, 1 and 3 odd: across the sources no item has a match of its own cluster, so match within a parity
    check_table(s->match({1}, {1}, 3), N / 2, 3, 0, 0);
    const pcv_match_stats st = s->last_match_stats();
    EXPECT(st.rows == N / 2 && st.partner_rows == N / 2 && st.k == 3 && st.listed == 3 * (N / 2) && st.candidates >= st.listed && st.tile_rows == 128);
    EXPECT(st.owner_blocks == 4 && st.partner_blocks == 4);
    // the square is the neighbours' table
    const NeighborTable a = s->match({1, 2}, {1, 2}, 3), b = s->neighbors({1, 2}, 3);
    EXPECT(a.ids == b.ids && a.neighbor_ids == b.neighbor_ids && a.counts == b.counts);
    for (size_t i = 0; i < a.scores.size(); ++i) EXPECT(a.scores[i] == b.scores[i]);
    // a rectangle: the items of source 2 against those of source 1 — other clusters, so nothing is near, and every list is full
    const NeighborTable x = s->match({2}, {1}, 3);
    EXPECT(x.ids.size() == (size_t)N / 2);
    for (size_t r = 0; r < x.ids.size(); ++r) {
        EXPECT(x.counts[r] == 3 && (x.ids[r] - 9000) % 2 == 1);
        for (size_t j = 0; j < 3; ++j) EXPECT((x.neighbor_ids[r * 3 + j] - 9000) % 2 == 0 && x.scores[r * 3 + j] < 0.8f);
    }
    EXPECT(s->last_match_stats().owner_blocks == 4 && s->last_match_stats().partner_blocks == 4 && s->last_match_stats().rows == N / 2);
    // ... and with a bound above them every list is empty
    const NeighborTable y = s->match({2}, {1}, 3, 0.8f);
    EXPECT(y.ids == x.ids);
    for (size_t r = 0; r < y.ids.size(); ++r) EXPECT(y.counts[r] == 0 && y.neighbor_ids[r * 3] == -1 && std::isnan(y.scores[r * 3]));
    // an empty `to` matches nothing, an empty `from` selects nothing
    const NeighborTable e = s->match({1}, {}, 3);
    EXPECT(e.ids.size() == (size_t)N / 2);
    for (size_t r = 0; r < e.ids.size(); ++r) EXPECT(e.counts[r] == 0 && e.neighbor_ids[r * 3] == -1);
    EXPECT(s->last_match_stats().partner_rows == 0 && s->last_match_stats().partner_blocks == 0);
    EXPECT(s->match({}, {1}, 3).ids.empty());
    // a view matches among its own items: the first 120, 60 a source
    SearcherView v = s->view(some);
    check_table(v.match({2}, {2}, 2), 60, 2, 1, 1);
    EXPECT(v.last_match_stats().rows == 60 && v.last_match_stats().partner_rows == 60);
    if (failures == 0) std::printf("match_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
