// Drives Searcher::neighbors and SearcherView::neighbors of the C++ host mirror (include/perceive.hpp) on the GPU: 200 items of 64
// features in four planted clusters — every item's three nearest items belong to its own cluster, best first, never the item
// itself; an empty filter selects nothing, one source lists its own items, and a view lists only its own.
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

static void check_table(const NeighborTable& t, size_t n, size_t k, int parity) {
    EXPECT(t.k == k && t.ids.size() == n && t.counts.size() == n && t.neighbor_ids.size() == n * k && t.scores.size() == n * k);
    for (size_t r = 0; r < t.ids.size(); ++r) {
        EXPECT(t.counts[r] == (int32_t)k);
        EXPECT(parity < 0 || (t.ids[r] - 9000) % 2 == parity);
        for (size_t j = 0; j < k; ++j) {
            const int64_t nb = t.neighbor_ids[r * k + j];
            EXPECT(nb != t.ids[r] && (nb - 9000) % 4 == (t.ids[r] - 9000) % 4);
            EXPECT(parity < 0 || (nb - 9000) % 2 == parity);
            EXPECT(t.scores[r * k + j] > 0.8f && t.scores[r * k + j] <= 1.0f);
            EXPECT(j == 0 || t.scores[r * k + j] <= t.scores[r * k + j - 1]);
        }
    }
}

int main() {
    Context ctx(0);
    const int D = 64, N = 200, K = 4;
    std::mt19937 rng(53);
    std::normal_distribution<float> nd;
    std::vector<float> centres((size_t)K * D);
    for (auto& v : centres) v = nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < N; ++i) {
        std::vector<float> e(D);
        for (int f = 0; f < D; ++f) e[f] = (centres[(size_t)(i % K) * D + f] + 0.2f * nd(rng)) * (1.0f + 0.25f * (i % 3));
        rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(e)});
        if (i % 2 == 0) even.push_back(9000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    check_table(s->neighbors({1, 2}, 3), N, 3, -1);
    const pcv_neighbor_stats st = s->last_neighbor_stats();
    EXPECT(st.rows == N && st.k == 3 && st.listed == 3 * N && st.candidates >= 3 * N && st.tile_rows == 128 && st.sample_stride == 1 && st.spans >= 1);
    EXPECT(s->neighbors({}, 3).ids.empty());  // an empty filter selects nothing
    check_table(s->neighbors({2}, 3), N / 2, 3, 1);  // source 2: the odd items, among themselves
    SearcherView v = s->view(even);
    check_table(v.neighbors({1, 2}, 2), even.size(), 2, 0);
    EXPECT(v.last_neighbor_stats().rows == (int64_t)even.size());
    if (failures == 0) std::printf("neighbors_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
