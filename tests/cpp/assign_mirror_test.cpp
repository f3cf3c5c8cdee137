// Drives Searcher::assign / kmeans and SearcherView::assign of the C++ host mirror (include/perceive.hpp) on the GPU: 200 items of
// 64 features in four planted clusters get the label of their cluster's centre, the counts add up, an empty filter selects nothing,
// a view labels only its own items, and k-means started from one item of each cluster finds the clusters and stops by itself.
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

int main() {
    Context ctx(0);
    const int D = 64, N = 200, K = 4;
    std::mt19937 rng(47);
    std::normal_distribution<float> nd;
    std::vector<float> centres((size_t)K * D);
    for (auto& v : centres) v = nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    std::vector<float> first((size_t)K * D);
    for (int i = 0; i < N; ++i) {
        std::vector<float> e(D);
        for (int f = 0; f < D; ++f) e[f] = (centres[(size_t)(i % K) * D + f] + 0.3f * nd(rng)) * (1.0f + 0.25f * (i % 3));
        if (i < K) std::copy(e.begin(), e.end(), first.begin() + (size_t)i * D);
        rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(e)});
        if (i % 2 == 0) even.push_back(9000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    {
        // the items come back by position: source 1 (even i) first, then source 2
        const Assignment a = s->assign({1, 2}, centres, K);
        EXPECT(a.label.size() == (size_t)N && a.score.size() == (size_t)N && a.ids.size() == (size_t)N && a.counts.size() == (size_t)K);
        int64_t total = 0;
        for (int j = 0; j < K; ++j) {
            EXPECT(a.counts[j] == N / K);
            total += a.counts[j];
        }
        EXPECT(total == N);
        for (size_t r = 0; r < a.label.size(); ++r) {
            EXPECT(a.label[r] == (int32_t)((a.ids[r] - 9000) % K));
            EXPECT(a.score[r] > 0.8f && a.score[r] <= 1.0f);
        }
        const pcv_assign_stats st = s->last_assign_stats();
        EXPECT(st.rows == N && st.label_tiles == 1 && st.tile_labels == 128 && st.candidates >= N);
        EXPECT(s->assign({}, centres, K).label.empty());  // an empty filter selects nothing
        const Assignment odd = s->assign({2}, centres, K);
        EXPECT(odd.label.size() == (size_t)N / 2);
        for (size_t r = 0; r < odd.ids.size(); ++r) EXPECT((odd.ids[r] - 9000) % 2 == 1 && odd.label[r] == (int32_t)((odd.ids[r] - 9000) % K));

        SearcherView v = s->view(even);
        const Assignment va = v.assign({1, 2}, centres, K);
        EXPECT(va.label.size() == even.size());
        for (size_t r = 0; r < va.ids.size(); ++r) EXPECT((va.ids[r] - 9000) % 2 == 0 && va.label[r] == (int32_t)((va.ids[r] - 9000) % K));
    }
    {
        const KMeansResult km = s->kmeans({1, 2}, first, K, 10);
        EXPECT(km.iterations >= 1 && km.iterations < 10);
        EXPECT(km.moved.size() == (size_t)km.iterations + 1 && km.moved.front() == N && km.moved.back() == 0);
        EXPECT(km.centroids.size() == (size_t)K * D);
        for (size_t r = 0; r < km.last.label.size(); ++r) EXPECT(km.last.label[r] == (int32_t)((km.last.ids[r] - 9000) % K));
        for (int j = 0; j < K; ++j) EXPECT(km.last.counts[j] == N / K);
        const KMeansResult zero = s->kmeans({1, 2}, centres, K, 0);
        const Assignment a = s->assign({1, 2}, centres, K);
        EXPECT(zero.iterations == 0 && zero.last.label == a.label && zero.centroids == centres);
    }
    if (failures == 0) std::printf("assign_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
