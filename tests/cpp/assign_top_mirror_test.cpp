// Drives Searcher::assign_top and SearcherView::assign_top of the C++ host mirror (include/perceive.hpp) on the GPU: 200 items of 64
// features in four planted clusters list their cluster's centre first and m labels in all, the first slot is what assign gives, the
// rows per label add up, a score bound keeps the centre alone, an empty filter selects nothing and a view lists only its own items.
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
    for (int i = 0; i < N; ++i) {
        std::vector<float> e(D);
        for (int f = 0; f < D; ++f) e[f] = (centres[(size_t)(i % K) * D + f] + 0.3f * nd(rng)) * (1.0f + 0.25f * (i % 3));
        rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(e)});
        if (i % 2 == 0) even.push_back(9000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const Assignment a = s->assign({1, 2}, centres, K);
    for (size_t m : {(size_t)1, (size_t)3, (size_t)8}) {
        const TopLabels t = s->assign_top({1, 2}, centres, K, m);
        const size_t kept = std::min<size_t>(m, K);
        EXPECT(t.m == m && t.ids.size() == (size_t)N && t.counts.size() == (size_t)N && t.labels.size() == (size_t)N * m);
        EXPECT(t.scores.size() == (size_t)N * m && t.label_rows.size() == (size_t)K);
        EXPECT(t.ids == a.ids);
        int64_t total = 0;
        for (int j = 0; j < K; ++j) total += t.label_rows[j];
        EXPECT(total == (int64_t)(N * kept));
        for (size_t r = 0; r < t.ids.size(); ++r) {
            EXPECT(t.counts[r] == (int32_t)kept);
            EXPECT(t.labels[r * m] == a.label[r] && t.scores[r * m] == a.score[r]);
            for (size_t j = 1; j < kept; ++j) {
                const float hi = t.scores[r * m + j - 1], lo = t.scores[r * m + j];
                EXPECT(hi > lo || (hi == lo && t.labels[r * m + j - 1] < t.labels[r * m + j]));
            }
            for (size_t j = kept; j < m; ++j) EXPECT(t.labels[r * m + j] == -1 && std::isnan(t.scores[r * m + j]));
        }
        if (m == 1) EXPECT(t.label_rows == a.counts);
        const pcv_assign_top_stats st = s->last_assign_top_stats();
        EXPECT(st.rows == N && st.m == (int32_t)m && st.label_tiles == 1 && st.tile_labels == 128 && st.reruns == 0);
        EXPECT(st.listed == (int64_t)(N * kept) && st.candidates >= st.listed);
    }
    {
        // with a bound between the centre's score and the others', every item lists its centre alone
        const TopLabels t = s->assign_top({1, 2}, centres, K, 3, 0.8f);
        for (size_t r = 0; r < t.ids.size(); ++r)
            EXPECT(t.counts[r] == 1 && t.labels[r * 3] == (int32_t)((t.ids[r] - 9000) % K) && t.labels[r * 3 + 1] == -1 && t.scores[r * 3] >= 0.8f);
        for (int j = 0; j < K; ++j) EXPECT(t.label_rows[j] == N / K);
        EXPECT(s->assign_top({}, centres, K, 3).ids.empty());  // an empty filter selects nothing
        const TopLabels odd = s->assign_top({2}, centres, K, 2);
        EXPECT(odd.ids.size() == (size_t)N / 2);
        for (size_t r = 0; r < odd.ids.size(); ++r) EXPECT((odd.ids[r] - 9000) % 2 == 1 && odd.labels[r * 2] == (int32_t)((odd.ids[r] - 9000) % K));

        SearcherView v = s->view(even);
        const TopLabels vt = v.assign_top({1, 2}, centres, K, 2);
        EXPECT(vt.ids.size() == even.size());
        for (size_t r = 0; r < vt.ids.size(); ++r)
            EXPECT((vt.ids[r] - 9000) % 2 == 0 && vt.counts[r] == 2 && vt.labels[r * 2] == (int32_t)((vt.ids[r] - 9000) % K));
        EXPECT(v.last_assign_top_stats().rows == (int64_t)even.size());
    }
    if (failures == 0) std::printf("assign_top_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
