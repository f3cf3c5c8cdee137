// Drives Searcher::hide_items / unhide_items of the C++ host mirror (include/perceive.hpp) on the GPU: the best hit of a
// query is hidden and comes back, with the same distance.  Expected values are recomputed with plain f64 loops.
#include <algorithm>
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
    const int D = 384, N = 2000;
    std::mt19937 rng(11);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    std::vector<EmbeddingRow> rows;
    for (int i = 0; i < N; ++i) {
        for (auto& v : emb[i]) v = nd(rng);
        rows.push_back({5000 + i, 1, serialize_embedding(emb[i])});
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Dot);
    std::vector<float> q(D);
    for (auto& v : q) v = nd(rng);
    std::vector<std::pair<double, int64_t>> ref;
    for (int i = 0; i < N; ++i) {
        double dot = 0;
        for (int k = 0; k < D; ++k) dot += (double)q[k] * (double)emb[i][k];
        ref.push_back({dot, rows[i].item_id});
    }
    std::stable_sort(ref.begin(), ref.end(), [](auto& a, auto& b) { return a.first > b.first; });

    const auto before = s->search_vector({1}, 5, q);
    EXPECT(before.size() == 5 && before[0].id == ref[0].second);
    EXPECT(s->hide_items({ref[0].second, ref[0].second, 424242}) == 1);  // a duplicate and an id no row has
    EXPECT(s->hidden.count(ref[0].second) == 1);
    const auto hidden = s->search_vector({1}, 5, q);
    EXPECT(hidden.size() == 5);
    for (size_t j = 0; j < hidden.size() && j + 1 < ref.size(); ++j) {
        EXPECT(hidden[j].id == ref[j + 1].second);
        EXPECT(std::fabs(hidden[j].score - (float)std::max(0.0, 1.0 - ref[j + 1].first / D)) < 1e-6f);
    }
    EXPECT(s->num_rows() == N);  // hidden rows keep their place
    EXPECT(s->unhide_items({ref[0].second}) == 1);
    EXPECT(s->hidden.count(ref[0].second) == 0);
    const auto after = s->search_vector({1}, 5, q);
    EXPECT(after.size() == before.size());
    for (size_t j = 0; j < after.size() && j < before.size(); ++j) {
        EXPECT(after[j].id == before[j].id);
        EXPECT(after[j].score == before[j].score);
    }
    if (failures) return 1;
    std::printf("hide_mirror_test: ok\n");
    return 0;
}
