// Drives Searcher::search_vector_distinct / SearcherView::search_vector_distinct of the C++ host mirror (include/perceive.hpp) on
// the GPU: planted copies of an item collapse into one hit that counts them, rows that are no duplicates come back as search_vector
// returns them, and a view walks only its own items.
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
    const int D = 384, N = 2000, COPIES = 6;
    std::mt19937 rng(41);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    for (int i = 0; i < N; ++i)
        for (auto& v : emb[i]) v = nd(rng);
    // rows 100 .. 100 + COPIES - 1 are row 50 with a little noise (cosine about 0.9998); the odd ones are out of the view
    for (int c = 0; c < COPIES; ++c)
        for (int f = 0; f < D; ++f) emb[100 + c][f] = emb[50][f] + 0.02f * nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < N; ++i) {
        rows.push_back({7000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 2 == 0) even.push_back(7000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const auto full = s->search_vector({1, 2}, 40, emb[50]);
    EXPECT(full.size() == 40 && full[0].id == 7050);
    {
        std::vector<int32_t> similar;
        const auto r = s->search_vector_distinct({1, 2}, 10, emb[50], 0.95f, 0, &similar);
        EXPECT(r.size() == 10 && similar.size() == 10);
        EXPECT(r[0].id == 7050 && r[0].score == full[0].score && similar[0] == COPIES);
        // behind the copies the list goes on as search_vector's: Gaussian rows are no duplicates of each other
        for (size_t j = 1; j < r.size(); ++j) EXPECT(r[j].id == full[j + COPIES].id && r[j].score == full[j + COPIES].score && similar[j] == 0);
        // a threshold nothing reaches: the plain list
        const auto plain = s->search_vector_distinct({1, 2}, 10, emb[50], 1.0f);
        for (size_t j = 0; j < plain.size(); ++j) EXPECT(plain[j].id == full[j].id && plain[j].score == full[j].score);
        EXPECT(plain.size() == 10);
        EXPECT(s->search_vector_distinct({}, 10, emb[50], 0.95f).empty());       // an empty filter matches nothing
        EXPECT(s->search_vector_distinct({1, 2}, 0, emb[50], 0.95f).empty());    // room for nothing
    }
    {
        SearcherView v = s->view(even);
        std::vector<int32_t> similar;
        const auto r = v.search_vector_distinct({1, 2}, 5, emb[50], 0.95f, 128, &similar);
        EXPECT(r.size() == 5 && r[0].id == 7050 && similar[0] == COPIES / 2);
        for (const auto& it : r) EXPECT(it.id % 2 == 0);
    }
    if (failures) return 1;
    std::printf("distinct_mirror_test: ok\n");
    return 0;
}
