// Drives Searcher::search_range / SearcherView::search_range of the C++ host mirror (include/perceive.hpp) on the GPU: a range
// search returns the hits of a full search_vector cut at the bound, `more` says when max_results cut it short, and a view
// returns only its own items.
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
    std::mt19937 rng(35);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < N; ++i) {
        for (auto& v : emb[i]) v = nd(rng);
        rows.push_back({7000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 2 == 0) even.push_back(7000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Dot);
    for (int i : {0, 11, 1999}) {
        const auto full = s->search_vector({1, 2}, N, emb[i]);
        EXPECT(full.size() == (size_t)N);
        for (size_t cut : {(size_t)1, (size_t)37, (size_t)700}) {
            const float bound = full[cut - 1].score;  // distance <= bound: the first `cut` hits and whatever ties with the last
            size_t want = cut;
            while (want < full.size() && full[want].score <= bound) ++want;
            bool more = true;
            const auto r = s->search_range({1, 2}, bound, N, emb[i], &more);
            EXPECT(r.size() == want && !more);
            for (size_t j = 0; j < r.size() && j < want; ++j) EXPECT(r[j].id == full[j].id && r[j].score == full[j].score);
            const auto few = s->search_range({1, 2}, bound, 5, emb[i], &more);
            EXPECT(few.size() == std::min<size_t>(5, want) && more == (want > 5));
            for (size_t j = 0; j < few.size(); ++j) EXPECT(few[j].id == full[j].id);
        }
        bool more = true;
        EXPECT(s->search_range({1, 2}, -1.0f, 10, emb[i], &more).empty() && !more);  // a negative distance bound matches nothing
        EXPECT(s->search_range({}, 2.0f, 10, emb[i]).empty());                       // an empty filter matches nothing
        more = true;
        EXPECT(s->search_range({1, 2}, 2.0f, 0, emb[i], &more).empty() && !more);    // room for nothing: empty, as the Rust twin
    }
    {
        SearcherView v = s->view(even);
        const auto full = v.search_vector({1, 2}, N, emb[11]);
        EXPECT(full.size() == even.size());
        const float bound = full[99].score;
        size_t want = 100;
        while (want < full.size() && full[want].score <= bound) ++want;
        const auto r = v.search_range({1, 2}, bound, N, emb[11]);
        EXPECT(r.size() == want);
        for (size_t j = 0; j < r.size() && j < want; ++j) EXPECT(r[j].id == full[j].id && r[j].score == full[j].score && r[j].id % 2 == 0);
    }
    if (failures) return 1;
    std::printf("range_mirror_test: ok\n");
    return 0;
}
