// Drives Searcher::view of the C++ host mirror (include/perceive.hpp) on the GPU: a view of the even item ids searches like a
// searcher built from the even rows only, follows a hide on its parent (one refresh), and keeps its parent alive.
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
    std::mt19937 rng(21);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    std::vector<EmbeddingRow> rows, even_rows;
    std::vector<int64_t> even;
    for (int i = 0; i < N; ++i) {
        for (auto& v : emb[i]) v = nd(rng);
        rows.push_back({7000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 2 == 0) {
            even.push_back(7000 + i);
            even_rows.push_back(rows.back());
        }
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Dot);
    auto f = Searcher::build(ctx, even_rows, D, Metric::Dot);
    {
        SearcherView v = s->view(even);
        EXPECT(v.num_rows() == N / 2);
        // an odd row's own vector: its best hit among the even rows, as the fresh searcher ranks them
        for (int i : {11, 12, 1999}) {
            const auto a = v.search_vector({1, 2}, 5, emb[i]);
            const auto b = f->search_vector({1, 2}, 5, emb[i]);
            EXPECT(a.size() == 5 && a.size() == b.size());
            for (size_t j = 0; j < a.size() && j < b.size(); ++j) EXPECT(a[j].id == b[j].id && a[j].score == b[j].score);
            for (const auto& h : a) EXPECT(h.id % 2 == 0);
        }
        EXPECT(v.search_vector({1}, 1, emb[12]).at(0).id == 7012);
        EXPECT(v.search_vector({2}, 3, emb[12]).empty());  // source 2 holds the odd rows only
        EXPECT(v.refreshes() == 0);
        s->hide_items({7012});
        const auto h = v.search_vector({1}, 1, emb[12]);
        EXPECT(!h.empty() && h[0].id != 7012);
        EXPECT(v.refreshes() == 1 && v.num_rows() == N / 2);
        bool threw = false;
        try {
            check(pcv_searcher_destroy(s->handle()));  // views alive: refused
        } catch (const Error&) {
            threw = true;
        }
        EXPECT(threw);
    }
    if (failures) return 1;
    std::printf("view_mirror_test: ok\n");
    return 0;
}
