// Drives Searcher::search_like / SearcherView::search_like of the C++ host mirror (include/perceive.hpp) on the GPU: searching
// by a stored item equals searching with that item's vector, the item itself comes first unless excluded, an unknown id is
// nullopt, and a view looks the example up in its parent.
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
    std::mt19937 rng(33);
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
        const auto a = s->search_like({1, 2}, 20, 7000 + i);
        const auto b = s->search_vector({1, 2}, 20, emb[i]);
        EXPECT(a.has_value() && a->size() == 20 && b.size() == 20);
        if (!a) continue;
        EXPECT(a->at(0).id == 7000 + i);  // the reference's behaviour: the item itself is hit 1
        for (size_t j = 0; j < a->size() && j < b.size(); ++j) EXPECT((*a)[j].id == b[j].id && (*a)[j].score == b[j].score);
        const auto x = s->search_like({1, 2}, 19, 7000 + i, true);
        EXPECT(x.has_value() && x->size() == 19);
        for (size_t j = 0; x && j < x->size(); ++j) EXPECT((*x)[j].id == b[j + 1].id && (*x)[j].score == b[j + 1].score);
    }
    EXPECT(!s->search_like({1, 2}, 5, 123).has_value());  // "Item not found"
    const auto none = s->search_like({}, 5, 7011);         // an empty filter matches nothing; the item exists
    EXPECT(none.has_value() && none->empty());
    {
        SearcherView v = s->view(even);
        // an odd item as the example: not in the view, found in the parent; every hit is an even item
        const auto a = v.search_like({1, 2}, 5, 7011);
        const auto b = v.search_vector({1, 2}, 5, emb[11]);
        EXPECT(a.has_value() && a->size() == 5 && b.size() == 5);
        for (size_t j = 0; a && j < a->size() && j < b.size(); ++j)
            EXPECT((*a)[j].id == b[j].id && (*a)[j].score == b[j].score && (*a)[j].id % 2 == 0);
        const auto e = v.search_like({1}, 3, 7012, true);
        EXPECT(e.has_value() && e->size() == 3);
        for (size_t j = 0; e && j < e->size(); ++j) EXPECT((*e)[j].id != 7012);
        EXPECT(!v.search_like({1, 2}, 5, 5).has_value());
    }
    if (failures) return 1;
    std::printf("like_mirror_test: ok\n");
    return 0;
}
