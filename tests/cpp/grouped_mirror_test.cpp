// Drives Searcher::set_groups / groups_of / search_vector_grouped and SearcherView::search_vector_grouped of the C++ host mirror
// (include/perceive.hpp) on the GPU: the rows of a planted document collapse into its best member, which counts them; rows without
// a group come back as search_vector returns them; a view walks only its own items by its parent's groups.
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
    const int D = 384, N = 2000, CHUNKS = 6;
    std::mt19937 rng(43);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    for (int i = 0; i < N; ++i)
        for (auto& v : emb[i]) v = nd(rng);
    // rows 100 .. 100 + CHUNKS - 1 are chunks of the document of row 50: row 50 with noise (cosine about 0.995, far above the
    // 0.2 or so of the best unrelated Gaussian row)
    for (int c = 0; c < CHUNKS; ++c)
        for (int f = 0; f < D; ++f) emb[100 + c][f] = emb[50][f] + 0.1f * nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < N; ++i) {
        rows.push_back({7000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 2 == 0) even.push_back(7000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const auto full = s->search_vector({1, 2}, 40, emb[50]);
    EXPECT(full.size() == 40 && full[0].id == 7050);
    {  // no table yet: the plain list
        const auto plain = s->search_vector_grouped({1, 2}, 10, emb[50]);
        EXPECT(plain.size() == 10);
        for (size_t j = 0; j < plain.size(); ++j)
            EXPECT(plain[j].item.id == full[j].id && plain[j].item.score == full[j].score && plain[j].group == PCV_NO_GROUP && plain[j].collapsed == 0);
    }
    std::vector<int64_t> doc_ids{7050}, doc_groups{9};
    for (int c = 0; c < CHUNKS; ++c) doc_ids.push_back(7100 + c), doc_groups.push_back(9);
    s->set_groups(doc_ids, doc_groups);
    {
        const auto g = s->groups_of({7050, 7103, 7051, -1});
        EXPECT(g.size() == 4 && g[0] == 9 && g[1] == 9 && g[2] == PCV_NO_GROUP && g[3] == PCV_NO_GROUP);
        bool more = true;
        const auto r = s->search_vector_grouped({1, 2}, 10, emb[50], 0, &more);
        EXPECT(r.size() == 10 && !more);
        EXPECT(r[0].item.id == 7050 && r[0].item.score == full[0].score && r[0].group == 9 && r[0].collapsed == CHUNKS);
        // behind the document the list goes on as search_vector's: the other rows have no group
        for (size_t j = 1; j < r.size(); ++j)
            EXPECT(r[j].item.id == full[j + CHUNKS].id && r[j].item.score == full[j + CHUNKS].score && r[j].group == PCV_NO_GROUP && r[j].collapsed == 0);
        EXPECT(s->search_vector_grouped({}, 10, emb[50]).empty());       // an empty filter matches nothing
        EXPECT(s->search_vector_grouped({1, 2}, 0, emb[50]).empty());    // room for nothing
    }
    {
        SearcherView v = s->view(even);
        const auto r = v.search_vector_grouped({1, 2}, 5, emb[50], 128);
        EXPECT(r.size() == 5 && r[0].item.id == 7050 && r[0].group == 9 && r[0].collapsed == CHUNKS / 2);
        for (const auto& it : r) EXPECT(it.item.id % 2 == 0);
    }
    s->clear_groups();
    {
        const auto r = s->search_vector_grouped({1, 2}, 10, emb[50]);
        EXPECT(r.size() == 10 && r[1].item.id == full[1].id && r[0].group == PCV_NO_GROUP);
    }
    if (failures) return 1;
    std::printf("grouped_mirror_test: ok\n");
    return 0;
}
