// Drives Searcher::remove_items of the C++ host mirror (include/perceive.hpp) on the GPU: items are removed from a searcher, and
// its searches are compared, id for id and score for score, with a searcher built fresh from the remaining rows.
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>

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
    const int D = 384, N = 3000;
    std::mt19937 rng(21);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    std::vector<EmbeddingRow> rows;
    for (int i = 0; i < N; ++i) {
        for (auto& v : emb[i]) v = nd(rng);
        rows.push_back({7000 + i, 1, serialize_embedding(emb[i])});
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Dot);
    // every 5th item, a run over several blocks, the first and the last item; one id twice, one that no row carries
    std::set<int64_t> gone;
    for (int i = 0; i < N; i += 5) gone.insert(7000 + i);
    for (int i = 1000; i < 1200; ++i) gone.insert(7000 + i);
    gone.insert(7000 + N - 1);
    std::vector<int64_t> ids(gone.begin(), gone.end());
    ids.push_back(7000);
    ids.push_back(999999);
    EXPECT(s->remove_items(ids) == (int64_t)gone.size());
    EXPECT(s->num_rows() == N - (int64_t)gone.size());
    EXPECT(s->remove_items(ids) == 0);  // they are gone
    std::vector<EmbeddingRow> rest;
    for (const auto& r : rows)
        if (!gone.count(r.item_id)) rest.push_back(r);
    auto fresh = Searcher::build(ctx, rest, D, Metric::Dot);
    for (int t = 0; t < 8; ++t) {
        std::vector<float> q(D);
        for (auto& v : q) v = nd(rng);
        const auto a = s->search_vector({1}, 20, q), b = fresh->search_vector({1}, 20, q);
        EXPECT(a.size() == 20 && a.size() == b.size());
        for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
            EXPECT(a[i].id == b[i].id && a[i].score == b[i].score);
            EXPECT(!gone.count(a[i].id));
        }
    }
    // a removed id is forgotten: added again it is a new item, and the best hit of its own vector
    s->upsert_items(1, {7000}, emb[0]);
    EXPECT(s->num_rows() == N - (int64_t)gone.size() + 1);
    const auto hits = s->search_vector({1}, 1, emb[0]);
    EXPECT(hits.size() == 1 && hits[0].id == 7000);
    if (failures) return 1;
    std::printf("remove_mirror_test: ok\n");
    return 0;
}
