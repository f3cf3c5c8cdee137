// Drives Searcher::update_items / upsert_items of the C++ host mirror (include/perceive.hpp) on the GPU: an item's vector is
// replaced by a query's, so it becomes the best hit; an unknown id is appended by the upsert.  Expected values are recomputed with
// plain f64 loops.
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
    std::mt19937 rng(12);
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
    // item 5100 takes 2 * q (the largest dot product by far), item 424242 is new
    std::vector<float> upd(2 * D);
    for (int k = 0; k < D; ++k) {
        upd[k] = 2.0f * q[k];
        upd[D + k] = nd(rng);
    }
    std::vector<bool> found;
    EXPECT(s->update_items({5100, 424242}, upd, &found) == 1);
    EXPECT(found.size() == 2 && found[0] && !found[1]);
    auto hits = s->search_vector({1}, 3, q);
    EXPECT(hits.size() == 3 && hits[0].id == 5100);
    double qq = 0;
    for (int k = 0; k < D; ++k) qq += 2.0 * (double)q[k] * (double)q[k];
    EXPECT(!hits.empty() && std::fabs(hits[0].score - (float)std::max(0.0, 1.0 - qq / D)) < 1e-6f);
    EXPECT(s->num_rows() == N);  // in place
    const auto ur = s->upsert_items(1, {5100, 424242}, upd);
    EXPECT(ur.first == 1 && ur.second == 1);
    EXPECT(s->num_rows() == N + 1);
    hits = s->search_vector({1}, 2, std::vector<float>(upd.begin() + D, upd.end()));
    bool has_new = false;
    for (const auto& h : hits) has_new = has_new || h.id == 424242;
    EXPECT(has_new);
    bool threw = false;
    try {
        s->update_items({7, 7}, std::vector<float>(2 * D, 1.0f));  // the same id twice
    } catch (const Error&) {
        threw = true;
    }
    EXPECT(threw);
    if (failures) return 1;
    std::printf("update_mirror_test: ok\n");
    return 0;
}
