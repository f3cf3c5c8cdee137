// Drives Searcher::search_vector_diverse / SearcherView::search_vector_diverse of the C++ host mirror (include/perceive.hpp) on the
// GPU and compares them with a plain C++ walk of its own over the list search_vector returns: the same picks in the same order, the
// same marginal values bit for bit (compile with -ffp-contract=off: the definition has no fused multiply-add).
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

// the canonical cosine of two f32 vectors: f64, products exact, sums in feature order
static double canonical_cosine(const std::vector<float>& a, const std::vector<float>& b) {
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (size_t f = 0; f < a.size(); ++f) {
        dot += (double)a[f] * (double)b[f];
        na += (double)a[f] * (double)a[f];
        nb += (double)b[f] * (double)b[f];
    }
    return dot / (std::sqrt(na) * std::sqrt(nb));
}

struct Pick {
    int64_t id;
    int rank;
    double marginal;
};
// greedy MMR over the first `pool` entries of `list` (ids 7000 + row), as include/perceive_hip.h defines it for the cosine metric
static std::vector<Pick> walk(const std::vector<SearchItem>& list, const std::vector<std::vector<float>>& emb, const std::vector<float>& query,
                              size_t k, float lambda, size_t pool) {
    const size_t n = std::min(pool, list.size());
    const double l = (double)lambda, u = 1.0 - l;
    std::vector<double> rel(n), div(n, 0.0);
    std::vector<char> picked(n, 0);
    for (size_t i = 0; i < n; ++i) rel[i] = canonical_cosine(emb[(size_t)(list[i].id - 7000)], query);
    std::vector<Pick> out;
    while (out.size() < std::min(k, n)) {
        int best = -1;
        double best_m = 0.0;
        for (size_t i = 0; i < n; ++i) {
            if (picked[i]) continue;
            const double x = l * rel[i];
            const double y = u * div[i];
            const double m = x - y;
            if (best < 0 || m > best_m) best = (int)i, best_m = m;
        }
        const bool first = out.empty();
        picked[(size_t)best] = 1;
        out.push_back({list[(size_t)best].id, best, best_m});
        for (size_t i = 0; i < n; ++i) {
            if (picked[i]) continue;
            const double c = canonical_cosine(emb[(size_t)(list[i].id - 7000)], emb[(size_t)(list[(size_t)best].id - 7000)]);
            if (first || c > div[i]) div[i] = c;
        }
    }
    return out;
}

static void same(const std::vector<DiverseItem>& got, const std::vector<Pick>& want, const std::vector<SearchItem>& list) {
    EXPECT(got.size() == want.size());
    for (size_t j = 0; j < got.size() && j < want.size(); ++j) {
        EXPECT(got[j].item.id == want[j].id && got[j].rank == want[j].rank && got[j].marginal == want[j].marginal);
        EXPECT(got[j].item.score == list[(size_t)want[j].rank].score);
    }
}

int main() {
    Context ctx(0);
    const int D = 384, N = 2000, COPIES = 6;
    std::mt19937 rng(43);
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
    const auto full = s->search_vector({1, 2}, 128, emb[50]);
    EXPECT(full.size() == 128 && full[0].id == 7050);
    {
        // a query near row 50 (cosine about 0.98): relevance and redundancy of a row differ, unlike for the row itself
        std::vector<float> near = emb[50];
        for (auto& v : near) v += 0.2f * nd(rng);
        const auto nfull = s->search_vector({1, 2}, 128, near);
        bool exact = true;
        const auto n = s->search_vector_diverse({1, 2}, 10, near, 0.5f, 128, &exact);
        same(n, walk(nfull, emb, near, 10, 0.5f, 128), nfull);
        // the copies of the item (ranks 1 .. COPIES) are not what a balanced walk wants next to the item itself
        EXPECT(n.size() == 10 && n[0].item.id == 7050 && n[0].rank == 0 && n[1].rank > COPIES && !exact);
        // the row itself as the query: every row's relevance IS its cosine with the first pick, all marginal values tie at 0
        const auto r = s->search_vector_diverse({1, 2}, 10, emb[50], 0.5f, 128);
        same(r, walk(full, emb, emb[50], 10, 0.5f, 128), full);
        EXPECT(r.size() == 10 && r[0].item.id == 7050 && r[0].rank == 0);
        // lambda = 1: the plain list
        const auto plain = s->search_vector_diverse({1, 2}, 10, emb[50], 1.0f);
        EXPECT(plain.size() == 10);
        for (size_t j = 0; j < plain.size(); ++j)
            EXPECT(plain[j].item.id == full[j].id && plain[j].item.score == full[j].score && plain[j].rank == (int)j);
        // the default pool (128 for ten results) and another lambda
        same(s->search_vector_diverse({1, 2}, 10, emb[50], 0.8f), walk(full, emb, emb[50], 10, 0.8f, 128), full);
        EXPECT(s->search_vector_diverse({}, 10, emb[50], 0.5f).empty());       // an empty filter matches nothing
        EXPECT(s->search_vector_diverse({1, 2}, 0, emb[50], 0.5f).empty());    // room for nothing
    }
    {
        SearcherView v = s->view(even);
        const auto vfull = v.search_vector({1, 2}, 64, emb[50]);
        const auto r = v.search_vector_diverse({1, 2}, 5, emb[50], 0.5f, 64);
        same(r, walk(vfull, emb, emb[50], 5, 0.5f, 64), vfull);
        EXPECT(r.size() == 5 && r[0].item.id == 7050);
        for (const auto& it : r) EXPECT(it.item.id % 2 == 0);
    }
    if (failures) return 1;
    std::printf("diverse_mirror_test: ok\n");
    return 0;
}
