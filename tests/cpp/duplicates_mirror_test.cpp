// Drives Searcher::find_duplicates / SearcherView::find_duplicates of the C++ host mirror (include/perceive.hpp) on the GPU: the
// planted copies of an item come back as pairs, best first, Gaussian rows pair with nothing, max_pairs cuts the list and leaves
// the total, a view joins only its own items, and pcv_duplicate_groups labels the group by its smallest id.
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
    const int D = 384, N = 2000, COPIES = 4;
    std::mt19937 rng(43);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    for (int i = 0; i < N; ++i)
        for (auto& v : emb[i]) v = nd(rng);
    // rows 100 .. 100 + COPIES - 1 are row 50 with a little noise (cosine about 0.9998, and 0.9996 among themselves)
    for (int c = 0; c < COPIES; ++c)
        for (int f = 0; f < D; ++f) emb[100 + c][f] = emb[50][f] + 0.02f * nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < N; ++i) {
        rows.push_back({7000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 2 == 0) even.push_back(7000 + i);
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const size_t group = COPIES + 1, all = group * (group - 1) / 2;
    {
        int64_t total = -1;
        const auto r = s->find_duplicates({1, 2}, 0.95f, 1000, &total);
        EXPECT(r.size() == all && total == (int64_t)all);
        for (size_t j = 0; j < r.size(); ++j) {
            EXPECT(r[j].id_a == 7050 || (r[j].id_a >= 7100 && r[j].id_a < 7100 + COPIES));
            EXPECT(r[j].id_b >= 7100 && r[j].id_b < 7100 + COPIES && r[j].id_a != r[j].id_b);
            EXPECT(r[j].score >= 0.95f && (j == 0 || r[j].score <= r[j - 1].score));
        }
        // the pairs with the original are the closest: one noise term instead of two
        for (size_t j = 0; j < (size_t)COPIES && j < r.size(); ++j) EXPECT(r[j].id_a == 7050);
        const auto cut = s->find_duplicates({1, 2}, 0.95f, 3, &total);
        EXPECT(cut.size() == 3 && total == (int64_t)all);
        for (size_t j = 0; j < cut.size(); ++j) EXPECT(cut[j].id_a == r[j].id_a && cut[j].id_b == r[j].id_b && cut[j].score == r[j].score);
        EXPECT(s->find_duplicates({}, 0.95f, 10, &total).empty() && total == 0);  // an empty filter matches nothing
        EXPECT(s->find_duplicates({1, 2}, 0.95f, 0).empty());                     // room for nothing
        // source 2 holds the odd rows: copies 101 and 103 only
        const auto odd = s->find_duplicates({2}, 0.95f, 10, &total);
        EXPECT(odd.size() == 1 && total == 1 && odd[0].id_a == 7101 && odd[0].id_b == 7103);

        std::vector<int64_t> a, b;
        for (const auto& pr : r) a.push_back(pr.id_a), b.push_back(pr.id_b);
        std::vector<int64_t> ids(2 * a.size()), label(2 * a.size());
        int64_t n = 0;
        check(pcv_duplicate_groups(a.data(), b.data(), (int64_t)a.size(), ids.data(), label.data(), (int64_t)ids.size(), &n));
        EXPECT(n == (int64_t)group);
        for (int64_t i = 0; i < n; ++i) EXPECT(label[(size_t)i] == 7050);
    }
    {
        SearcherView v = s->view(even);
        int64_t total = -1;
        const auto r = v.find_duplicates({1, 2}, 0.95f, 100, &total);  // 7050, 7100, 7102
        EXPECT(r.size() == 3 && total == 3);
        for (const auto& pr : r) EXPECT(pr.id_a % 2 == 0 && pr.id_b % 2 == 0);
    }
    if (failures) return 1;
    std::printf("duplicates_mirror_test: ok\n");
    return 0;
}
