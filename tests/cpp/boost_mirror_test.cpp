// Drives Searcher::search_vector_boosted and its SearcherView form of the C++ host mirror (include/perceive.hpp) on the GPU: a zero
// boost is the plain search; a step of 4.0 at value 5000 keeps exactly what search_vector_where keeps under "value >= 5000"; a view
// reads its parent's values.  The rows come from an integer hash that tests/test_boost_gpu.py repeats, and the result of one query
// under a rising boost is printed for it to compare with the Python call, bit for bit.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>

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

static float hashed(uint32_t i, uint32_t j) {
    uint32_t h = i * 2654435761u + j * 40503u + 12345u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    return (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;  // exact: a 24-bit integer over 2^24, less a half
}

int main() {
    Context ctx(0);
    const int D = 384, N = 1500;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) emb[i][j] = hashed((uint32_t)i, (uint32_t)j);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> ids, values;
    for (int i = 0; i < N; ++i) {
        rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 7 != 3) {  // (every seventh item stays without a value)
            ids.push_back(9000 + i);
            values.push_back(10 * (int64_t)i);
        }
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    s->set_values(ids, values);
    const auto full = s->search_vector({1, 2}, 128, emb[50]);
    EXPECT(full.size() == 128 && full[0].id == 9050);
    {  // a zero boost: the plain search, certified after one step
        Boost zero;
        zero.values = {0};
        zero.boosts = {0.0};
        bool exact = false;
        const auto r = s->search_vector_boosted({1, 2}, 10, emb[50], zero, 0, &exact);
        EXPECT(r.size() == 10 && exact);
        for (size_t j = 0; j < r.size(); ++j)
            EXPECT(r[j].item.id == full[j].id && r[j].item.score == full[j].score && r[j].rank == (int32_t)j && (float)r[j].boosted == full[j].score);
        EXPECT(r[0].value == 500 && s->search_vector_boosted({}, 10, emb[50], zero).empty() && s->search_vector_boosted({1, 2}, 0, emb[50], zero).empty());
    }
    {  // a tier: what has a value of 5000 or more comes first, in list order — search_vector_where's rows
        Boost tier;
        tier.values = {4999, 5000};
        tier.boosts = {0.0, 4.0};
        Where late;
        late.lo = 5000;
        bool exact = false;
        const auto r = s->search_vector_boosted({1, 2}, 10, emb[50], tier, 4096, &exact);
        const auto w = s->search_vector_where({1, 2}, 10, emb[50], late, 4096);
        EXPECT(r.size() == 10 && w.size() == 10 && exact);
        for (size_t j = 0; j < r.size() && j < w.size(); ++j)
            EXPECT(r[j].item.id == w[j].item.id && r[j].item.score == w[j].item.score && r[j].value == w[j].value && r[j].value >= 5000);
        // a view reads its parent's table and walks its own rows
        std::vector<int64_t> even;
        for (int i = 0; i < N; i += 2) even.push_back(9000 + i);
        SearcherView v = s->view(even);
        const auto vr = v.search_vector_boosted({1, 2}, 5, emb[50], tier, 4096);
        EXPECT(vr.size() == 5);
        for (const auto& x : vr) EXPECT(x.value >= 5000 && (x.item.id - 9000) % 2 == 0);
    }
    Boost rising;
    rising.values = {0, 15000};
    rising.boosts = {0.0, 0.05};
    rising.unset = 0.02;
    bool exact = false;
    const auto r = s->search_vector_boosted({1, 2}, 10, emb[77], rising, 128, &exact);
    EXPECT(r.size() == 10);
    for (const auto& x : r) {
        uint32_t sb;
        uint64_t mb;
        std::memcpy(&sb, &x.item.score, 4);
        std::memcpy(&mb, &x.boosted, 8);
        std::printf("row %" PRId64 " %" PRIu32 " %" PRIu64 " %" PRId64 " %d\n", x.item.id, sb, mb, x.value, (int)x.rank);
    }
    std::printf("exact %d\n", exact ? 1 : 0);
    if (failures) return 1;
    std::printf("boost_mirror_test: ok\n");
    return 0;
}
