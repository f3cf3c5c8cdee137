// Drives Searcher::search_compound, its SearcherView form and search_compound_like_items of the C++ host mirror
// (include/perceive.hpp) on the GPU: one wanted vector is the plain search; ANY of two vectors holds the best row of each; ALL never
// scores above either part; a weight of 0 makes the avoided vectors idle; the like-items form equals the vector form built from the
// same rows; a view walks its own rows.  The rows come from an integer hash that tests/test_compound_gpu.py repeats, and the result
// of one compound is printed for it to compare with the Python call, bit for bit.
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
    for (int i = 0; i < N; ++i) rows.push_back({9000 + i, 1 + i % 2, serialize_embedding(emb[i])});
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const auto full = s->search_vector({1, 2}, 10, emb[50]);
    EXPECT(full.size() == 10 && full[0].id == 9050);
    {  // one wanted vector: the plain search, in either mode
        Compound one;
        one.want = {emb[50]};
        for (CompoundMode mode : {CompoundMode::All, CompoundMode::Any}) {
            bool exact = false;
            const auto r = s->search_compound({1, 2}, 10, one, mode, 1.0f, 0, &exact);
            EXPECT(r.size() == 10 && exact);
            for (size_t j = 0; j < r.size() && j < full.size(); ++j)
                EXPECT(r[j].id == full[j].id && r[j].part_scores.size() == 1 && r[j].part_scores[0] == full[j].score && r[j].penalty == 0.0 &&
                       (float)r[j].combined == full[j].score);
        }
        EXPECT(s->search_compound({}, 10, one).empty() && s->search_compound({1, 2}, 0, one).empty());
    }
    Compound two;
    two.want = {emb[50], emb[60]};
    {  // ANY holds the best row of each part; ALL never scores above either part
        const auto any = s->search_compound({1, 2}, 10, two, CompoundMode::Any);
        EXPECT(any.size() == 10 && ((any[0].id == 9050 && any[1].id == 9060) || (any[0].id == 9060 && any[1].id == 9050)));
        const auto all = s->search_compound({1, 2}, 10, two, CompoundMode::All, 1.0f, 4096);
        EXPECT(all.size() == 10);
        for (const auto& x : all) EXPECT(x.part_scores.size() == 2 && (float)x.combined <= x.part_scores[0] && (float)x.combined <= x.part_scores[1]);
        // a weight of 0: the avoided vector is idle
        Compound with = two;
        with.avoid = {emb[70]};
        const auto idle = s->search_compound({1, 2}, 10, with, CompoundMode::All, 0.0f, 4096);
        EXPECT(idle.size() == all.size());
        for (size_t j = 0; j < idle.size() && j < all.size(); ++j) EXPECT(idle[j].id == all[j].id && idle[j].combined == all[j].combined && idle[j].penalty == 0.0);
        // the like-items form: the same vectors, built on the device from the stored rows
        const auto like = s->search_compound_like_items({1, 2}, 10, {{9050}, {9060}}, {}, CompoundMode::All, 1.0f, 4096, false);
        EXPECT(like.size() == all.size());
        for (size_t j = 0; j < like.size() && j < all.size(); ++j) EXPECT(like[j].id == all[j].id && like[j].combined == all[j].combined);
        const auto others = s->search_compound_like_items({1, 2}, 10, {{9050}, {9060}}, {}, CompoundMode::Any, 1.0f, 4096, true);
        EXPECT(others.size() == 10);
        for (const auto& x : others) EXPECT(x.id != 9050 && x.id != 9060);
        // a view walks its own rows
        std::vector<int64_t> even;
        for (int i = 0; i < N; i += 2) even.push_back(9000 + i);
        SearcherView v = s->view(even);
        const auto vr = v.search_compound({1, 2}, 5, two, CompoundMode::Any);
        EXPECT(vr.size() == 5);
        for (const auto& x : vr) EXPECT((x.id - 9000) % 2 == 0);
    }
    Compound c;
    c.want = {emb[77], emb[78]};
    c.avoid = {emb[79]};
    bool exact = false;
    const auto r = s->search_compound({1, 2}, 10, c, CompoundMode::All, 0.5f, 300, &exact);
    EXPECT(r.size() == 10);
    for (const auto& x : r) {
        uint64_t mb, pb;
        uint32_t s0, s1;
        std::memcpy(&mb, &x.combined, 8);
        std::memcpy(&pb, &x.penalty, 8);
        std::memcpy(&s0, &x.part_scores[0], 4);
        std::memcpy(&s1, &x.part_scores[1], 4);
        std::printf("row %" PRId64 " %" PRIu64 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", x.id, mb, s0, s1, pb);
    }
    std::printf("exact %d\n", exact ? 1 : 0);
    if (failures) return 1;
    std::printf("compound_mirror_test: ok\n");
    return 0;
}
