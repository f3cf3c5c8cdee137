// Drives Searcher::set_values / values_of / count_where / search_vector_where / view_where and the SearcherView forms of the C++
// host mirror (include/perceive.hpp) on the GPU: with value = row number, "value >= 1000" keeps exactly the hits of search_vector
// that carry such a row, in its order and with its scores; the predicate view holds those rows and follows a later set_values.
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
    std::mt19937 rng(47);
    std::normal_distribution<float> nd;
    std::vector<std::vector<float>> emb(N, std::vector<float>(D));
    for (int i = 0; i < N; ++i)
        for (auto& v : emb[i]) v = nd(rng);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> ids, values;
    for (int i = 0; i < N; ++i) {
        rows.push_back({7000 + i, 1 + i % 2, serialize_embedding(emb[i])});
        if (i % 10 != 3) {  // (every tenth item stays without a value)
            ids.push_back(7000 + i);
            values.push_back(i);
        }
    }
    auto s = Searcher::build(ctx, rows, D, Metric::Cosine);
    const auto full = s->search_vector({1, 2}, 128, emb[50]);
    EXPECT(full.size() == 128 && full[0].id == 7050);
    Where late;
    late.lo = 1000;
    {  // no table yet: nothing has a value
        EXPECT(s->search_vector_where({1, 2}, 10, emb[50], late).empty());
        EXPECT(s->count_where({1, 2}, late) == 0);
        Where any = late;
        any.unset_passes = true;
        const auto plain = s->search_vector_where({1, 2}, 10, emb[50], any);
        EXPECT(plain.size() == 10);
        for (size_t j = 0; j < plain.size(); ++j)
            EXPECT(plain[j].item.id == full[j].id && plain[j].item.score == full[j].score && plain[j].value == PCV_NO_VALUE);
    }
    s->set_values(ids, values);
    {
        const auto got = s->values_of({7050, 7103, 7051, -1});
        EXPECT(got.size() == 4 && got[0] == 50 && got[1] == PCV_NO_VALUE && got[2] == 51 && got[3] == PCV_NO_VALUE);
        const pcv_value_stats st = s->value_stats();
        EXPECT(st.ids == (int64_t)ids.size() && st.entries == st.ids && st.slots >= 2 * st.entries);
        int64_t live = -1;
        EXPECT(s->count_where({1, 2}, late, &live) == 900 && live == 900);
        EXPECT(s->count_where({1}, late) == 500);  // source 1: the even rows, none of which is a 3 mod 10
        EXPECT(s->count_where({}, late) == 0);
        std::vector<SearchItem> want;  // the hits of the plain list that pass, in its order
        for (const auto& h : full)
            if (h.id - 7000 >= 1000 && (h.id - 7000) % 10 != 3) want.push_back(h);
        EXPECT(want.size() >= 10);
        bool more = true;
        const auto r = s->search_vector_where({1, 2}, 10, emb[50], late, 128, &more);
        EXPECT(r.size() == 10 && !more);
        for (size_t j = 0; j < r.size(); ++j)
            EXPECT(r[j].item.id == want[j].id && r[j].item.score == want[j].score && r[j].value == want[j].id - 7000);
        EXPECT(s->search_vector_where({}, 10, emb[50], late).empty());     // an empty filter matches nothing
        EXPECT(s->search_vector_where({1, 2}, 0, emb[50], late).empty());  // room for nothing
        // the predicate view: the same rows, found by a plain search of it
        SearcherView v = s->view_where(late);
        EXPECT(v.count_where({1, 2}, late) == 900);
        const auto vr = v.search_vector({1, 2}, 10, emb[50]);
        EXPECT(vr.size() == 10);
        for (size_t j = 0; j < vr.size(); ++j) EXPECT(vr[j].id == want[j].id && vr[j].score == want[j].score);
        const auto vw = v.search_vector_where({1, 2}, 3, emb[50], late);
        EXPECT(vw.size() == 3 && vw[0].item.id == want[0].id);
        // ... and it follows the values: item 7050 moves into the interval and comes first
        s->set_values({7050}, {5000});
        const auto moved = v.search_vector({1, 2}, 10, emb[50]);
        EXPECT(moved.size() == 10 && moved[0].id == 7050 && moved[1].id == want[0].id);
    }
    s->clear_values();
    EXPECT(s->search_vector_where({1, 2}, 10, emb[50], late).empty());
    if (failures) return 1;
    std::printf("where_mirror_test: ok\n");
    return 0;
}
