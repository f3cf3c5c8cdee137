// Drives Searcher::seeds and SearcherView::seeds of the C++ host mirror (include/perceive.hpp) on the GPU with one case the Python
// test computed with its reference:
//     seeds_mirror_test <rows.f32> <n> <dim> <k> <method> <seed> <count> then per pick: <id> <position> <total> <cover bits, hex>
// The rows come from the raw little-endian f32 file, the ids are 5000 + 3 * position, everything in source 1.  Ids, positions, the
// int64 totals and the f32 bits of cover must be equal; then an empty filter, a first id, and a view of the even positions.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>

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

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const int n = std::atoi(argv[2]), dim = std::atoi(argv[3]), k = std::atoi(argv[4]), method = std::atoi(argv[5]);
    const uint64_t seed = std::strtoull(argv[6], nullptr, 10);
    const int count = std::atoi(argv[7]);
    if (argc != 8 + 4 * count) return 2;
    std::vector<float> all((size_t)n * dim);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(all.data(), sizeof(float), all.size(), f) != all.size()) return 2;
    std::fclose(f);

    Context ctx(0);
    std::vector<EmbeddingRow> rows;
    std::vector<int64_t> even;
    for (int i = 0; i < n; ++i) {
        rows.push_back({5000 + 3 * i, 1, serialize_embedding(std::vector<float>(all.begin() + (size_t)i * dim, all.begin() + (size_t)(i + 1) * dim))});
        if (i % 2 == 0) even.push_back(5000 + 3 * i);
    }
    auto s = Searcher::build(ctx, rows, dim, Metric::Cosine);
    const SeedItems got = s->seeds({1}, (size_t)k, (SeedMethod)method, seed);
    EXPECT((int)got.ids.size() == count && got.positions.size() == got.ids.size() && got.totals.size() == got.ids.size() && got.cover.size() == got.ids.size());
    for (int j = 0; j < count && j < (int)got.ids.size(); ++j) {
        const char* const* a = argv + 8 + 4 * j;
        EXPECT(got.ids[j] == std::strtoll(a[0], nullptr, 10));
        EXPECT(got.positions[j] == std::strtoll(a[1], nullptr, 10));
        EXPECT(got.totals[j] == std::strtoll(a[2], nullptr, 10));
        if (j == 0)
            EXPECT(std::isnan(got.cover[j]));
        else
            EXPECT(bits(got.cover[j]) == (uint32_t)std::strtoul(a[3], nullptr, 16));
    }
    const pcv_seed_stats st = s->last_seed_stats();
    EXPECT(st.rows == n && st.steps == count && st.method == method && st.participating == got.totals[0]);
    EXPECT(s->seeds({}, 3).ids.empty());   // an empty filter selects nothing
    EXPECT(s->seeds({2}, 3).ids.empty());  // ... and so does a source without rows
    const SeedItems first = s->seeds({1}, 2, SeedMethod::Farthest, 0, 5000 + 3 * 40);
    EXPECT(first.ids.size() == 2 && first.ids[0] == 5000 + 3 * 40 && first.positions[0] == 40);
    SearcherView v = s->view(even);
    const SeedItems vs = v.seeds({1}, 4, SeedMethod::Farthest);
    EXPECT(vs.ids.size() == 4 && vs.ids[0] == 5000);
    for (int64_t id : vs.ids) EXPECT((id - 5000) % 6 == 0);  // only the view's items
    EXPECT(v.last_seed_stats().rows == (int64_t)even.size());
    if (failures == 0) std::printf("seeds_mirror_test: ok\n");
    return failures == 0 ? 0 : 1;
}
