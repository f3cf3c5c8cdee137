// linkage_select.cpp — pcv_linkage_select (perceive_hip.h; DESIGN.md §4 "Reach tree"): HDBSCAN's condensed tree and excess-of-mass
// selection over the edges of a reach or linkage tree.  Host only: no context, no GPU.  A file of its own because of the pragma
// below: a stability is a chain of f64 subtract, multiply, add whose every rounding the definition fixes, so the compiler must not
// fuse a multiplication and an addition into one FMA anywhere in this file.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

using namespace pcv;

pcv_status pcv_linkage_select(const int64_t* pos_a, const int64_t* pos_b, const double* w, int64_t n_edges, const int8_t* part, int64_t n_rows,
                              int64_t min_cluster_size, int allow_single, int32_t* out_label, int32_t* out_clusters, double* out_stability,
                              int64_t* out_size, int64_t cluster_capacity) {
    return guarded([&] {
        PCV_REQUIRE(n_edges >= 0 && n_rows >= 0, "linkage_select: %lld edges, %lld rows", (long long)n_edges, (long long)n_rows);
        PCV_REQUIRE(n_edges == 0 || (pos_a != nullptr && pos_b != nullptr && w != nullptr), "linkage_select: %lld edges without their arrays",
                    (long long)n_edges);
        PCV_REQUIRE(n_rows == 0 || out_label != nullptr, "linkage_select: out_label is NULL");
        PCV_REQUIRE(n_rows <= (int64_t)INT32_MAX, "linkage_select: %lld rows do not fit the int32 labels", (long long)n_rows);
        PCV_REQUIRE(min_cluster_size >= 2, "linkage_select: min_cluster_size %lld is below 2", (long long)min_cluster_size);
        PCV_REQUIRE(cluster_capacity >= 0, "linkage_select: cluster_capacity %lld is negative", (long long)cluster_capacity);
        PCV_REQUIRE(cluster_capacity == 0 || out_stability != nullptr || out_size != nullptr, "linkage_select: cluster_capacity %lld without an array",
                    (long long)cluster_capacity);
        int64_t P = 0;
        for (int64_t r = 0; r < n_rows; ++r) P += (part == nullptr || part[r] != 0) ? 1 : 0;
        PCV_REQUIRE(n_edges == (P > 0 ? P - 1 : 0), "linkage_select: %lld edges do not span %lld participating rows", (long long)n_edges, (long long)P);

        // the dendrogram: node r < n_rows is row r, node n_rows + i is edge i; top[root of a component] is its node
        const size_t N = (size_t)n_rows, E = (size_t)n_edges;
        std::vector<int64_t> parent(N), top(N), left(E), right(E), size(N + E, 1), low(N + E);
        std::iota(parent.begin(), parent.end(), (int64_t)0);
        std::iota(top.begin(), top.end(), (int64_t)0);
        std::iota(low.begin(), low.begin() + (std::ptrdiff_t)N, (int64_t)0);
        auto find = [&](int64_t i) {
            while (parent[(size_t)i] != i) i = parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];
            return i;
        };
        for (int64_t i = 0; i < n_edges; ++i) {
            PCV_REQUIRE(pos_a[i] >= 0 && pos_a[i] < pos_b[i] && pos_b[i] < n_rows, "linkage_select: edge %lld joins positions %lld and %lld of %lld rows",
                        (long long)i, (long long)pos_a[i], (long long)pos_b[i], (long long)n_rows);
            PCV_REQUIRE(w[i] == w[i] && (i == 0 || w[i] <= w[i - 1]), "linkage_select: the edges are not ordered from best to worst at edge %lld", (long long)i);
            PCV_REQUIRE(part == nullptr || (part[pos_a[i]] != 0 && part[pos_b[i]] != 0), "linkage_select: edge %lld has an end that takes no part", (long long)i);
            const int64_t x = find(pos_a[i]), y = find(pos_b[i]);
            PCV_REQUIRE(x != y, "linkage_select: edge %lld closes a cycle", (long long)i);
            int64_t l = top[(size_t)x], r = top[(size_t)y];
            if (low[(size_t)r] < low[(size_t)l]) std::swap(l, r);
            const size_t node = N + (size_t)i;
            left[(size_t)i] = l;
            right[(size_t)i] = r;
            size[node] = size[(size_t)l] + size[(size_t)r];
            low[node] = low[(size_t)l];
            const int64_t root = std::min(x, y);
            parent[(size_t)std::max(x, y)] = root;
            top[(size_t)root] = (int64_t)node;
        }

        // the condensed tree, from the root down.  Cluster 0 is the root's; a cluster's children are made together, left then right.
        std::vector<int64_t> c_parent, c_child;  // c_child: the left child cluster (the right one is the next), -1: none
        std::vector<double> c_birth, c_stab;
        std::vector<int32_t> row_cluster(N, -1);  // the cluster a row was in when it left
        auto new_cluster = [&](int64_t par, double birth) {
            c_parent.push_back(par);
            c_child.push_back(-1);
            c_birth.push_back(birth);
            c_stab.push_back(0.0);
            return (int64_t)c_parent.size() - 1;
        };
        std::vector<int64_t> walk;  // nodes whose rows all leave one cluster: a stack of their own
        auto leave_all = [&](int64_t node, int64_t cl) {
            walk.push_back(node);
            while (!walk.empty()) {
                const int64_t v = walk.back();
                walk.pop_back();
                if (v < n_rows) {
                    row_cluster[(size_t)v] = (int32_t)cl;
                } else {
                    walk.push_back(left[(size_t)(v - n_rows)]);
                    walk.push_back(right[(size_t)(v - n_rows)]);
                }
            }
        };
        const int64_t M = min_cluster_size;
        if (n_edges > 0) {
            std::vector<std::pair<int64_t, int64_t>> todo;  // (node a cluster starts at, the cluster)
            todo.emplace_back((int64_t)(N + E - 1), new_cluster(-1, w[n_edges - 1]));
            while (!todo.empty()) {
                int64_t node = todo.back().first;
                const int64_t cl = todo.back().second;
                todo.pop_back();
                while (true) {  // node is an edge's: a cluster never goes on into a single row (M >= 2)
                    const int64_t e = node - n_rows;
                    const int64_t l = left[(size_t)e], r = right[(size_t)e];
                    const int64_t nl = size[(size_t)l], nr = size[(size_t)r];
                    const double rise = w[e] - c_birth[(size_t)cl];
                    if (nl >= M && nr >= M) {
                        c_stab[(size_t)cl] = c_stab[(size_t)cl] + (double)(nl + nr) * rise;
                        const int64_t a = new_cluster(cl, w[e]), b = new_cluster(cl, w[e]);
                        c_child[(size_t)cl] = a;
                        todo.emplace_back(r, b);
                        todo.emplace_back(l, a);
                        break;
                    }
                    if (nl < M && nr < M) {
                        c_stab[(size_t)cl] = c_stab[(size_t)cl] + (double)(nl + nr) * rise;
                        leave_all(node, cl);
                        break;
                    }
                    const int64_t small = nl < M ? l : r, big = nl < M ? r : l;
                    c_stab[(size_t)cl] = c_stab[(size_t)cl] + (double)size[(size_t)small] * rise;
                    leave_all(small, cl);
                    node = big;
                }
            }
        }

        // excess of mass, bottom-up (a child's number is above its parent's), then the selection from the top down
        const size_t K = c_parent.size();
        std::vector<double> total(K);
        std::vector<char> wins(K);
        for (size_t q = K; q-- > 0;) {
            if (c_child[q] < 0) {
                total[q] = c_stab[q];
                wins[q] = 1;
            } else {
                const double tc = total[(size_t)c_child[q]] + total[(size_t)c_child[q] + 1];
                wins[q] = c_stab[q] >= tc ? 1 : 0;
                total[q] = wins[q] ? c_stab[q] : tc;
            }
        }
        std::vector<int64_t> chosen(K, -1);  // the selected cluster that is q or an ancestor of it
        for (size_t q = 0; q < K; ++q) {
            if (c_parent[q] >= 0 && chosen[(size_t)c_parent[q]] >= 0)
                chosen[q] = chosen[(size_t)c_parent[q]];
            else if (wins[q] && (q != 0 || allow_single != 0))
                chosen[q] = (int64_t)q;
        }
        std::vector<int32_t> number(K, -1);
        std::vector<int64_t> members;
        std::vector<int64_t> order;
        for (int64_t r = 0; r < n_rows; ++r) {
            const int32_t cr = row_cluster[(size_t)r];
            const int64_t q = cr < 0 ? -1 : chosen[(size_t)cr];
            if (q < 0) {
                out_label[r] = -1;
                continue;
            }
            if (number[(size_t)q] < 0) {
                number[(size_t)q] = (int32_t)order.size();
                order.push_back(q);
                members.push_back(0);
            }
            out_label[r] = number[(size_t)q];
            members[(size_t)number[(size_t)q]] += 1;
        }
        for (size_t k = 0; k < order.size() && (int64_t)k < cluster_capacity; ++k) {
            if (out_stability) out_stability[k] = c_stab[(size_t)order[k]];
            if (out_size) out_size[k] = members[k];
        }
        if (out_clusters) *out_clusters = (int32_t)order.size();
    });
}
