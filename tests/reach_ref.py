"""What the reach-tree tests share (test_reach_cpu.py, test_reach_gpu.py): the reference of pcv_searcher_reach_tree, a verifier for
corpora too large for it, and pcv_linkage_select in plain Python.  A plain module, like linkage_ref.py, whose helpers it uses.

c(a, b) is orc_canonical_score(row_a, row_b, D, 0).  core(r) is the j-th largest c(r, p) over the other participating rows,
j = min(min_items - 1, P - 1), +inf for j = 0, taken by sorting.  The weight of {a, b} is w = min(core(a), core(b), c(a, b)); an
edge is BETTER than another iff its w is larger, then its lower position is lower, then its higher position is lower.  reference()
is Kruskal over every participating pair.  verify() is linkage_ref.verify with w in the place of c: the pairs of A x B are screened
by an f64 product of unit rows, and since w <= c, a pair that could be better than edge i has c >= w_i.

select() follows pcv_linkage_select operation for operation: Python's float is the C double, and a * b + c in Python is two roundings,
as in the library, which is compiled with contraction off."""
import ctypes as C

import numpy as np

from density_ref import canonical_norm2, takes_part
from linkage_ref import _Forest, _pointers, better

MAX_REFERENCE_ROWS = 700


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def score_matrix(oracle, rows, live):
    """c of every pair of the rows `live` by the oracle -> [n, n] f64, NaN elsewhere and on the diagonal"""
    n, dim = rows.shape
    ptr = _pointers(rows)
    score = oracle.lib.orc_canonical_score
    G = np.full((n, n), np.nan)
    for i, a in enumerate(live):
        for b in live[i + 1:]:
            G[a, b] = G[b, a] = score(ptr[a], ptr[b], dim, 0)
    return G


def cores_of(G, live, min_items):
    """-> core [n] f64: NaN for the rows that take no part"""
    n = G.shape[0]
    P = len(live)
    j = min(int(min_items) - 1, P - 1)
    core = np.full(n, np.nan)
    for a in live:
        if j <= 0:
            core[a] = np.inf
        else:
            core[a] = np.sort(G[a, live][np.array(live) != a])[::-1][j - 1]
    return core


def reference(oracle, rows, ids, min_items, part=None, G=None):
    """-> (ids, part int8, core, pos_a, pos_b, id_a, id_b, w, c) as the call returns them.  part: bool per row, the rows a search
    could return (None: all).  G: score_matrix of these rows, if the caller has it"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    n, dim = rows.shape
    assert n <= MAX_REFERENCE_ROWS
    tp = takes_part(rows, part) if n else np.zeros(0, dtype=bool)
    live = np.nonzero(tp)[0].tolist()
    if G is None:
        G = score_matrix(oracle, rows, live)
    core = cores_of(G, live, min_items)
    pairs = []
    for i, a in enumerate(live):
        for b in live[i + 1:]:
            c = float(G[a, b])
            assert c == c and abs(c) < np.inf  # the graph is complete
            pairs.append((-min(float(core[a]), float(core[b]), c), a, b, c))
    pairs.sort(key=lambda t: t[:3])
    forest = _Forest(n)
    tree = []
    for nw, a, b, c in pairs:
        x, y = forest.find(a), forest.find(b)
        if x != y:
            forest.parent[max(x, y)] = min(x, y)
            tree.append((a, b, -nw, c))
            if len(tree) == len(live) - 1:
                break
    assert len(tree) == max(0, len(live) - 1)
    pos_a = np.array([t[0] for t in tree], dtype=np.int64)
    pos_b = np.array([t[1] for t in tree], dtype=np.int64)
    w = np.array([t[2] for t in tree], dtype=np.float64)
    c = np.array([t[3] for t in tree], dtype=np.float64)
    return ids.copy(), tp.astype(np.int8), core, pos_a, pos_b, ids[pos_a], ids[pos_b], w, c


NAMES = ("ids", "part", "core", "pos_a", "pos_b", "id_a", "id_b", "w", "c")
DTYPES = (np.int64, np.int8, np.float64, np.int64, np.int64, np.int64, np.int64, np.float64, np.float64)


def check(got, want, stats=None, min_items=None):
    """got: Searcher.reach_tree's tuple; want: reference()'s.  Everything for equality; core, w and c by their bits."""
    print("rows %d/%d edges %d/%d" % (len(got[0]), len(want[0]), len(got[7]), len(want[7])))
    for name, dt, g, w in zip(NAMES, DTYPES, got, want):
        assert g.dtype == dt, name
        if dt == np.float64:
            np.testing.assert_array_equal(bits(g), bits(w), err_msg=name)
        else:
            np.testing.assert_array_equal(g, w, err_msg=name)
    if stats is not None:
        P = int(want[1].sum())
        assert stats["rows"] == len(want[0]) and stats["participating"] == P and stats["edges"] == max(0, P - 1)
        assert stats["rounds"] >= 1 if P >= 2 else stats["rounds"] == 0
        assert stats["rounds"] <= max(0, int(np.ceil(np.log2(max(P, 1)))))
        assert stats["candidates"] >= stats["edges"]  # every edge was a candidate of the round that chose it
        if min_items is not None:
            assert stats["min_items"] == min_items
            j = min(min_items - 1, P - 1)
            assert stats["core_candidates"] >= max(j, 0) * P  # every row's j best were rescored


def oracle_cores(oracle, rows, part, min_items):
    """the cores of a corpus too large for score_matrix: the f64 Gram of unit rows picks every partner within 1e-6 of a row's j-th
    best (the two f64 computations differ by D * 2^-53 at most), the oracle scores those"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    part = np.asarray(part).astype(bool)
    live = np.nonzero(part)[0]
    P = len(live)
    j = min(int(min_items) - 1, P - 1)
    core = np.full(n, np.nan)
    if j <= 0:
        core[live] = np.inf
        return core
    ptr = _pointers(rows)
    score = oracle.lib.orc_canonical_score
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        U = rows.astype(np.float64) / np.sqrt(canonical_norm2(rows))[:, None]
    Ul = U[live]
    for lo in range(0, P, 1024):  # (a stretch of rows at a time: the whole Gram of a large corpus is too much memory)
        Gl = Ul[lo : lo + 1024] @ Ul.T
        for i in range(Gl.shape[0]):
            g = Gl[i]
            g[lo + i] = -np.inf
            a = int(live[lo + i])
            kth = np.partition(g, P - j)[P - j]  # the j-th largest
            near = np.nonzero(g >= kth - 1e-6)[0]
            exact = sorted((score(ptr[a], ptr[int(live[q])], dim, 0) for q in near), reverse=True)
            core[a] = exact[j - 1]
    return core


def check_verified(oracle, rows, ids, got, min_items, part=None, stats=None):
    """got against oracle_cores() and verify(): ids, part and the ids of the edges for equality, the cores by their bits, the tree by
    the verifier"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    g_ids, g_part, core, pos_a, pos_b, id_a, id_b, w, c = got
    np.testing.assert_array_equal(g_ids, ids)
    np.testing.assert_array_equal(g_part, takes_part(rows, part).astype(np.int8))
    assert w.dtype == c.dtype == core.dtype == np.float64 and pos_a.dtype == np.int64 and g_part.dtype == np.int8
    np.testing.assert_array_equal(bits(core), bits(oracle_cores(oracle, rows, g_part, min_items)), err_msg="core")
    verdict = verify(oracle, rows, g_part, core, (pos_a, pos_b, w, c))
    assert verdict is None, verdict
    np.testing.assert_array_equal(id_a, ids[pos_a])
    np.testing.assert_array_equal(id_b, ids[pos_b])
    if stats is not None:
        P = int(g_part.sum())
        assert stats["rows"] == len(ids) and stats["participating"] == P and stats["edges"] == max(0, P - 1)
        assert stats["rounds"] <= max(0, int(np.ceil(np.log2(max(P, 1))))) and stats["min_items"] == min_items


def verify(oracle, rows, part, core, edges):
    """edges: (pos_a, pos_b, w, c) of a returned tree; part, core: the returned out_part and out_core, core already checked against
    oracle_cores.  -> None if it is the tree of the definition, otherwise a sentence saying what is wrong with it"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    pos_a, pos_b, w, c = (np.asarray(e) for e in edges)
    part = np.asarray(part).astype(bool)
    P = int(part.sum())
    if not len(pos_a) == len(pos_b) == len(w) == len(c) == max(0, P - 1):
        return "%d edges for %d participating rows" % (len(w), P)
    ptr = _pointers(rows)
    score = oracle.lib.orc_canonical_score
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        U = rows.astype(np.float64) / np.sqrt(canonical_norm2(rows))[:, None] if n else rows.astype(np.float64)
    forest = _Forest(n)
    last = None
    for i, (a, b, wi, ci) in enumerate(zip(pos_a.tolist(), pos_b.tolist(), w.tolist(), c.tolist())):
        if not 0 <= a < b < n:
            return "edge %d: positions %d, %d" % (i, a, b)
        if not (part[a] and part[b]):
            return "edge %d has an end that takes no part" % i
        want_c = score(ptr[a], ptr[b], dim, 0)
        if bits([ci])[0] != bits([want_c])[0]:
            return "edge %d: c %r, the oracle says %r" % (i, ci, want_c)
        want_w = min(float(core[a]), float(core[b]), want_c)
        if bits([wi])[0] != bits([want_w])[0]:
            return "edge %d: w %r, the definition says %r" % (i, wi, want_w)
        e = (wi, a, b)
        if last is not None and not better(last, e):
            return "edge %d is not behind edge %d in the edge order" % (i, i - 1)
        last = e
        x, y = forest.find(a), forest.find(b)
        if x == y:
            return "edge %d closes a cycle: the edges are no spanning tree" % i
        A, B = forest.union(x, y)
        A, B = A[core[A] >= wi], B[core[B] >= wi]  # (a row whose core is below w_i has no edge as good as edge i)
        if len(A) > len(B):
            A, B = B, A
        if len(A) == 0:
            continue
        G = (U[A] @ U.T)[:, B] if len(B) > 64 else U[A] @ U[B].T
        for p, q in zip(*np.nonzero(G >= wi - 1e-6)):
            u, v = int(A[p]), int(B[q])
            u, v = min(u, v), max(u, v)
            if (u, v) == (a, b):
                continue
            f = (min(float(core[u]), float(core[v]), score(ptr[u], ptr[v], dim, 0)), u, v)
            if better(f, e):
                return "edge %d (%d, %d, w %r) joins two components that the better pair (%d, %d, w %r) joins too" % (i, a, b, wi, u, v, f[0])
    return None


def select(n, part, edges, min_cluster_size, allow_single=False):
    """pcv_linkage_select in plain Python, the same operations in the same order -> (labels int32, stability f64, size int64)"""
    pos_a, pos_b, w = ([int(x) for x in edges[0]], [int(x) for x in edges[1]], [float(x) for x in edges[2]])
    part = np.ones(n, dtype=bool) if part is None else np.asarray(part).astype(bool)
    E, M = len(w), int(min_cluster_size)
    assert M >= 2 and E == max(0, int(part.sum()) - 1)
    parent = list(range(n))
    top = list(range(n))
    size = [1] * (n + E)
    low = list(range(n)) + [0] * E
    left, right = [0] * E, [0] * E

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i in range(E):
        x, y = find(pos_a[i]), find(pos_b[i])
        assert x != y
        l, r = top[x], top[y]
        if low[r] < low[l]:
            l, r = r, l
        left[i], right[i] = l, r
        size[n + i] = size[l] + size[r]
        low[n + i] = low[l]
        parent[max(x, y)] = min(x, y)
        top[min(x, y)] = n + i

    c_parent, c_child, c_birth, c_stab = [], [], [], []
    row_cluster = [-1] * n

    def new_cluster(par, birth):
        c_parent.append(par)
        c_child.append(-1)
        c_birth.append(birth)
        c_stab.append(0.0)
        return len(c_parent) - 1

    def leave_all(node, cl):
        walk = [node]
        while walk:
            v = walk.pop()
            if v < n:
                row_cluster[v] = cl
            else:
                walk.append(left[v - n])
                walk.append(right[v - n])

    if E > 0:
        todo = [(n + E - 1, new_cluster(-1, w[E - 1]))]
        while todo:
            node, cl = todo.pop()
            while True:
                e = node - n
                l, r = left[e], right[e]
                nl, nr = size[l], size[r]
                rise = w[e] - c_birth[cl]
                if nl >= M and nr >= M:
                    c_stab[cl] = c_stab[cl] + float(nl + nr) * rise
                    a = new_cluster(cl, w[e])
                    b = new_cluster(cl, w[e])
                    c_child[cl] = a
                    todo.append((r, b))
                    todo.append((l, a))
                    break
                if nl < M and nr < M:
                    c_stab[cl] = c_stab[cl] + float(nl + nr) * rise
                    leave_all(node, cl)
                    break
                small, big = (l, r) if nl < M else (r, l)
                c_stab[cl] = c_stab[cl] + float(size[small]) * rise
                leave_all(small, cl)
                node = big

    K = len(c_parent)
    total, wins = [0.0] * K, [False] * K
    for q in range(K - 1, -1, -1):
        if c_child[q] < 0:
            total[q], wins[q] = c_stab[q], True
        else:
            tc = total[c_child[q]] + total[c_child[q] + 1]
            wins[q] = c_stab[q] >= tc
            total[q] = c_stab[q] if wins[q] else tc
    chosen = [-1] * K
    for q in range(K):
        if c_parent[q] >= 0 and chosen[c_parent[q]] >= 0:
            chosen[q] = chosen[c_parent[q]]
        elif wins[q] and (q != 0 or allow_single):
            chosen[q] = q
    labels = np.full(n, -1, dtype=np.int32)
    number, order, members = {}, [], []
    for r in range(n):
        q = chosen[row_cluster[r]] if row_cluster[r] >= 0 else -1
        if q < 0:
            continue
        if q not in number:
            number[q] = len(order)
            order.append(q)
            members.append(0)
        labels[r] = number[q]
        members[number[q]] += 1
    return labels, np.array([c_stab[q] for q in order], dtype=np.float64), np.array(members, dtype=np.int64)


def check_select(got, want):
    np.testing.assert_array_equal(got[0], want[0], err_msg="labels")
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg="stability")
    np.testing.assert_array_equal(got[2], want[2], err_msg="size")
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int64
