"""What the linkage-tree tests share (test_linkage_cpu.py, test_linkage_gpu.py): the reference of pcv_searcher_linkage_tree, a
verifier for corpora too large for it, and the cut in plain Python.  A plain module, like density_ref.py, whose helpers it uses.

The weight of the edge {a, b} is orc_canonical_score(row_a, row_b, D, 0); an edge is BETTER than another iff its c is larger, then
its lower position is lower, then its higher position is lower.  reference() is Kruskal over every participating pair.  verify()
replays a returned tree best first: when edge i joins the components A and B of the edges before it, no other pair of A x B may be
better than edge i.  That is enough: a pair (x, y) outside the tree lies, when the worst edge e of the tree's path from x to y is
added, in the two components e joins (every other edge of the path is better and already in), so it is worse than e and with it
than every edge of the path — the cycle property, which only the Kruskal tree of a strict order has.  The pairs of A x B are screened
by an f64 product of unit rows and the oracle is asked about every pair within 1e-6 of c_i or above it (the argument of
duplicates_ref.reference: the two f64 computations differ by D * 2^-53 at most)."""
import ctypes as C

import numpy as np

from density_ref import canonical_norm2, takes_part

_FP = C.POINTER(C.c_float)
MAX_REFERENCE_ROWS = 700  # 245 000 oracle calls


def better(x, y):
    """(c, a, b) x is better than y"""
    return (-x[0], x[1], x[2]) < (-y[0], y[1], y[2])


def _pointers(rows):
    dim = rows.shape[1]
    return [C.cast(rows.ctypes.data + r * dim * 4, _FP) for r in range(rows.shape[0])]


class _Forest:
    """union-find whose roots are the lowest rows, with the members of every component (ascending arrays)"""

    def __init__(self, n):
        self.parent = list(range(n))
        self.members = {}

    def find(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def rows_of(self, root):
        m = self.members.get(root)
        return np.array([root], dtype=np.int64) if m is None else m

    def union(self, x, y):
        """x, y roots -> the members the two had"""
        ma, mb = self.rows_of(x), self.rows_of(y)
        lo, hi = min(x, y), max(x, y)
        self.parent[hi] = lo
        self.members.pop(hi, None)
        self.members[lo] = np.concatenate([ma, mb])
        return ma, mb


def reference(oracle, rows, ids, part=None):
    """-> (ids, part int8, pos_a, pos_b, id_a, id_b, c f64) as the call returns them.  part: bool per row, the rows a search could
    return (None: all)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    n, dim = rows.shape
    assert n <= MAX_REFERENCE_ROWS
    tp = takes_part(rows, part) if n else np.zeros(0, dtype=bool)
    live = np.nonzero(tp)[0].tolist()
    ptr = _pointers(rows)
    score = oracle.lib.orc_canonical_score
    pairs = [(-score(ptr[a], ptr[b], dim, 0), a, b) for i, a in enumerate(live) for b in live[i + 1:]]
    assert all(p[0] == p[0] and abs(p[0]) < np.inf for p in pairs)  # the graph is complete
    pairs.sort()
    forest = _Forest(n)
    tree = []
    for nc, a, b in pairs:
        x, y = forest.find(a), forest.find(b)
        if x != y:
            forest.parent[max(x, y)] = min(x, y)  # (the members are not kept here)
            tree.append((a, b, -nc))
            if len(tree) == len(live) - 1:
                break
    assert len(tree) == max(0, len(live) - 1)
    pos_a = np.array([t[0] for t in tree], dtype=np.int64)
    pos_b = np.array([t[1] for t in tree], dtype=np.int64)
    c = np.array([t[2] for t in tree], dtype=np.float64)
    return ids.copy(), tp.astype(np.int8), pos_a, pos_b, ids[pos_a], ids[pos_b], c


def verify(oracle, rows, part, edges):
    """edges: (pos_a, pos_b, c) of a returned tree; part: the returned out_part.  -> None if it is the tree of the definition,
    otherwise a sentence saying what is wrong with it"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    pos_a, pos_b, c = (np.asarray(e) for e in edges)
    part = np.asarray(part).astype(bool)
    if part.shape != (n,):
        return "part has %s entries for %d rows" % (part.shape, n)
    P = int(part.sum())
    if not len(pos_a) == len(pos_b) == len(c) == max(0, P - 1):
        return "%d edges for %d participating rows" % (len(c), P)
    ptr = _pointers(rows)
    score = oracle.lib.orc_canonical_score
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        U = rows.astype(np.float64) / np.sqrt(canonical_norm2(rows))[:, None] if n else rows.astype(np.float64)
    forest = _Forest(n)
    last = None
    for i, (a, b, ci) in enumerate(zip(pos_a.tolist(), pos_b.tolist(), c.tolist())):
        if not 0 <= a < b < n:
            return "edge %d: positions %d, %d" % (i, a, b)
        if not (part[a] and part[b]):
            return "edge %d has an end that takes no part" % i
        want = score(ptr[a], ptr[b], dim, 0)
        if np.float64(ci).view(np.uint64) != np.float64(want).view(np.uint64):
            return "edge %d: c %r, the oracle says %r" % (i, ci, want)
        e = (ci, a, b)
        if last is not None and not better(last, e):
            return "edge %d is not behind edge %d in the edge order" % (i, i - 1)
        last = e
        x, y = forest.find(a), forest.find(b)
        if x == y:
            return "edge %d closes a cycle: the edges are no spanning tree" % i
        A, B = forest.union(x, y)
        if len(A) > len(B):
            A, B = B, A
        G = (U[A] @ U.T)[:, B] if len(B) > 64 else U[A] @ U[B].T  # (one side is often a row or two: no copy of the other side's rows)
        for p, q in zip(*np.nonzero(G >= ci - 1e-6)):
            u, v = int(A[p]), int(B[q])
            u, v = min(u, v), max(u, v)
            if (u, v) == (a, b):
                continue
            f = (score(ptr[u], ptr[v], dim, 0), u, v)
            if better(f, e):
                return "edge %d (%d, %d, c %r) joins two components that the better pair (%d, %d, c %r) joins too" % (i, a, b, ci, u, v, f[0])
    return None


def cut(n, part, edges, threshold=-np.inf, min_clusters=1):
    """pcv_linkage_cut in plain Python -> (labels int32, clusters)"""
    pos_a, pos_b, c = edges
    part = np.ones(n, dtype=bool) if part is None else np.asarray(part).astype(bool)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    keep_below = len(c) - (int(min_clusters) - 1)
    for i in range(len(c)):
        if c[i] >= threshold and i < keep_below:
            x, y = find(int(pos_a[i])), find(int(pos_b[i]))
            if x != y:
                parent[max(x, y)] = min(x, y)
    labels = np.full(n, -1, dtype=np.int32)
    clusters = 0
    for r in range(n):
        if not part[r]:
            continue
        root = find(r)
        if root == r:
            labels[r] = clusters
            clusters += 1
        else:
            labels[r] = labels[root]
    return labels, clusters


def check(got, want, stats=None):
    """got: Searcher.linkage_tree's tuple; want: reference()'s.  Everything for equality, c by its bits."""
    names = ("ids", "part", "pos_a", "pos_b", "id_a", "id_b", "c")
    dtypes = (np.int64, np.int8, np.int64, np.int64, np.int64, np.int64, np.float64)
    print("rows %d/%d edges %d/%d" % (len(got[0]), len(want[0]), len(got[6]), len(want[6])))
    for name, dt, g, w in zip(names, dtypes, got, want):
        assert g.dtype == dt, name
        if name == "c":
            np.testing.assert_array_equal(g.view(np.uint64), w.view(np.uint64), err_msg=name)
        else:
            np.testing.assert_array_equal(g, w, err_msg=name)
    if stats is not None:
        P = int(want[1].sum())
        assert stats["rows"] == len(want[0]) and stats["participating"] == P and stats["edges"] == max(0, P - 1)
        assert stats["rounds"] >= 1 if P >= 2 else stats["rounds"] == 0
        assert stats["rounds"] <= max(0, int(np.ceil(np.log2(max(P, 1)))))
        assert stats["candidates"] >= stats["edges"]  # every edge was a candidate of the round that chose it


def check_verified(oracle, rows, ids, got, part=None, stats=None):
    """got against verify(): ids, part and the ids of the edges for equality, the tree by the verifier"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    g_ids, g_part, pos_a, pos_b, id_a, id_b, c = got
    np.testing.assert_array_equal(g_ids, ids)
    np.testing.assert_array_equal(g_part, takes_part(rows, part).astype(np.int8))
    assert c.dtype == np.float64 and pos_a.dtype == np.int64 and g_part.dtype == np.int8
    verdict = verify(oracle, rows, g_part, (pos_a, pos_b, c))
    assert verdict is None, verdict
    np.testing.assert_array_equal(id_a, ids[pos_a])
    np.testing.assert_array_equal(id_b, ids[pos_b])
    if stats is not None:
        P = int(g_part.sum())
        assert stats["rows"] == len(ids) and stats["participating"] == P and stats["edges"] == max(0, P - 1)
