"""What the density-cluster tests share (test_density_cpu.py, test_density_gpu.py): the reference of pcv_searcher_density_clusters
and the comparison with it.  A plain module, like duplicates_ref.py, whose corpus helpers the tests use beside it.

near(a, b) is orc_canonical_score(row_a, row_b, D, 0) >= (double)threshold, asked of the oracle for every pair of participating rows
whose f64 cosine by numpy is within 1e-6 of the threshold or above it (the argument of duplicates_ref.reference: the two f64
computations differ by D * 2^-53 at most, so a pair further below cannot reach the threshold in the oracle either).  Degrees, core
rows, components, their numbering, border rows and kinds follow the definition in include/perceive_hip.h, in plain Python."""
import ctypes as C

import numpy as np

NONE, NOISE, BORDER, CORE = -1, 0, 1, 2  # PCV_DENSITY_*

_FP = C.POINTER(C.c_float)
_CHUNK = 1024  # rows of one side of a Gram block


def canonical_norm2(rows):
    """|x|^2 in f64, products exact, summed in feature order"""
    r = np.ascontiguousarray(rows, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.cumsum(r * r, axis=1)[:, -1]


def takes_part(rows, part=None):
    """the rows with a cosine (canonical |x|^2 in [2^-126, inf)) among those a search could return (`part`: bool per row; None: all)"""
    n2 = canonical_norm2(rows)
    ok = (n2 >= 2.0 ** -126) & (n2 < np.inf)
    return ok if part is None else ok & np.asarray(part, dtype=bool)


def margin(dim):
    """selfjoin_margin(Dp) in f32 arithmetic (selfjoin_kernels.hip): the certified bound on |screening score - canonical cosine|"""
    dp = (dim + 15) // 16 * 16
    f = np.float32
    return float(f(0.00783) + f(1.02) * (f(dp + 16) * f(1.2e-7)) + f(1e-6))


def near_pairs(oracle, rows, threshold, live):
    """-> [(a, b, c)]: positions a < b of the rows `live` (ascending) with oracle cosine c >= (double)threshold"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    dim = rows.shape[1]
    thr = float(np.float32(threshold))
    live = np.asarray(live, dtype=np.int64)
    P = live.size
    out = []
    if P < 2:
        return out
    R = rows[live].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        U = R / np.sqrt(canonical_norm2(rows[live]))[:, None]  # (wild rows: exact enough for a 1e-6 window; the oracle decides)
    ptr = [C.cast(rows.ctypes.data + int(r) * dim * 4, _FP) for r in live]
    for lo_a in range(0, P, _CHUNK):
        hi_a = min(P, lo_a + _CHUNK)
        for lo_b in range(lo_a, P, _CHUNK):
            hi_b = min(P, lo_b + _CHUNK)
            G = U[lo_a:hi_a] @ U[lo_b:hi_b].T
            close = G >= thr - 1e-6
            if lo_a == lo_b:
                close = np.triu(close, k=1)
            for i, j in zip(*np.nonzero(close)):
                a, b = int(i) + lo_a, int(j) + lo_b
                c = oracle.lib.orc_canonical_score(ptr[a], ptr[b], dim, 0)
                if c >= thr:
                    out.append((int(live[a]), int(live[b]), c))
    return out


def cluster(n, live, pairs, min_items):
    """The definition on a graph: n positions, `live` those that take part, pairs [(a, b)] the near ones.
    -> (labels int32, kinds int8, degrees int32, clusters)"""
    part = np.zeros(n, dtype=bool)
    part[np.asarray(live, dtype=np.int64)] = True
    degrees = np.zeros(n, dtype=np.int32)
    adj = [[] for _ in range(n)]
    for a, b in pairs:
        assert a != b and part[a] and part[b]
        degrees[a] += 1
        degrees[b] += 1
        adj[a].append(b)
        adj[b].append(a)
    core = part & (degrees.astype(np.int64) + 1 >= int(min_items))
    labels = np.full(n, -1, dtype=np.int32)
    kinds = np.where(part, NOISE, NONE).astype(np.int8)
    clusters = 0
    for r in range(n):  # ascending position: a component is numbered when its first core row is met
        if not core[r] or labels[r] >= 0:
            continue
        labels[r] = clusters
        stack = [r]
        while stack:
            x = stack.pop()
            for y in adj[x]:
                if core[y] and labels[y] < 0:
                    labels[y] = clusters
                    stack.append(y)
        clusters += 1
    kinds[core] = CORE
    for r in range(n):
        if part[r] and not core[r]:
            near_core = [y for y in adj[r] if core[y]]
            if near_core:
                labels[r] = labels[min(near_core)]
                kinds[r] = BORDER
    return labels, kinds, degrees, clusters


def reference(oracle, rows, ids, threshold, min_items, part=None):
    """-> (ids, labels, kinds, degrees, clusters) by position, as the call returns them; reference.pairs: the near pairs"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    live = np.nonzero(takes_part(rows, part))[0]
    pairs = near_pairs(oracle, rows, threshold, live)
    labels, kinds, degrees, clusters = cluster(rows.shape[0], live, [(a, b) for a, b, _c in pairs], min_items)
    reference.pairs = pairs
    return np.asarray(ids, dtype=np.int64).copy(), labels, kinds, degrees, clusters


def check(got, want, stats=None):
    g_ids, g_labels, g_kinds, g_degrees, g_clusters = got
    w_ids, w_labels, w_kinds, w_degrees, w_clusters = want
    counts = {k: int((w_kinds == v).sum()) for k, v in (("core", CORE), ("border", BORDER), ("noise", NOISE))}
    print("rows %d/%d clusters %d/%d %s" % (len(g_ids), len(w_ids), g_clusters, w_clusters, counts))
    assert g_labels.dtype == np.int32 and g_kinds.dtype == np.int8 and g_degrees.dtype == np.int32 and g_ids.dtype == np.int64
    assert g_clusters == w_clusters
    np.testing.assert_array_equal(g_ids, w_ids)
    np.testing.assert_array_equal(g_degrees, w_degrees)
    np.testing.assert_array_equal(g_kinds, w_kinds)
    np.testing.assert_array_equal(g_labels, w_labels)
    if stats is not None:
        assert stats["rows"] == len(w_ids) and stats["participating"] == int((w_kinds != NONE).sum())
        assert stats["clusters"] == w_clusters
        for k, v in counts.items():
            assert stats[k] == v, (k, stats[k], v)
        # every near pair is found exactly once: by the screen alone, or in the band and confirmed
        assert 2 * (stats["sure_pairs"] + stats["confirmed"]) == int(w_degrees.astype(np.int64).sum())
        assert stats["confirmed"] <= stats["candidates"]
