"""bench.py --dump-outputs (no GPU needed: the writer is fed arrays shaped like a search call's result)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _result(B, k, seed=1):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 100_000_000, (B, k)).astype(np.int64)
    scores = rng.standard_normal((B, k)).astype(np.float32)
    counts = np.full(B, k, np.int32)
    return ids, scores, counts


def test_dump_writes_the_result_exactly(tmp_path):
    ids, scores, counts = _result(64, 10)
    _bench().dump_outputs(str(tmp_path / "out"), (ids, scores, counts))
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in ("ids", "scores", "counts")}
    assert sorted(os.listdir(tmp_path / "out")) == ["counts.npy", "ids.npy", "scores.npy"]
    assert got["ids"].dtype == np.float64 and (got["ids"].astype(np.int64) == ids).all()
    assert got["scores"].dtype == np.float32 and np.array_equal(got["scores"], scores)
    assert got["counts"].dtype == np.float64 and (got["counts"] == counts).all()


def test_dump_of_a_large_result_is_a_fixed_sample_within_64_mb(tmp_path):
    bench = _bench()
    B, k = 400_000, 16  # 400k x 16 x (8 + 4) B + 400k x 8 B = 80 MB
    res = _result(B, k)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES
    keep = np.load(tmp_path / "a" / "sampled_queries.npy").astype(np.int64)
    assert np.array_equal(keep, np.load(tmp_path / "b" / "sampled_queries.npy").astype(np.int64))
    assert len(np.unique(keep)) == len(keep) and 0 < len(keep) < B
    assert (np.load(tmp_path / "a" / "ids.npy").astype(np.int64) == res[0][keep]).all()
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), res[1][keep])
