"""The 6-bit screen at the benchmarked size: 100M x 384, 64 queries, top-10.  AUTO builds the 6-bit copy beside the int8 one
(sources of 8M rows and more); a 64-query pass under the AUTO kernel choice streams it in one launch and returns what the
whole-int8 scan (PCV_KERNEL_MFMA) returns, bit for bit."""
import numpy as np
import pytest

import perceive_amd as pa

pytestmark = pytest.mark.gpu

N = 100_000_000
D = 384
SEED = 0xC0FFEE


def test_headline_100m_b64_six_equals_int8(ctx, oracle):
    s = pa.Searcher(ctx, D, "cosine")
    s.add_synthetic(1, N, SEED)
    s.finalize()
    q = oracle.synth_rows(SEED + 9, 0, 64, D)
    q[:4] = oracle.synth_rows(SEED, 77_777_777, 4, D)  # rows planted by value
    s.set_kernel("auto")
    ids, sc, cnt = s.search_vectors(None, 10, q)
    st = s.last_stats()
    assert st["screening_copy"] == 2 and st["screen_bits"] == 6 and st["scan_launches"] == 1 and st["rows_scanned"] == N
    assert st["bytes_streamed"] == N * D * 3 // 4 + (N // 32) * 16  # 6-bit pieces + four constants per 32-row block
    assert st["narrow_survivors"] >= st["coarse_survivors"] > 0
    np.testing.assert_array_equal(ids[:4, 0], 77_777_777 + np.arange(4))
    s.set_kernel("mfma")  # the whole-int8 scan
    ids8, sc8, cnt8 = s.search_vectors(None, 10, q)
    assert s.last_stats()["screen_bits"] == 8 and s.last_stats()["bytes_streamed"] == N * D + (N // 32) * 4
    np.testing.assert_array_equal(ids, ids8)
    np.testing.assert_array_equal(sc, sc8)
    np.testing.assert_array_equal(cnt, cnt8)
    s.close()
