"""The encoder's launch paths that tests/test_encoder_gpu.py never reaches, each against the float64 reference
(tests/encoder_ref.py): the whole batch's output, and every layer's hidden states on unmasked positions while the
batch is within the debug token limit.  The cases and the label each one exists for are tests/encoder_paths.py's CASES
(checked against the dispatch mirror without a GPU by tests/test_encoder_paths_cpu.py); they were sized for 256 CUs.

Bars, as in tests/test_encoder_gpu.py: outputs 2e-5 * max(1, max|ref|), hidden states of 1-2 layer models 1e-4 (the
shared-layer models run one layer's weights three times; same bar).  The f32 C oracle measures 1e-7 and 7e-6 against the
same reference.  Observed on an MI355X: outputs at most 1.0e-5 and 0.29 of their bar (case B.1024.dense1000), hidden states at most
1.1e-5; per group and per label in DESIGN.md, "Encoder launch paths".

The dispatch switches are read once per process: the three groups that need one run in a child process each
(tests/encoder_child.py), one at a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import encoder_paths as ep
import encoder_ref
import perceive_amd as pa

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

_weights = {}  # (description, seed) -> state dict, fetched once
_refs = {}  # (description, seed, B, L, mask kind) -> the reference's (out, hidden)


@pytest.fixture(scope="module")
def cus():
    # the attribute current_device_cus() reads, asked of torch in a process of its own: torch brings its own HIP runtime,
    # which finds no device once the library's runtime has opened it in this process
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    n = int(r.stdout.split()[-1])
    if n != 256:
        pytest.skip(f"the encoder path cases were sized for 256 CUs; this device has {n}")
    return n


def _key(case):
    return (tuple(sorted(case["desc"].items())), case["seed"])


def _reference(case, model=None, ctx=None):
    k = _key(case)
    if k not in _weights:
        m = model or ep.build_model(pa, ctx, case["desc"], "f32", case["seed"])
        _weights[k] = encoder_ref.fetch_state_dict(m, case["desc"])
        if model is None:
            m.close()
    rk = k + (case["B"], case["L"], case["mask"])
    if rk not in _refs:
        ids, mask = ep.inputs(case)
        _refs[rk] = encoder_ref.forward(case["desc"], _weights[k], ids, mask)
    return _refs[rk]


def _check(case, out, hid, ref):
    _, mask = ep.inputs(case)
    fails, seen = encoder_ref.compare(out, hid, ref[0], ref[1] if hid is not None else None, mask)
    print(f"ENCODER_PATHS {case['id']} target={case['target']} out={seen['out']:.3e} out_bar={seen['out_bar']:.3e} "
          f"hidden={seen.get('hidden', float('nan')):.3e}")
    assert fails == [], f"{case['id']}: " + "; ".join(fails)


def _run(ctx, case):
    try:
        m = ep.build_model(pa, ctx, case["desc"], case["compute"], case["seed"])
        ids, mask = ep.inputs(case)
        out, hid = ep.run_model(m, case, ids, mask)
    except (pa.PcvError, pa.ModelError) as e:  # a device error leaves nothing to run the later cases on
        pytest.exit(f"case {case['id']}: the library failed ({e}); nothing more is started on the device", returncode=3)
    ref = _reference(case, model=m)
    m.close()
    return out, hid, ref


@pytest.mark.parametrize("case", [c for c in ep.CASES if c["child"] is None], ids=lambda c: c["id"])
def test_path_matches_the_float64_reference(ctx, cus, case):
    assert case["target"] in ep.paths(case["desc"], case["B"], case["L"], case["compute"], cus, case["env"])
    out, hid, ref = _run(ctx, case)
    assert (hid is None) == (case["B"] * case["L"] > ep.DEBUG_TOKEN_LIMIT)
    _check(case, out, hid, ref)


def _children(tmp_path, which, timeout):
    """The cases of one child, run in a fresh process with their switch set: [(case, out, hidden)]."""
    cases = [c for c in ep.CASES if c["child"] == which]
    env = cases[0]["env"]
    assert all(c["env"] == env for c in cases)
    arrays = {"cases": json.dumps([dict(desc=c["desc"], compute=c["compute"], seed=c["seed"]) for c in cases])}
    for i, c in enumerate(cases):
        arrays[f"ids{i}"], arrays[f"mask{i}"] = ep.inputs(c)
    src, dst = str(tmp_path / "cases.npz"), str(tmp_path / "results.npz")
    np.savez(src, **arrays)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "encoder_child.py"), src, dst], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"encoder child {which} did not finish in {timeout} s; nothing more is started on the device: "
                    f"{(e.stderr or b'')[-800:]}", returncode=3)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"encoder child {which} ended on a signal ({r.returncode}); nothing more is started on the device: "
                    f"{r.stderr[-800:]}", returncode=3)
    assert r.returncode == 0, r.stderr[-800:]
    res = np.load(dst)
    return [(c, res[f"out{i}"], res[f"hid{i}"] if f"hid{i}" in res.files else None) for i, c in enumerate(cases)]


def test_child_a_64_row_layernorm_tiles_at_the_smallest_partial_tiles(ctx, cus, tmp_path):
    # PCV_LN32_MAX_M=0: the 64-row persistent form at 129 ... 193 tokens (the smallest partial tiles, the M - 1 clamps of the
    # residual prefetch), and the cross-check of the mirror's threshold: at 32 x 256 tokens the default is the 32-row
    # form (other bits), at 33 x 250 the default is the 64-row form itself (the same bits)
    results = _children(tmp_path, "A", timeout=180)
    for c, out, hid in results:
        assert c["target"] in ep.paths(c["desc"], c["B"], c["L"], c["compute"], cus, c["env"])
        _check(c, out, hid, _reference(c, ctx=ctx))
    by = {c["id"]: (c, out, hid) for c, out, hid in results}
    c, out, hid = by["A.d8192"]
    assert "gemm_f32_ln32_kernel<3>" in ep.paths(c["desc"], c["B"], c["L"], "f32", cus)
    dout, dhid, ref = _run(ctx, dict(c, env={}))
    _check(dict(c, id="A.d8192 (default: 32-row tiles)"), dout, dhid, ref)
    assert not np.array_equal(dhid, hid), "32 x 256 tokens: the default dispatch gave the 64-row form's bits"
    c, out, hid = by["A.d8250"]
    assert "gemm_f32_ln8_kernel<3>" in ep.paths(c["desc"], c["B"], c["L"], "f32", cus)
    dout, dhid, _ = _run(ctx, dict(c, env={}))
    np.testing.assert_array_equal(dhid, hid)
    np.testing.assert_array_equal(dout, out)


def test_child_b_staged_attention_without_the_persistent_form(ctx, cus, tmp_path):
    # PCV_ATTN_NO_PERSIST=1: attention_kernel<64, true, 8, 2> at 225 and 256 keys
    for c, out, hid in _children(tmp_path, "B", timeout=120):
        assert c["target"] in ep.paths(c["desc"], c["B"], c["L"], c["compute"], cus, c["env"])
        _check(c, out, hid, _reference(c, ctx=ctx))


def test_child_c_wave_specialised_bf16x3_gemm_walks_tiles(ctx, cus, tmp_path):
    # PCV_GEMM_WS=1 at 18 x 160 tokens: 276 FFN-up tiles for 256 workgroups, erf and tanh activation; 17 x 150 ends in a
    # partial quarter.  Same bits as the default kernel, and within the bars of the reference.
    for c, out, hid in _children(tmp_path, "C", timeout=180):
        assert c["target"] in ep.paths(c["desc"], c["B"], c["L"], c["compute"], cus, c["env"])
        _check(c, out, hid, _reference(c, ctx=ctx))
        dout, dhid, _ = _run(ctx, dict(c, env={}))
        np.testing.assert_array_equal(dout, out)
        np.testing.assert_array_equal(dhid, hid)
