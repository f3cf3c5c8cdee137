"""The float64 encoder reference (tests/encoder_ref.py) is proved here, without a GPU, before any kernel is
compared with it: against the committed Hugging Face BertModel vectors, against the f32 C oracle, against
Hugging Face AlbertModel in double precision (tanh GELU, factorised embeddings, shared layers), and the
comparison helper is shown to notice one token row that is off by 1e-3."""
import os

import numpy as np
import pytest

import encoder_paths
import encoder_ref


def _weights(desc, seed):
    """Random weights at the library's synthetic scales (model.cpp fill_synthetic), f32."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in encoder_ref.tensor_shapes(desc).items():
        if "LayerNorm.weight" in name:
            a = 1.0 + 0.1 * rng.uniform(-1, 1, shape)
        elif name.endswith("bias"):
            a = 0.05 * rng.uniform(-1, 1, shape)
        elif name.startswith("embeddings."):
            a = 0.5 * rng.uniform(-1, 1, shape)
        else:
            a = 0.05 * rng.uniform(-1, 1, shape)
        w[name] = a.astype(np.float32)
    return w


def _ragged(rng, B, L, vocab):
    ids = rng.integers(1, vocab, (B, L)).astype(np.int64)
    mask = np.ones_like(ids)
    for b, n in enumerate(rng.integers(1, L + 1, B)):
        mask[b, n:] = 0
    mask[0, :] = 1
    if B > 1:
        mask[-1, 1:] = 0
    return ids * mask, mask


def test_reference_matches_the_hf_golden_vectors(golden_dir):
    # bounds: the measured 1.2e-7 / 1.1e-6 / 2.1e-6 with the golden's own f32 rounding as margin
    g = np.load(os.path.join(golden_dir, "encoder_tiny.npz"))
    v, h, ly, nh, it, mp = [int(x) for x in g["desc"]]
    desc = dict(vocab=v, hidden=h, layers=ly, heads=nh, inter=it, max_pos=mp, eps=1e-12, pooling=0, normalize=1)
    weights = {k[2:]: g[k] for k in g.files if k.startswith("w.")}
    out, hid = encoder_ref.forward(desc, weights, g["ids"], g["mask"])
    e_normed = np.abs(out - g["normed"]).max()
    mean, _ = encoder_ref.forward(dict(desc, normalize=0), weights, g["ids"], g["mask"])
    e_mean = np.abs(mean - g["mean"]).max()
    msk = g["mask"].astype(bool)
    e_hid = max(np.abs(hid[i][msk] - g["hidden"][i][msk]).max() for i in range(ly + 1))
    print(f"golden: normed {e_normed:.2e} mean {e_mean:.2e} hidden {e_hid:.2e}")
    assert e_normed < 1e-6 and e_mean < 5e-6 and e_hid < 1e-5


TINY = dict(vocab=300, hidden=128, layers=2, heads=4, inter=256, max_pos=64, eps=1e-12, pooling=0, normalize=1)


@pytest.mark.parametrize("variant", [dict(pooling=0, normalize=1), dict(pooling=0, normalize=0), dict(pooling=1, normalize=0),
                                     dict(pooling=2, normalize=0), dict(pooling=3, normalize=0), dict(pooling=2, normalize=1),
                                     dict(dense_out=64, dense_act=1, normalize=1), dict(dense_out=96, dense_act=0, normalize=0)],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()))
def test_reference_matches_the_c_oracle_tiny(oracle, variant):
    desc = dict(TINY, **variant)
    w = _weights(desc, 3)
    ids, mask = _ragged(np.random.default_rng(5), 6, 40, desc["vocab"])
    out, hid = encoder_ref.forward(desc, w, ids, mask)
    oout, ohid = oracle.encode_tokens(desc, w, ids, mask, want_hidden=True)
    e_out, e_hid = np.abs(out - oout).max(), np.abs(hid - ohid)[:, mask.astype(bool)].max()
    print(f"oracle tiny {variant}: out {e_out:.2e} (max|ref| {np.abs(out).max():.2f}) hidden {e_hid:.2e}")
    assert e_out < 1e-6 * max(1.0, np.abs(out).max()) and e_hid < 5e-5


def test_reference_matches_the_c_oracle_minilm_width(oracle):
    # 384 wide, 12 heads, FFN 1 536, 2 layers, 4 x 250 ragged; measured 1e-7 and 7.2e-6, hidden values up to about 4
    desc = dict(vocab=400, hidden=384, layers=2, heads=12, inter=1536, max_pos=256, eps=1e-12, pooling=0, normalize=1)
    w = _weights(desc, 7)
    ids, mask = _ragged(np.random.default_rng(8), 4, 250, desc["vocab"])
    out, hid = encoder_ref.forward(desc, w, ids, mask)
    oout, ohid = oracle.encode_tokens(desc, w, ids, mask, want_hidden=True)
    e_out, e_hid = np.abs(out - oout).max(), np.abs(hid - ohid)[:, mask.astype(bool)].max()
    print(f"oracle 384: out {e_out:.2e} hidden {e_hid:.2e} (max|hidden| {np.abs(hid).max():.2f})")
    assert e_out < 1e-6 and e_hid < 5e-5


def test_reference_matches_hf_albert_in_double_precision():
    # tanh GELU + factorised embeddings + shared layers: both sides float64, they differ in summation order only
    import torch
    from transformers import AlbertConfig, AlbertModel

    torch.manual_seed(13)
    cfg = AlbertConfig(vocab_size=300, embedding_size=128, hidden_size=256, num_hidden_layers=3, num_hidden_groups=1,
                       inner_group_num=1, num_attention_heads=4, intermediate_size=512, max_position_embeddings=64,
                       type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu_new", hidden_dropout_prob=0.0,
                       attention_probs_dropout_prob=0.0, classifier_dropout_prob=0.0, pad_token_id=0, bos_token_id=2, eos_token_id=3)
    hf = AlbertModel(cfg, add_pooling_layer=False).double().eval()
    with torch.no_grad():
        for k, v in hf.state_dict().items():
            if "LayerNorm.weight" in k or "layer_norm.weight" in k:
                v.copy_(1.0 + 0.2 * torch.randn_like(v))
            elif k.endswith("bias"):
                v.copy_(0.1 * torch.randn_like(v))
            elif v.dim() == 2:
                v.mul_(3.0)
    sd = {k: v.numpy() for k, v in hf.state_dict().items()}
    g = "encoder.albert_layer_groups.0.albert_layers.0."
    names = {"attention.self.query": "attention.query", "attention.self.key": "attention.key", "attention.self.value": "attention.value",
             "attention.output.dense": "attention.dense", "attention.output.LayerNorm": "attention.LayerNorm",
             "intermediate.dense": "ffn", "output.dense": "ffn_output", "output.LayerNorm": "full_layer_layer_norm"}
    w = {k: sd[k] for k in sd if k.startswith("embeddings.") and "position_ids" not in k and "token_type_ids" not in k}
    for k in ("weight", "bias"):
        w[f"encoder.embedding_hidden_mapping_in.{k}"] = sd[f"encoder.embedding_hidden_mapping_in.{k}"]
        for ours, theirs in names.items():
            w[f"encoder.layer.0.{ours}.{k}"] = sd[f"{g}{theirs}.{k}"]
    desc = dict(vocab=300, hidden=256, layers=3, heads=4, inter=512, max_pos=64, eps=1e-12, pooling=0, normalize=0,
                hidden_act=1, embedding_size=128, shared_layers=1)
    assert set(w) == set(encoder_ref.tensor_shapes(desc))
    ids, mask = _ragged(np.random.default_rng(2), 5, 47, 300)
    with torch.no_grad():
        r = hf(input_ids=torch.tensor(ids), attention_mask=torch.tensor(mask), output_hidden_states=True)
    out, hid = encoder_ref.forward(desc, w, ids, mask)
    live = mask.astype(bool)
    assert len(r.hidden_states) == 4
    e = max(np.abs(hid[i][live] - r.hidden_states[i].numpy()[live]).max() for i in range(4))
    print(f"HF albert, float64: hidden {e:.2e} (max|hidden| {np.abs(hid).max():.2f})")
    assert e < 1e-9


def test_the_comparison_notices_one_wrong_token_row():
    # the thin batch of case A.c (4 201 x 8 tokens, mean pooling, not normalised) at a narrow width: 1e-3 on ONE token row
    # of the last hidden state moves that sequence's output by 1e-3 / 8 = 1.25e-4, over the output bar
    case = next(c for c in encoder_paths.CASES if c["id"] == "A.c")
    assert case["L"] == 8 and case["desc"]["pooling"] == 0 and case["desc"]["normalize"] == 0
    desc = dict(case["desc"], hidden=128, heads=4, inter=128)
    w = _weights(desc, 1)
    ids, mask = encoder_paths.inputs(dict(case, B=40))
    out, hid = encoder_ref.forward(desc, w, ids, mask)
    fails, seen = encoder_ref.compare(out.astype(np.float32), hid.astype(np.float32), out, hid, mask)
    assert fails == [] and seen["out"] < 1e-6 and seen["hidden"] < 1e-6
    b, t = int(np.flatnonzero(mask.sum(1) == 8)[3]), 5  # a full-length row
    bad = hid.copy()
    bad[-1, b, t, :] += 1e-3
    fails, _ = encoder_ref.compare(out, hid, out, bad, mask)
    assert len(fails) == 1 and "hidden state 1" in fails[0]
    bad_out, _ = _pool_mean(bad[-1], mask), None
    assert np.isclose(np.abs(bad_out - out).max(), 1e-3 / mask[b].sum())
    fails, _ = encoder_ref.compare(out, None, bad_out, None, mask)
    assert len(fails) == 1 and f"output row {b}" in fails[0]


def _pool_mean(h, mask):
    m = mask.astype(np.float64)
    return (h * m[:, :, None]).sum(1) / np.maximum(m.sum(1, keepdims=True), 1e-9)
