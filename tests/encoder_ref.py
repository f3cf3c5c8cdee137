"""Float64 numpy reference of the encoder forward (pcv_model_encode_tokens), TEST INFRASTRUCTURE ONLY.

`forward(desc, weights, ids, mask)` restates the graph of model.cpp's launch_forward for everything a
pcv_model_desc can express, in double precision and plain numpy:

  embeddings   word + position + token_type(0), LayerNorm at the embedding width; with
               `embedding_size > 0` that width is the narrow one and a Linear maps it up to hidden
  layers       QKV, softmax(QK^T / sqrt(head_dim) + (1 - mask) * -10000) V, projection + residual +
               LayerNorm, FFN up + GELU (erf, or 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))), FFN down +
               residual + LayerNorm; with `shared_layers` one set of weights runs `layers` times
  pooling      mean (sum(h m) / clamp_min(sum m, 1e-9)), cls, max (masked -> -1e9), mean_sqrt_len
  dense        optional Linear + identity | tanh
  normalise    x / clamp_min(||x||, 1e-12)

desc is a dict with the oracle's keys (vocab, hidden, layers, heads, inter, max_pos, eps, pooling, normalize,
dense_out, dense_act) plus hidden_act (0 erf, 1 tanh), embedding_size and shared_layers; weights are arrays
under the names `fetch_state_dict` returns (Model.state_dict()'s names, plus
encoder.embedding_hidden_mapping_in.* for a factorised embedding).
"""
import math

import numpy as np
from scipy.special import erf

POOL = {"mean": 0, "cls": 1, "max": 2, "mean_sqrt_len": 3}
OUT_BAR = 2e-5  # outputs: OUT_BAR * max(1, max|ref|) (tests/test_encoder_gpu.py)
HIDDEN_BAR = 1e-4  # hidden states of a 1-2 layer model, unmasked positions (tests/test_encoder_gpu.py)

_PER_LAYER = ["attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
              "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"]


def tensor_shapes(desc):
    """name -> shape of every tensor a model of this description owns."""
    H, F = desc["hidden"], desc["inter"]
    E = desc.get("embedding_size", 0) or H
    s = {"embeddings.word_embeddings.weight": (desc["vocab"], E),
         "embeddings.position_embeddings.weight": (desc["max_pos"], E),
         "embeddings.token_type_embeddings.weight": (desc.get("type_vocab", 2), E),
         "embeddings.LayerNorm.weight": (E,), "embeddings.LayerNorm.bias": (E,)}
    if desc.get("embedding_size", 0) > 0:
        s["encoder.embedding_hidden_mapping_in.weight"] = (H, E)
        s["encoder.embedding_hidden_mapping_in.bias"] = (H,)
    for i in range(1 if desc.get("shared_layers", 0) else desc["layers"]):
        p = f"encoder.layer.{i}."
        for n in _PER_LAYER:
            if "LayerNorm" in n:
                s[p + n + ".weight"] = (H,)
            elif n == "intermediate.dense":
                s[p + n + ".weight"] = (F, H)
            elif n == "output.dense":
                s[p + n + ".weight"] = (H, F)
            else:
                s[p + n + ".weight"] = (H, H)
            s[p + n + ".bias"] = (F,) if n == "intermediate.dense" else (H,)
    if desc.get("dense_out", 0) > 0:
        s["dense.linear.weight"] = (desc["dense_out"], H)
        s["dense.linear.bias"] = (desc["dense_out"],)
    return s


def fetch_state_dict(model, desc):
    """Every tensor of a pa.Model, shaped, through get_tensor (Model.state_dict() knows neither the factorised
    embedding's tensors nor that a shared-layer model holds one set of layer weights)."""
    return {n: model.get_tensor(n).reshape(shape) for n, shape in tensor_shapes(desc).items()}


def _layer_norm(x, w, b, eps):
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + eps) * w + b


def _gelu(x, tanh_form):
    if tanh_form:
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))
    return 0.5 * x * (1.0 + erf(x * math.sqrt(0.5)))


def _attention(q, k, v, add_mask, heads):
    B, L, H = q.shape
    hd = H // heads
    out = np.empty_like(q)
    step = max(1, (1 << 24) // (heads * L * L))  # score blocks of at most 128 MB
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        qh = q[sl].reshape(-1, L, heads, hd).transpose(0, 2, 1, 3)
        kh = k[sl].reshape(-1, L, heads, hd).transpose(0, 2, 3, 1)
        vh = v[sl].reshape(-1, L, heads, hd).transpose(0, 2, 1, 3)
        s = qh @ kh / math.sqrt(hd) + add_mask[sl, None, None, :]
        s -= s.max(-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(-1, keepdims=True)
        out[sl] = (p @ vh).transpose(0, 2, 1, 3).reshape(-1, L, H)
    return out


def forward(desc, weights, ids, mask):
    """Returns (out [B, out_dim], hidden [(layers + 1), B, L, hidden]), both float64."""
    w = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    ids = np.asarray(ids, np.int64)
    m = np.asarray(mask, np.float64)
    B, L = ids.shape
    eps = float(desc.get("eps", 1e-12))
    x = (w["embeddings.word_embeddings.weight"][ids] + w["embeddings.position_embeddings.weight"][:L][None]
         + w["embeddings.token_type_embeddings.weight"][0])
    h = _layer_norm(x, w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], eps)
    if desc.get("embedding_size", 0) > 0:
        h = h @ w["encoder.embedding_hidden_mapping_in.weight"].T + w["encoder.embedding_hidden_mapping_in.bias"]
    hidden = [h]
    add_mask = (1.0 - m) * -10000.0
    for ly in range(desc["layers"]):
        p = f"encoder.layer.{0 if desc.get('shared_layers', 0) else ly}."

        def lin(a, name):
            return a @ w[p + name + ".weight"].T + w[p + name + ".bias"]

        ctx = _attention(lin(h, "attention.self.query"), lin(h, "attention.self.key"), lin(h, "attention.self.value"),
                         add_mask, desc["heads"])
        h = _layer_norm(lin(ctx, "attention.output.dense") + h, w[p + "attention.output.LayerNorm.weight"],
                        w[p + "attention.output.LayerNorm.bias"], eps)
        ff = _gelu(lin(h, "intermediate.dense"), desc.get("hidden_act", 0) == 1)
        h = _layer_norm(lin(ff, "output.dense") + h, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps)
        hidden.append(h)
    pooling = desc.get("pooling", 0)
    den = np.maximum(m.sum(1, keepdims=True), 1e-9)
    if pooling == 1:
        pooled = h[:, 0, :]
    elif pooling == 2:
        pooled = np.where(m[:, :, None] != 0, h, -1e9).max(1)
    else:
        s = (h * m[:, :, None]).sum(1)
        pooled = s / np.sqrt(den) if pooling == 3 else s / den
    out = pooled
    if desc.get("dense_out", 0) > 0:
        out = pooled @ w["dense.linear.weight"].T + w["dense.linear.bias"]
        if desc.get("dense_act", 0) == 1:
            out = np.tanh(out)
    if desc.get("normalize", 1):
        out = out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12)
    return out, np.stack(hidden)


def compare(out, hidden, ref_out, ref_hidden, mask, out_bar=OUT_BAR, hidden_bar=HIDDEN_BAR):
    """Compares a forward's output [B, D] and (where given) hidden states [(layers + 1), B, L, H] with the
    reference's.  Returns (failures, observed): a list of messages, empty when everything is within its bar, and
    the largest errors seen: {"out": e, "out_bar": bar, "hidden": e}.  Hidden states count on unmasked positions."""
    failures, seen = [], {}
    ref_out = np.asarray(ref_out, np.float64)
    bar = out_bar * max(1.0, float(np.abs(ref_out).max()))
    d = np.abs(np.asarray(out, np.float64) - ref_out)
    seen["out"], seen["out_bar"] = float(d.max()), bar
    if not np.isfinite(d).all() or d.max() >= bar:
        r = int(np.nanargmax(d.max(1)))
        failures.append(f"output row {r}: error {d.max():.3e} >= {bar:.3e}")
    if hidden is not None:
        live = np.asarray(mask).astype(bool)
        worst = 0.0
        for ly in range(len(ref_hidden)):
            dh = np.abs(np.asarray(hidden[ly], np.float64) - ref_hidden[ly])[live]
            e = float(dh.max())
            worst = max(worst, e)
            if not np.isfinite(dh).all() or e >= hidden_bar:
                t = int(np.nanargmax(dh.max(1)))
                failures.append(f"hidden state {ly}, live token {t}: error {e:.3e} >= {hidden_bar:.3e}")
        seen["hidden"] = worst
    return failures, seen
