"""Which kernels one encoder forward launches, worked out on the CPU: a mirror of the host dispatch in
perceive_amd/csrc/encoder_kernels.hip (launch_gemm_f32_ln, launch_gemm_f32, launch_gemm_bf16x3, launch_gemm_f16x2,
launch_attention*, launch_layer_norm, launch_pool, launch_dense) and of launch_forward / forward in model.cpp.
TEST INFRASTRUCTURE ONLY: tests/test_encoder_paths_cpu.py checks that the tables below reach every label the
mirror can produce, tests/test_encoder_paths_gpu.py runs CASES against the float64 reference.

A label is a kernel with its template arguments and epilogue ("gemm_f32_kernel<EPI_BIAS>"); an edge label is
"<kernel>:<edge>" where the code has a distinct form (a partial last tile, a workgroup that walks several tiles,
...).  The mirror is a copy, so it can be wrong: the GPU test cross-checks its 32-row / 64-row LayerNorm-tile
threshold against the hardware (the two forms sum K in a different order, so their results differ in bits).

CASES was sized for a device with 256 CUs.
"""
import numpy as np

BM, BN, BN96, LBM, L32M = 128, 128, 96, 64, 32
GRAPH_TOKENS, DEBUG_TOKEN_LIMIT = 128, 16384  # model.cpp: kGraphTokens, kDebugTokenLimit
POOLS = ["mean", "cls", "max", "mean_sqrt_len"]

# every __global__ kernel of encoder_kernels.hip: the ones a forward can launch ...
FORWARD_KERNELS = {"gemm_f32_kernel", "gemm_f32_n96_kernel", "gemm_f32_ln_kernel", "gemm_f32_ln8_kernel", "gemm_f32_ln32_kernel",
                   "gemm_skinny_f32_kernel", "gemm_bf16x3_kernel", "gemm_bf16x3_ws_kernel", "gemm_f16x2_kernel",
                   "attention_f16_kernel", "attention_kernel", "attention_persist_kernel", "embed_ln_kernel",
                   "layer_norm_fixed_kernel", "layer_norm_kernel", "pool_kernel", "dense_kernel",
                   # (before a forward, when the weights changed: the bf16 / f16 planes of a split-precision mode)
                   "split_planes_kernel", "split_planes_f16_kernel"}
# ... and the ones that belong to something else, with where they are tested
OTHER_KERNELS = {"synth_weights_kernel": "model creation without a weight file; every synthetic-weight test reads its output back",
                 "chunk_argmax_kernel": "pcv_model_highlight (tests/test_highlight_gpu.py)"}


def _ceil(a, b):
    return (a + b - 1) // b


def _quarters(lab, name, M):
    """gemm epilogues on 128-row tiles (store_quarter): a partial last tile's 64-row quarters."""
    m = M % BM
    if m:
        lab.add(f"{name}:partial_last_tile")
        if m >= 64:
            lab.add(f"{name}:full_quarter")
        if m % 64:
            lab.add(f"{name}:partial_quarter")


def _gemm_f32(lab, M, N, K, epi, cus, env):
    if M <= 128 and K % 128 == 0:
        mt, nw = (1, 8) if M <= 32 else (2, 8) if M <= 64 else (4, 4)
        lab.add(f"gemm_skinny_f32_kernel<{epi},{mt},{nw}>")
        return
    if epi in ("EPI_BIAS", "EPI_BIAS_GELU") and N % BN96 == 0:
        mt = _ceil(M, BM)
        t128, t96 = mt * (N // BN), mt * (N // BN96)
        if "PCV_NO_N96" not in env and N % BN == 0 and 3 * _ceil(t96, cus) < 4 * _ceil(t128, cus):
            lab.add(f"gemm_f32_n96_kernel<{epi}>")
            if M % BM:
                lab.add("gemm_f32_n96_kernel:partial_last_tile")
            return
    lab.add(f"gemm_f32_kernel<{epi}>")
    _quarters(lab, "gemm_f32_kernel", M)


def _gemm(lab, compute, M, N, K, epi, cus, env):
    if compute == "bf16x3":
        if env.get("PCV_GEMM_WS", "")[:1] == "1":
            lab.add(f"gemm_bf16x3_ws_kernel<{epi}>")
            _quarters(lab, "gemm_bf16x3_ws_kernel", M)
            if (N // BN) * _ceil(M, BM) > cus:
                lab.add("gemm_bf16x3_ws_kernel:walk")
        else:
            lab.add(f"gemm_bf16x3_kernel<{epi}>")
            _quarters(lab, "gemm_bf16x3_kernel", M)
    elif compute == "f16x2":
        lab.add(f"gemm_f16x2_kernel<{epi},1>")
        _quarters(lab, "gemm_f16x2_kernel", M)
    else:
        _gemm_f32(lab, M, N, K, epi, cus, env)


def _gemm_f32_ln(lab, M, N, K, cus, env):
    """launch_gemm_f32_ln: False where the caller runs the projection and the LayerNorm as two kernels."""
    if M <= 128 or N not in (128, 256, 384) or K % 32:
        return False
    t32, t64 = _ceil(M, L32M), _ceil(M, LBM)
    if N == 384 and K % 64 == 0 and "PCV_NO_LN32" not in env:
        max32 = int(env["PCV_LN32_MAX_M"]) if "PCV_LN32_MAX_M" in env else -1
        if (M <= max32) if max32 >= 0 else 6 * _ceil(t32, cus) < 10 * _ceil(t64, cus):
            lab.add("gemm_f32_ln32_kernel<3>")
            if M % L32M:
                lab.add("gemm_f32_ln32_kernel<3>:partial_last_tile")
            if t32 > cus:
                lab.add("gemm_f32_ln32_kernel<3>:walk")
            return True
    if N == 384:
        lab.add("gemm_f32_ln8_kernel<3>")
        if M % LBM:
            lab.add("gemm_f32_ln8_kernel<3>:partial_last_tile")
            if M % LBM <= 32:
                lab.add("gemm_f32_ln8_kernel<3>:last_tile_le32_rows")
        if t64 > 2 * 256:
            lab.add("gemm_f32_ln8_kernel<3>:walk")
        return True
    lab.add(f"gemm_f32_ln_kernel<{N // 128}>")
    if M % LBM:
        lab.add(f"gemm_f32_ln_kernel<{N // 128}>:partial_last_tile")
    return True


def _layer_norm(lab, T, H):
    if T >= 64 and H in (384, 768, 1024):
        lab.add(f"layer_norm_fixed_kernel<{H // 64},2>")
    else:
        lab.add("layer_norm_kernel:T>=64" if T >= 64 else "layer_norm_kernel:T<64")


def _idle(lab, name, Lp, nw):
    if (Lp // 32) % nw:
        lab.add(f"{name}:idle_waves_in_last_workgroup")


def _attention_f16(lab, Lp, HD):
    if 2 * Lp * (HD * 2 + 16) + 2 * HD * (Lp * 2 + 16) > 150 * 1024:
        return False
    nw = 8 if Lp >= 256 else 4
    lab.add(f"attention_f16_kernel<{HD},{nw},2>")
    _idle(lab, f"attention_f16_kernel<{HD},{nw},2>", Lp, nw)
    return True


def _attention(lab, B, Lp, HD, heads, cus, env):
    lds = (2 * Lp * (HD + 4) + Lp) * 4
    if lds <= 150 * 1024:
        if Lp == 256 and HD == 64 and "PCV_ATTN_NO_PERSIST" not in env:
            lab.add("attention_persist_kernel<64,8,2,8,true>")
            per_cu = max(1, min(1, (160 * 1024) // lds))
            if B * heads > cus * per_cu:
                lab.add("attention_persist_kernel<64,8,2,8,true>:walk")
            return
        nw = 8 if Lp >= 256 else 4
        lab.add(f"attention_kernel<{HD},true,{nw},2>")
        _idle(lab, f"attention_kernel<{HD},true,{nw},2>", Lp, nw)
        return
    lab.add(f"attention_kernel<{HD},false>")
    _idle(lab, f"attention_kernel<{HD},false>", Lp, 4)


def paths(desc, B, L, compute, cus, env={}, calls=1):
    """The labels of what forward number `calls` of this (B, L) shape on one model launches."""
    lab = set()
    H, F, heads = desc["hidden"], desc["inter"], desc["heads"]
    E = desc.get("embedding_size", 0)
    T, Lp, HD = B * L, _ceil(L, 32) * 32, H // heads
    act = "EPI_BIAS_GELU_TANH" if desc.get("hidden_act", 0) == 1 else "EPI_BIAS_GELU"
    if compute == "bf16x3":
        lab.add("split_planes_kernel")
    elif compute == "f16x2":
        lab.add("split_planes_f16_kernel")
    lab.add("embed_ln_kernel")
    if E > 0:
        lab.add("embed_ln_kernel:narrow_embedding")
        _gemm(lab, compute, T, H, E, "EPI_BIAS", cus, env)
    if desc.get("shared_layers", 0) and desc["layers"] > 1:
        lab.add("shared_layers")
    _gemm(lab, compute, T, 3 * H, H, "EPI_BIAS", cus, env)
    if not (compute == "f16x2" and _attention_f16(lab, Lp, HD)):
        if compute == "f16x2":
            lab.add("f16_attention_fallback")
        _attention(lab, B, Lp, HD, heads, cus, env)
    fuse = compute == "f32" and "PCV_NO_FUSED_LN" not in env
    for K in (H, F):  # attention output, then FFN up + FFN down
        if K == F:
            _gemm(lab, compute, T, F, H, act, cus, env)
        if not (fuse and _gemm_f32_ln(lab, T, H, K, cus, env)):
            _gemm(lab, compute, T, H, K, "EPI_BIAS_RESIDUAL", cus, env)
            _layer_norm(lab, T, H)
    pool = "pool_kernel<8,8,8>" if H <= 512 else "pool_kernel<8,4,16>"
    dense = desc.get("dense_out", 0)
    lab.add(pool)
    lab.add(f"{pool}:{POOLS[desc.get('pooling', 0)]}")
    if H in (512, 1024):
        lab.add(f"{pool}:all_columns_of_a_lane")
    if dense > 0:
        lab.add("dense_kernel:" + ("tanh" if desc.get("dense_act", 0) == 1 else "identity"))
        if dense == 1024 or dense % 256:
            lab.add("dense_kernel:four_full_column_groups" if dense == 1024 else "dense_kernel:partial_column_group")
        if desc.get("normalize", 1):
            lab.add("dense_kernel:normalize")
    elif desc.get("normalize", 1):
        lab.add(f"{pool}:normalize")
    if T <= GRAPH_TOKENS and "PCV_NO_GRAPHS" not in env and calls >= 2:
        lab.add("graph_replay")
    return lab


# ------------------------------------------------------------------------------------------------
# the cases


def _desc(hidden, heads, inter, layers=1, max_pos=512, pooling="mean", normalize=0, dense_out=0, dense_act=0, act=0, emb=0,
          shared=0, vocab=400):
    return dict(vocab=vocab, hidden=hidden, layers=layers, heads=heads, inter=inter, max_pos=max_pos, eps=1e-12,
                pooling=POOLS.index(pooling), normalize=normalize, dense_out=dense_out, dense_act=dense_act, hidden_act=act,
                embedding_size=emb, shared_layers=shared)


def _case(cid, target, desc, B, L, compute="f32", mask="ragged", env=None, child=None, seed=None):
    return dict(id=cid, target=target, desc=desc, B=B, L=L, compute=compute, mask=mask, env=env or {}, child=child,
                seed=seed if seed is not None else 1 + sum(int(v) for v in desc.values()) % 97)  # (one set of weights per description)


def inputs(case):
    """ids and mask of a case.  ragged: row 0 full, the last row one live token, the others cut at random;
    hole: ragged, and row 0 has masked tokens in its middle; cut50: full rows except 50 random ones cut short."""
    B, L, vocab = case["B"], case["L"], case["desc"]["vocab"]
    rng = np.random.default_rng(case["seed"] * 7919 + B * 1000 + L)
    ids = rng.integers(1, vocab, (B, L)).astype(np.int64)
    mask = np.ones_like(ids)
    if case["mask"] == "cut50":
        for b in rng.choice(B, min(50, B // 2), replace=False):
            mask[b, rng.integers(1, L):] = 0
    else:
        for b, n in enumerate(rng.integers(1, L + 1, B)):
            mask[b, n:] = 0
        mask[0, :] = 1
        if B > 1:
            mask[-1, 1:] = 0
        if case["mask"] == "hole":
            mask[0, L // 3: L // 2] = 0
    return ids * mask, mask


def build_model(pa, ctx, desc, compute, seed):
    """A pa.Model of this description with the library's synthetic weights."""
    d = pa.make_desc(desc["vocab"], desc["hidden"], desc["layers"], desc["heads"], desc["inter"], desc["max_pos"],
                     layer_norm_eps=desc["eps"], pooling=POOLS[desc["pooling"]], normalize=bool(desc["normalize"]),
                     dense_out=desc["dense_out"], dense_activation="tanh" if desc["dense_act"] else "identity", compute=compute)
    d.hidden_act, d.embedding_size, d.shared_layers = desc["hidden_act"], desc["embedding_size"], desc["shared_layers"]
    return pa.Model(ctx, d, synthetic_seed=seed)


def run_model(model, case, ids, mask):
    """(output, hidden states of every layer or None above the debug token limit) of one forward."""
    B, L = ids.shape
    out = model.encode_tokens(ids, mask)
    hid = None
    if B * L <= DEBUG_TOKEN_LIMIT:
        hid = np.stack([model.debug_hidden(ly, B, L) for ly in range(case["desc"]["layers"] + 1)])
    return out, hid


def _build_cases():
    c = []
    LN8 = "gemm_f32_ln8_kernel<3>"
    minilm = dict(hidden=384, heads=12, inter=1536)
    # A: fused projection + LayerNorm, 64-row persistent form
    c.append(_case("A.a", LN8 + ":partial_last_tile", _desc(**minilm, layers=2), 33, 250))
    c.append(_case("A.b1", LN8 + ":last_tile_le32_rows", _desc(**minilm), 23, 359))
    c.append(_case("A.b2", "attention_kernel<32,true,8,2>:idle_waves_in_last_workgroup", _desc(**minilm), 27, 307))
    c.append(_case("A.c", LN8 + ":walk", _desc(384, 12, 256), 4201, 8, mask="cut50"))
    for B, L in ((3, 43), (5, 32), (7, 23), (6, 32), (1, 193)):
        c.append(_case(f"A.d{B * L}", LN8 + (":last_tile_le32_rows" if 0 < B * L % 64 <= 32 else ":partial_last_tile" if B * L % 64 else ""),
                       _desc(**minilm), B, L, env={"PCV_LN32_MAX_M": "0"}, child="A"))
    c.append(_case("A.d8192", LN8, _desc(**minilm, layers=2), 32, 256, env={"PCV_LN32_MAX_M": "0"}, child="A"))
    c.append(_case("A.d8250", LN8 + ":partial_last_tile", _desc(**minilm, layers=2), 33, 250, env={"PCV_LN32_MAX_M": "0"}, child="A"))
    # B: widths the suite never instantiated
    for H, heads in ((512, 8), (640, 20), (896, 14), (1024, 16), (1024, 32)):
        tag = f"B.{H}x{heads}"
        ln = "layer_norm_fixed_kernel<16,2>" if H == 1024 else "layer_norm_kernel:T>=64"
        c.append(_case(tag + ".210", ln, _desc(H, heads, 2 * H), 3, 70))
        c.append(_case(tag + ".40", "layer_norm_kernel:T<64", _desc(H, heads, 2 * H), 1, 40))
    c.append(_case("B.1024x16.210.bf16x3", "gemm_bf16x3_kernel:partial_quarter", _desc(1024, 16, 2048), 3, 70, "bf16x3"))
    c.append(_case("B.1024x16.40.bf16x3", "gemm_bf16x3_kernel:partial_last_tile", _desc(1024, 16, 2048), 1, 40, "bf16x3"))
    for H, heads in ((640, 20), (1024, 16)):
        for pooling, norm in (("max", 0), ("mean_sqrt_len", 0), ("mean", 1)):
            c.append(_case(f"B.{H}.{pooling}", "pool_kernel<8,4,16>:" + ("normalize" if norm else pooling),
                           _desc(H, heads, 2 * H, pooling=pooling, normalize=norm), 3, 70, mask="hole"))
    c.append(_case("B.1024.dense1024", "dense_kernel:four_full_column_groups", _desc(1024, 16, 2048, dense_out=1024, normalize=1), 3, 70))
    c.append(_case("B.1024.dense1000", "dense_kernel:partial_column_group", _desc(1024, 16, 2048, dense_out=1000, dense_act=1), 3, 70))
    # C: tanh GELU, factorised embeddings, shared layers
    albert = dict(hidden=256, heads=4, inter=512, layers=3, act=1, emb=128, shared=1)
    for compute in ("f32", "bf16x3", "f16x2"):
        g = {"f32": "gemm_f32_kernel", "bf16x3": "gemm_bf16x3_kernel", "f16x2": "gemm_f16x2_kernel"}[compute]
        e = "<EPI_BIAS_GELU_TANH,1>" if compute == "f16x2" else "<EPI_BIAS_GELU_TANH>"
        for B, L, f32_target in ((1, 5, "gemm_skinny_f32_kernel<EPI_BIAS_GELU_TANH,1,8>"), (1, 40, "gemm_skinny_f32_kernel<EPI_BIAS_GELU_TANH,2,8>"),
                                 (2, 50, "gemm_skinny_f32_kernel<EPI_BIAS_GELU_TANH,4,4>"), (4, 50, g + ":partial_quarter"), (4, 250, g + e)):
            target = f32_target if compute == "f32" or B * L > 128 else g + e
            c.append(_case(f"C.{compute}.{B * L}", target, _desc(**albert), B, L, compute))
    c.append(_case("C.768.300", "embed_ln_kernel:narrow_embedding", _desc(768, 12, 1536, act=1, emb=128, shared=1), 3, 100))
    # D: attention
    for compute in ("f32", "f16x2"):
        for L in (257, 300, 500, 512):
            k = "attention_kernel<32,true,8,2>" if compute == "f32" else "attention_f16_kernel<32,8,2>"
            c.append(_case(f"D.h32.{compute}.{L}", k + (":idle_waves_in_last_workgroup" if L < 500 else ""), _desc(256, 8, 512), 3, L, compute))
        for L in (513, 530):
            c.append(_case(f"D.h32.{compute}.{L}", "attention_kernel<32,false>" if compute == "f32" else "f16_attention_fallback",
                           _desc(256, 8, 512, max_pos=544), 3, L, compute))
    for L in (257, 300):
        c.append(_case(f"D.h64.f16x2.{L}", "f16_attention_fallback", _desc(256, 4, 512), 3, L, "f16x2"))
    for L in (225, 256):
        c.append(_case(f"D.nopersist.{L}", "attention_kernel<64,true,8,2>", _desc(256, 4, 512), 5, L, env={"PCV_ATTN_NO_PERSIST": "1"}, child="B"))
    # E: GEMM forms
    c.append(_case("E.plain128", "gemm_f32_kernel<EPI_BIAS>", _desc(256, 8, 512), 33, 128))
    for act in (0, 1):
        c.append(_case(f"E.ws.{'tanh' if act else 'erf'}", "gemm_bf16x3_ws_kernel:walk", _desc(**minilm, act=act), 18, 160, "bf16x3",
                       env={"PCV_GEMM_WS": "1"}, child="C"))
    c.append(_case("E.ws.partial_quarter", "gemm_bf16x3_ws_kernel:partial_quarter", _desc(**minilm), 17, 150, "bf16x3",
                   env={"PCV_GEMM_WS": "1"}, child="C"))
    return c


CASES = _build_cases()


def _old(where, desc, shapes, compute="f32", calls=1):
    return [dict(id=f"{where}[{B}x{L},{compute}]", desc=desc, B=B, L=L, compute=compute, env={}, calls=calls) for B, L in shapes]


def _build_old_cases():
    """The shapes of tests/test_encoder_gpu.py and of the checkpoint tests (tests/test_pretrained.py), as they stand."""
    o = []
    tiny = _desc(128, 4, 256, layers=2, max_pos=64, normalize=1, vocab=300)  # tests/golden/encoder_tiny.npz: hidden 128, 4 heads
    minilm = _desc(384, 12, 1536, layers=6, normalize=1, vocab=30522)
    o += _old("hf_golden_tiny", tiny, [(5, 24)]) + _old("hf_golden_tiny", dict(tiny, normalize=0), [(5, 24)])
    o += _old("ragged_lengths", tiny, [(7, 40), (1, 1), (1, 33), (1, 17)])
    for p in (1, 2, 3):
        o += _old("pooling_modes", dict(tiny, pooling=p, normalize=0), [(5, 24)])
    o += _old("dense_module", dict(tiny, dense_out=64, dense_act=1), [(5, 24)])
    o += _old("minilm_synthetic", minilm, [(4, 48)])
    o += _old("minilm_32_row_tiles", minilm, [(32, 256), (40, 200), (9, 100), (97, 250)])
    o += _old("head_dim_64_long", _desc(256, 4, 512, normalize=1, vocab=500), [(3, 300)])
    for compute in ("bf16x3", "f16x2"):
        o += _old("split_precision", tiny, [(5, 24)], compute) + _old("split_precision", minilm, [(5, 64)], compute)
    for compute in ("f32", "f16x2"):
        for heads, L in ((4, 77), (8, 40), (4, 200), (8, 129), (4, 256), (8, 250), (4, 250), (4, 225)):
            o += _old("attention_shapes", _desc(256, heads, 512, layers=2, max_pos=256, normalize=1), [(5, L)], compute)
    o += _old("wave_specialised", minilm, [(6, 160)], "bf16x3")
    o += [dict(id="wave_specialised[child]", desc=minilm, B=6, L=160, compute="bf16x3", env={"PCV_GEMM_WS": "1"}, calls=1)]  # (its child process)
    o += _old("persistent_attention", _desc(256, 4, 512, max_pos=256, normalize=1), [(72, 250)])
    for compute in ("f32", "bf16x3", "f16x2"):
        o += _old("bert_base_width", _desc(768, 12, 3072, layers=2, max_pos=128, pooling="cls", vocab=1000), [(3, 70)], compute)
    o += _old("skinny", _desc(256, 8, 512, layers=2, max_pos=64, normalize=1), [(1, 5), (1, 32), (2, 20), (3, 33), (8, 16), (5, 40)])
    o += _old("graph_replay", _desc(256, 8, 512, layers=2, max_pos=64, normalize=1), [(1, 12), (2, 7)], calls=4)
    o += _old("graph_replay", _desc(256, 8, 512, layers=2, max_pos=64, normalize=1), [(40, 60)])
    o += _old("split_precision", minilm, [(5, 64)])  # (its f32 comparison model)
    o += _old("workspace_reuse", _desc(128, 4, 256, layers=2, max_pos=128, normalize=1), [(4, 33), (4, 60), (1, 64), (9, 100), (2, 7)])
    for compute in ("f32", "bf16x3", "f16x2"):  # test_albert_checkpoint_matches_hf: 4 texts, the longest 48 tokens
        o += _old("albert_checkpoint", _desc(256, 4, 512, layers=3, max_pos=64, act=1, emb=128, shared=1, vocab=1000), [(4, 48)], compute)
    return o


OLD_CASES = _build_old_cases()

# labels no case reaches, each with its reason (the aim: nothing but the comparison switches PCV_NO_N96 and PCV_NO_GRAPHS,
# which add no kernel of their own and therefore no label)
UNREACHED = {}


def universe(cus):
    """Every label the mirror produces over the descriptions model_create accepts (each width with each head size it
    allows, both activations, factorised or not, the three compute modes, every pooling and dense form), token counts
    and lengths on both sides of every threshold in the dispatch, and the switches that select a kernel."""
    shapes = [(1, 1), (1, 32), (1, 33), (1, 64), (1, 65), (1, 128), (3, 43), (5, 32), (7, 23), (6, 32), (1, 193), (4, 50), (3, 70),
              (4, 250), (3, 225), (3, 256), (300, 256), (3, 257), (3, 300), (3, 500), (3, 512), (3, 513), (3, 530), (33, 128), (18, 160),
              (17, 150), (32, 256), (40, 200), (33, 250), (23, 359), (27, 307), (64, 256), (97, 250), (256, 256), (4201, 8), (2051, 32)]
    envs = [{}, {"PCV_GEMM_WS": "1"}, {"PCV_ATTN_NO_PERSIST": "1"}, {"PCV_LN32_MAX_M": "0"}]
    lab = set()
    for H in range(128, 1025, 128):
        for hd in (32, 64):
            for emb in (0, 128):
                for act in (0, 1):
                    for inter in (2 * H, 4 * H):
                        d = _desc(H, H // hd, inter, layers=2, max_pos=544, act=act, emb=emb, shared=emb > 0)
                        for compute in ("f32", "bf16x3", "f16x2"):
                            for env in envs:
                                for B, L in shapes:
                                    lab |= paths(d, B, L, compute, cus, env, calls=1 + (B * L <= 64))
    for H in (128, 512, 640, 1024):
        for pooling in POOLS:
            for norm in (0, 1):
                for dense_out, dense_act in ((0, 0), (64, 1), (256, 0), (1000, 1), (1024, 0)):
                    lab |= paths(_desc(H, H // 64, 2 * H, pooling=pooling, normalize=norm, dense_out=dense_out, dense_act=dense_act),
                                 3, 70, "f32", cus)
    return lab
