"""The encoder's dispatch mirror (tests/encoder_paths.py) and its case tables, checked without a GPU: every kernel
of encoder_kernels.hip is known to the mirror, every label the mirror can produce is reached by a case of the
suite at 256 CUs, and every case of CASES reaches the label it exists for."""
import os
import re

import encoder_paths as ep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256


def _reached():
    """label -> ids of the cases of CASES and OLD_CASES whose forward launches it."""
    by = {}
    for c in ep.CASES + ep.OLD_CASES:
        for lab in ep.paths(c["desc"], c["B"], c["L"], c["compute"], CUS, c["env"], c.get("calls", 1)):
            by.setdefault(lab, []).append(c["id"])
    return by


def test_every_kernel_of_the_encoder_is_known_to_the_mirror():
    src = open(os.path.join(ROOT, "perceive_amd", "csrc", "encoder_kernels.hip")).read()
    names = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    assert len(names) >= 20
    known = ep.FORWARD_KERNELS | set(ep.OTHER_KERNELS)
    assert names - known == set(), f"kernels the dispatch mirror does not classify: {sorted(names - known)}"
    assert known - names == set(), f"the mirror names kernels that are gone: {sorted(known - names)}"
    # and every forward kernel appears in some label of the universe
    labelled = {re.split(r"[<:]", lab)[0] for lab in ep.universe(CUS)}
    assert ep.FORWARD_KERNELS - labelled == set()


def test_every_label_is_reached_by_a_case():
    by = _reached()
    uni = ep.universe(CUS)
    assert set(by) - uni == set(), f"labels outside the universe: {sorted(set(by) - uni)}"
    print(f"{len(uni)} labels, {len(ep.CASES)} cases + {len(ep.OLD_CASES)} shapes of the earlier tests")
    new_only = 0
    for lab in sorted(uni):
        ids = by.get(lab, [])
        old = [i for i in ids if "[" in i]
        new_only += bool(ids) and not old
        print(f"  {lab:62s} {'(new) ' if ids and not old else ''}{', '.join(ids[:4])}{' ...' if len(ids) > 4 else ''}")
    print(f"{new_only} labels are reached by CASES only")
    missing = sorted(lab for lab in uni if lab not in by and lab not in ep.UNREACHED)
    assert missing == [], f"labels no case reaches: {missing}"
    stale = sorted(lab for lab in ep.UNREACHED if lab in by or lab not in uni)
    assert stale == [], f"listed as unreached, but reached or unknown: {stale}"


def test_every_case_reaches_the_label_it_exists_for():
    ids = [c["id"] for c in ep.CASES]
    assert len(set(ids)) == len(ids)
    for c in ep.CASES:
        got = ep.paths(c["desc"], c["B"], c["L"], c["compute"], CUS, c["env"])
        assert c["target"] in got, f"case {c['id']} ({c['B']} x {c['L']}, {c['compute']}) no longer reaches {c['target']}: {sorted(got)}"


# What has to stay covered, written out: the label, then hidden, heads, compute mode, B, L, hidden_act, pooling, normalize, dense_out
# and the switch it was asked for at.  Removing a case from CASES (or a retuned threshold) leaves its line unmet.
REQUIRED = """
gemm_f32_ln8_kernel<3>:partial_last_tile 384 12 f32 33 250 0 0 0 0
gemm_f32_ln8_kernel<3>:last_tile_le32_rows 384 12 f32 23 359 0 0 0 0
attention_kernel<32,true,8,2>:idle_waves_in_last_workgroup 384 12 f32 27 307 0 0 0 0
gemm_f32_ln8_kernel<3>:walk 384 12 f32 4201 8 0 0 0 0
gemm_f32_ln8_kernel<3>:last_tile_le32_rows 384 12 f32 3 43 0 0 0 0 PCV_LN32_MAX_M
gemm_f32_ln8_kernel<3>:last_tile_le32_rows 384 12 f32 5 32 0 0 0 0 PCV_LN32_MAX_M
gemm_f32_ln8_kernel<3>:partial_last_tile 384 12 f32 7 23 0 0 0 0 PCV_LN32_MAX_M
gemm_f32_ln8_kernel<3> 384 12 f32 6 32 0 0 0 0 PCV_LN32_MAX_M
gemm_f32_ln8_kernel<3>:last_tile_le32_rows 384 12 f32 1 193 0 0 0 0 PCV_LN32_MAX_M
gemm_f32_ln8_kernel<3> 384 12 f32 32 256 0 0 0 0 PCV_LN32_MAX_M
gemm_f32_ln8_kernel<3>:partial_last_tile 384 12 f32 33 250 0 0 0 0 PCV_LN32_MAX_M
layer_norm_kernel:T>=64 512 8 f32 3 70 0 0 0 0
layer_norm_kernel:T<64 512 8 f32 1 40 0 0 0 0
layer_norm_kernel:T>=64 640 20 f32 3 70 0 0 0 0
layer_norm_kernel:T<64 640 20 f32 1 40 0 0 0 0
layer_norm_kernel:T>=64 896 14 f32 3 70 0 0 0 0
layer_norm_kernel:T<64 896 14 f32 1 40 0 0 0 0
layer_norm_fixed_kernel<16,2> 1024 16 f32 3 70 0 0 0 0
layer_norm_kernel:T<64 1024 16 f32 1 40 0 0 0 0
layer_norm_fixed_kernel<16,2> 1024 32 f32 3 70 0 0 0 0
layer_norm_kernel:T<64 1024 32 f32 1 40 0 0 0 0
gemm_bf16x3_kernel:partial_quarter 1024 16 bf16x3 3 70 0 0 0 0
gemm_bf16x3_kernel:partial_last_tile 1024 16 bf16x3 1 40 0 0 0 0
pool_kernel<8,4,16>:max 640 20 f32 3 70 0 2 0 0
pool_kernel<8,4,16>:mean_sqrt_len 640 20 f32 3 70 0 3 0 0
pool_kernel<8,4,16>:normalize 640 20 f32 3 70 0 0 1 0
pool_kernel<8,4,16>:max 1024 16 f32 3 70 0 2 0 0
pool_kernel<8,4,16>:mean_sqrt_len 1024 16 f32 3 70 0 3 0 0
pool_kernel<8,4,16>:normalize 1024 16 f32 3 70 0 0 1 0
dense_kernel:four_full_column_groups 1024 16 f32 3 70 0 0 1 1024
dense_kernel:partial_column_group 1024 16 f32 3 70 0 0 0 1000
gemm_skinny_f32_kernel<EPI_BIAS_GELU_TANH,1,8> 256 4 f32 1 5 1 0 0 0
gemm_skinny_f32_kernel<EPI_BIAS_GELU_TANH,2,8> 256 4 f32 1 40 1 0 0 0
gemm_skinny_f32_kernel<EPI_BIAS_GELU_TANH,4,4> 256 4 f32 2 50 1 0 0 0
gemm_f32_kernel:partial_quarter 256 4 f32 4 50 1 0 0 0
gemm_f32_kernel<EPI_BIAS_GELU_TANH> 256 4 f32 4 250 1 0 0 0
gemm_bf16x3_kernel<EPI_BIAS_GELU_TANH> 256 4 bf16x3 1 5 1 0 0 0
gemm_bf16x3_kernel<EPI_BIAS_GELU_TANH> 256 4 bf16x3 1 40 1 0 0 0
gemm_bf16x3_kernel<EPI_BIAS_GELU_TANH> 256 4 bf16x3 2 50 1 0 0 0
gemm_bf16x3_kernel:partial_quarter 256 4 bf16x3 4 50 1 0 0 0
gemm_bf16x3_kernel<EPI_BIAS_GELU_TANH> 256 4 bf16x3 4 250 1 0 0 0
gemm_f16x2_kernel<EPI_BIAS_GELU_TANH,1> 256 4 f16x2 1 5 1 0 0 0
gemm_f16x2_kernel<EPI_BIAS_GELU_TANH,1> 256 4 f16x2 1 40 1 0 0 0
gemm_f16x2_kernel<EPI_BIAS_GELU_TANH,1> 256 4 f16x2 2 50 1 0 0 0
gemm_f16x2_kernel:partial_quarter 256 4 f16x2 4 50 1 0 0 0
gemm_f16x2_kernel<EPI_BIAS_GELU_TANH,1> 256 4 f16x2 4 250 1 0 0 0
embed_ln_kernel:narrow_embedding 768 12 f32 3 100 1 0 0 0
attention_kernel<32,true,8,2>:idle_waves_in_last_workgroup 256 8 f32 3 257 0 0 0 0
attention_kernel<32,true,8,2>:idle_waves_in_last_workgroup 256 8 f32 3 300 0 0 0 0
attention_kernel<32,true,8,2> 256 8 f32 3 500 0 0 0 0
attention_kernel<32,true,8,2> 256 8 f32 3 512 0 0 0 0
attention_kernel<32,false> 256 8 f32 3 513 0 0 0 0
attention_kernel<32,false> 256 8 f32 3 530 0 0 0 0
attention_f16_kernel<32,8,2>:idle_waves_in_last_workgroup 256 8 f16x2 3 257 0 0 0 0
attention_f16_kernel<32,8,2>:idle_waves_in_last_workgroup 256 8 f16x2 3 300 0 0 0 0
attention_f16_kernel<32,8,2> 256 8 f16x2 3 500 0 0 0 0
attention_f16_kernel<32,8,2> 256 8 f16x2 3 512 0 0 0 0
f16_attention_fallback 256 8 f16x2 3 513 0 0 0 0
f16_attention_fallback 256 8 f16x2 3 530 0 0 0 0
f16_attention_fallback 256 4 f16x2 3 257 0 0 0 0
f16_attention_fallback 256 4 f16x2 3 300 0 0 0 0
attention_kernel<64,true,8,2> 256 4 f32 5 225 0 0 0 0 PCV_ATTN_NO_PERSIST
attention_kernel<64,true,8,2> 256 4 f32 5 256 0 0 0 0 PCV_ATTN_NO_PERSIST
gemm_f32_kernel<EPI_BIAS> 256 8 f32 33 128 0 0 0 0
gemm_bf16x3_ws_kernel:walk 384 12 bf16x3 18 160 0 0 0 0 PCV_GEMM_WS
gemm_bf16x3_ws_kernel:walk 384 12 bf16x3 18 160 1 0 0 0 PCV_GEMM_WS
gemm_bf16x3_ws_kernel:partial_quarter 384 12 bf16x3 17 150 0 0 0 0 PCV_GEMM_WS
"""


def test_no_required_label_has_lost_its_case():
    have = set()
    for c in ep.CASES:
        d = c["desc"]
        for lab in ep.paths(d, c["B"], c["L"], c["compute"], CUS, c["env"]):
            have.add((lab, d["hidden"], d["heads"], c["compute"], c["B"], c["L"], d["hidden_act"], d["pooling"], d["normalize"],
                      d["dense_out"], ",".join(sorted(c["env"]))))
    lines = [ln.split() for ln in REQUIRED.strip().splitlines()]
    lost = [ln[0] + f" at hidden {ln[1]}, {ln[2]} heads, {ln[3]}, {ln[4]} x {ln[5]}" for ln in lines
            if (ln[0], int(ln[1]), int(ln[2]), ln[3], *map(int, ln[4:10]), ln[10] if len(ln) > 10 else "") not in have]
    assert lost == [], "labels that lost their case: " + "; ".join(lost)
    assert len(lines) == len(ep.CASES), "a case was added to CASES without its line in REQUIRED"
