"""The gfx950 kernel SOURCES executed on the CPU (no GPU needed): chatterbox_amd/csrc/*.hip compiled for the x86 host against the SIMT
emulator of tests/simt/ (fibers per lane, MFMA / DPP / buffer-resource semantics of gfx950) and driven through the SAME C ABI and the SAME
`ops` wrappers as on the GPU -- by the SAME test bodies as `-m gpu` (tests/test_ops_gpu.py, tests/test_planes_gpu.py), called here with a
CPU device at shapes the emulator finishes in seconds.

What this pins without a GPU: index arithmetic, operand layouts (packed GEMV images, plane format, LDS swizzles, DMA addressing),
bounds handling, barriers and reductions, the epilogues, and the arithmetic to fp32 rounding.  What it cannot show: speed, memory-model
visibility, missing waits (simt_emu.h).  The emulator itself is pinned the other way round: every body below passes on the MI355X too.

Test infrastructure only: nothing under chatterbox_amd/ can reach the emulated library.
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


CPU = torch.device("cpu")

# (module, test function, arguments after `dev`)
_OPS = [
    ("test_linear", (1, 8, 16)), ("test_linear", (37, 80, 192)), ("test_linear", (40, 128, 1024)),
    ("test_linear_strided_accumulate_and_second_output", ()),
    ("test_swiglu", ()),
    ("test_conv1d", (32, 48, 3, 1, 1, 1, 77)), ("test_conv1d", (64, 64, 11, 5, 1, 25, 300)),
    ("test_conv1d_ragged_and_upsample", ()),
    ("test_conv_transpose", (32, 16, 11, 5, 3)),
    ("test_bmm", ()),
    ("test_layernorm_rmsnorm", ()),
    ("test_flash_attn", (103, 103, True)), ("test_flash_attn", (130, 130, False)), ("test_flash_attn_keys_from_the_kv_cache", ()),
    ("test_split_flash_attn", (130, 130, False, 3)), ("test_split_flash_attn", (103, 103, True, 6)), ("test_split_flash_attn", (130, 130, False, 16)),
    ("test_decode_attn", ()),
    ("test_softmax_relpos", ()),
    ("test_rope_and_kv_append", ()),
    ("test_elementwise", ()),
    ("test_sampler", (1.0, 0.05)), ("test_sampler", (0.9, 0.0)), ("test_sampler", (0.8, 0.05)),
    ("test_sampler_all_surviving_ids_banned", ()),
    ("test_hift_source_stft_istft", ()),
    ("test_gemv_decode", (16, 64, 256, 1, 4)), ("test_gemv_decode", (16, 1024, 1024, 4, 4)),
    ("test_gemv_swiglu", ()),
    ("test_decode_attn_rope_fused", ()), ("test_decode_attn_rope_split_context", (2, 16, True, 1)),
    ("test_gemv_packed_rms_fused", (16, 3072, 1024, False, 8)), ("test_gemv_packed_rms_fused", (16, 4096, 1024, True, 8)),
    ("test_gemv_packed_residual_epilogue", (16, 1024, 1024, 16)), ("test_gemv_packed_residual_epilogue", (7, 1024, 1024, 8)),
    ("test_gemv_packed_residual_epilogue", (16, 64, 256, 4)),
    ("test_gemv_partial_sum_operand", (9, 1024, 2, False)), ("test_gemv_partial_sum_operand", (16, 4096, 2, True)),
    ("test_gemv_partial_sum_operand", (16, 3072, 4, False)),
    ("test_decode_attn_packed_output_and_embed_packed", ()),
    ("test_gemv_layernorm_fused", (5, 2304, 768, 4, False)), ("test_gemv_layernorm_fused", (16, 4096, 1024, 0, True)),
    ("test_gemv_half_tile", (16, 1024, 4096, 2, 8, False)), ("test_gemv_half_tile", (16, 1024, 1024, 1, 8, True)), ("test_gemv_half_tile", (9, 40, 256, 1, 4, False)),
    ("test_gemv_bf16_weights_equal_rounded_fp32", ("plain",)), ("test_gemv_bf16_weights_equal_rounded_fp32", ("rms_np2",)),
    ("test_decode_attn_rope_pipelined_equals_plain", (3, 16, True, 512, 7, 4)), ("test_decode_attn_rope_pipelined_equals_plain", (1, 12, False, 1, 3, 4)),
    ("test_decode_attn_rope_pipelined_equals_plain", (1, 12, False, 1, 1, 8)),
    ("test_gemv_deep_batches_equal_plain", (16, 1024, 4096, 1, 4, True)), ("test_gemv_deep_batches_equal_plain", (9, 64, 2048, 1, 0, False)),
    ("test_gemv_narrow_tiles", (16, 3072, 1024, 1, 8, 12, "rms_np2")), ("test_gemv_narrow_tiles", (16, 1024, 4096, 1, 16, 4, "res")),
    ("test_gemv_narrow_tiles", (9, 1024, 4096, 1, 8, 4, "plain")), ("test_gemv_narrow_tiles", (5, 40, 256, 2, 4, 12, "plain")),
    ("test_gemv_narrow_tiles", (16, 1024, 4096, 1, 8, 4, "bf16")),
    ("test_gemv_col_tiles_and_split_k", (16, 3072, 1024, 3, 4, 2)), ("test_gemv_col_tiles_and_split_k", (16, 8194, 1024, 2, 1, 2)),
    ("test_gemv_col_tiles_and_split_k", (9, 200, 2048, 3, 2, 0)), ("test_gemv_col_tiles_and_split_k", (16, 3072, 1024, 3, 1, 4)),
    ("test_gemv_col_tiles_layernorm_form", (1, 6563, 1024, 2, 2)), ("test_gemv_col_tiles_layernorm_form", (5, 6563, 768, 2, 0)),
    ("test_decode_attn_folds_qkv_partial_sums", (5, 16, 2, 1)), ("test_decode_attn_folds_qkv_partial_sums", (2, 12, 4, 0)),
    ("test_flash_relpos_equals_materialised_scores", (2, 150, 2, (150, 70))), ("test_flash_relpos_equals_materialised_scores", (3, 33, 1, (33, 1, 0))),
    ("test_flash_relpos_equals_materialised_scores", (1, 300, 2, (257,))),
    ("test_gemv_row", (40, 256, "plain", 0)), ("test_gemv_row", (1030, 256, "ln", 3)), ("test_gemv_row", (70, 1024, "ln", 8)), ("test_gemv_row", (33, 768, "plain", 2)),
    ("test_gemv_row", (9, 4096, "plain", 0)), ("test_gemv_row", (256, 256, "attn", 1)), ("test_gemv_row", (50, 768, "attn", 2)),
    ("test_gemv_row_few_rows", (2, 70, 1024, "ln", 4)), ("test_gemv_row_few_rows", (4, 37, 256, "ln", 3)), ("test_gemv_row_few_rows", (3, 9, 4096, "plain", 2)),
    ("test_gemv_row_few_rows", (2, 64, 256, "attn", 2)), ("test_gemv_row_few_rows", (4, 50, 768, "attn", 1)),
    ("test_decode_attn_parts", (8, 4, False)), ("test_decode_attn_parts", (3, 2, True)), ("test_decode_attn_parts", (16, 8, False)),
]
_EPI = [("test_gemv_decode", (6, 64, 256, 1, 4)), ("test_gemv_decode", (16, 1024, 1024, 4, 4)), ("test_gemv_swiglu", ()),
        ("test_gemv_packed_residual_epilogue", (7, 1024, 1024, 8)), ("test_gemv_layernorm_fused", (5, 2304, 768, 4, False)),
        ("test_gemv_narrow_tiles", (16, 1024, 4096, 1, 16, 4, "res"))]


@pytest.mark.parametrize("name,args", _OPS, ids=[f"{n}{list(a)}" for n, a in _OPS])
def test_gpu_op_bodies_on_the_emulator(emu, name, args):
    import test_ops_gpu
    import test_zz_abi_v9_gpu
    getattr(test_ops_gpu if hasattr(test_ops_gpu, name) else test_zz_abi_v9_gpu, name)(CPU, *args)


@pytest.mark.parametrize("name,args", _EPI, ids=[f"{n}{list(a)}" for n, a in _EPI])
def test_gemv_epilogue_prefetch_on_the_emulator(emu, name, args, monkeypatch):
    import test_zz_abi_v9_gpu
    test_zz_abi_v9_gpu.test_gemv_epilogue_prefetch_equals_plain(CPU, name, args, monkeypatch)


# tests/test_wide_batch_decode_gpu.py (wide_batch_common.py: the decode forms above 16 rows): the kernel bodies in full (under a second each), and the Turbo engine
# body on both sides of the 16-row seam -- B = 17 is the 7-launch form, B = 16 the packed layer (11 s each; the larger batches are left to the GPU)
def _wide_batch_cases():
    import wide_batch_common as W
    cases = [("check_gemv_wide_rows_packed_weight", (M, *s)) for M in W.GEMV_M for s in W.GEMV_SHAPES]
    cases += [("check_add_norm_layernorm_wide", c) for c in W.ADD_NORM_CASES]
    return cases + [("check_turbo_engine_vs_oracle", (17,)), ("check_turbo_engine_vs_oracle", (16,))]


_WIDE = _wide_batch_cases()


@pytest.mark.parametrize("name,args", _WIDE, ids=[f"{n}{list(a)}" for n, a in _WIDE])
def test_wide_batch_decode_bodies_on_the_emulator(emu, name, args):
    import wide_batch_common as W
    getattr(W, name)(CPU, *args)


# tests/test_sampler_gpu.py and tests/test_frontend_ops_gpu.py at emulator sizes (the sampler: 10 utterances per launch, one seed, a reduced matrix that keeps both
# orders, cfg 0 / 1, dev_params, V < 1024, V not a multiple of 1024, the ties and the state machine)
_SAMPLER = [("test_sampler_matrix", (0, 10, 1, True)), ("test_sampler_matrix", (1, 10, 1, True)),
            ("test_sampler_dev_params_per_utterance", (0, 10, 704)), ("test_sampler_dev_params_per_utterance", (1, 10, 704)),
            ("test_sampler_state_machine", (0, 1)), ("test_sampler_state_machine", (1, 0)), ("test_sampler_state_machine", (1, 1)),
            ("test_sampler_no_mass_left_gives_the_best_allowed_raw_logit", (0,)), ("test_sampler_no_mass_left_gives_the_best_allowed_raw_logit", (1,))]
_FRONT = [("test_dwconv1d", (2, 50, 1280, 31, 15, 1)), ("test_dwconv1d", (5, 20, 8, 4, 0, 0)), ("test_dwconv1d", (5, 20, 4, 5, 4, 1)), ("test_dwconv1d", (5, 7, 8, 31, 15, 0)),
          ("test_dwconv1d", (3, 1, 4, 3, 1, 1)), ("test_dwconv1d", (5, 33, 12, 2, 1, 1)),
          ("test_lstm_cell", (1, 256)), ("test_lstm_cell", (5, 40)), ("test_affine_act", (4,)), ("test_affine_act", (128,)), ("test_affine_act", (1000,)),
          ("test_cplx_power", (201,)), ("test_cplx_power", (257,)), ("test_cplx_power", (513,)), ("test_cplx_power", (1,)), ("test_unary", ()), ("test_reduce_max", (False,)),
          ("test_seg_context_and_gate", (100,)), ("test_seg_context_and_gate", (37,)), ("test_stats_pool", (1,)), ("test_stats_pool", (3,)), ("test_stats_pool", (512,)),
          ("test_fsq_index", (2000,)), ("test_axpby", ()), ("test_add_norm_layernorm_form", (768, 1)), ("test_add_norm_layernorm_form", (1024, 2)),
          ("test_add_norm_layernorm_form", (768, 4)), ("test_softmax_rows", ()), ("test_hift_stft_ragged", ()), ("test_embed_negative_ids_and_scale", ()),
          ("test_act_kinds", (1 << 13,)), ("test_add_rmsnorm_first_abi_name", ()), ("test_flash_attn_plane_output", (130, False)), ("test_flash_attn_plane_output", (103, True))]


@pytest.mark.parametrize("name,args", _SAMPLER + _FRONT, ids=[f"{n}{list(a)}" for n, a in _SAMPLER + _FRONT])
def test_sampler_and_frontend_op_bodies_on_the_emulator(emu, name, args):
    import test_frontend_ops_gpu
    import test_sampler_gpu
    getattr(test_sampler_gpu if hasattr(test_sampler_gpu, name) else test_frontend_ops_gpu, name)(CPU, *args)


_PLANES = [("test_split_planes_roundtrip_and_range_flag", ()), ("test_layernorm_planes", ()), ("test_gemm_planes_transposed_rejects_bad_arguments", ()),
           ("test_range_flag_words_attribute_a_trip_to_the_batch_that_raised_it", ())]


@pytest.mark.parametrize("name,args", _PLANES, ids=[n for n, _ in _PLANES])
def test_gpu_planes_bodies_on_the_emulator(emu, name, args):
    import test_planes_gpu
    getattr(test_planes_gpu, name)(CPU, *args)


# tests/test_softmax_stress_gpu.py (prescribed scores: rescale, "no key seen yet", masks, merges of partial (m, l, O) triples) at emulator sizes: every kernel of
# that module at least once, the patterns asc / late_spike / two / neg / masked_spike, T <= 150, contexts <= 129
_CTX = (1, 17, 65, 129)
_STRESS = [("test_prefill_attention_stress", ("f32", "asc", [(150, 150, None), (150, 150, "causal")])), ("test_prefill_attention_stress", ("f32", "masked_spike", [(150, 150, "70"), (65, 65, "causal")])),
           ("test_prefill_attention_stress", ("kv", "late_spike", [(33, 65, "causal"), (130, 150, None)])), ("test_prefill_attention_stress", ("kv", "masked_spike", [(130, 150, "causal")])),
           ("test_prefill_attention_stress", ("p3", "asc", [(150, 150, None)])), ("test_prefill_attention_stress", ("p3", "two", [(150, 150, "70")])),
           ("test_prefill_attention_stress", ("p6", "late_spike", [(150, 150, None)])), ("test_prefill_attention_stress", ("p6", "masked_spike", [(150, 150, "causal")])),
           ("test_prefill_attention_stress", ("p16", "asc", [(150, 150, "causal")])), ("test_prefill_attention_stress", ("p16", "neg", [(65, 65, "0")])),
           ("test_prefill_attention_stress", ("po", "two", [(130, 130, None)])), ("test_prefill_attention_stress", ("po", "masked_spike", [(150, 150, "70")])),
           ("test_prefill_attention_stress", ("planes1", "asc", [(150, 150, "causal")])), ("test_prefill_attention_stress", ("planes2", "late_spike", [(150, 150, None)])),
           ("test_prefill_attention_stress", ("planes3", "two", [(150, 150, "70")])), ("test_prefill_attention_stress", ("planes4", "asc", [(150, 150, None)])),
           ("test_prefill_attention_stress", ("planes4", "masked_spike", [(150, 150, "70"), (65, 65, "0")])), ("test_prefill_attention_stress", ("planes5", "neg", [(130, 130, None)])),
           ("test_prefill_attention_stress", ("planes6", "late_spike", [(150, 150, "1")])),
           ("test_flash_relpos_stress", ("content", "asc", [(150, None)])), ("test_flash_relpos_stress", ("position", "two", [(150, "70")])),
           ("test_flash_relpos_stress", ("position", "masked_spike", [(65, "1")])),
           ("test_softmax_relpos_stress", ("content", "late_spike")), ("test_softmax_relpos_stress", ("position", "masked_spike")), ("test_softmax_rows_stress", ("two",)),
           ("test_softmax_rows_stress", ("neg",)),
           ("test_decode_attn_stress", (12, "asc", _CTX)), ("test_decode_attn_stress", (16, "masked_spike", _CTX)),
           ("test_decode_attn_rope_stress", (12, "none", "asc", _CTX)), ("test_decode_attn_rope_stress", (16, "quarter", "late_spike", _CTX)),
           ("test_decode_attn_rope_stress", (16, "identity", "two", _CTX)), ("test_decode_attn_rope_stress", (12, "quarter", "masked_spike", _CTX)),
           ("test_decode_attn_rope_stress", (12, "none", "neg", _CTX, ((3, 4),), (1,))),
           ("test_decode_attn_parts_stress", (12, "none", 2, 3, "two", _CTX)), ("test_decode_attn_parts_stress", (16, "quarter", 4, 8, "asc", _CTX)),
           ("test_decode_attn_parts_stress", (16, "identity", 8, 2, "masked_spike", _CTX)), ("test_decode_attn_parts_stress", (12, "quarter", 4, 16, "late_spike", _CTX))]


@pytest.mark.parametrize("name,args", _STRESS, ids=[f"{n}{list(a)}" for n, a in _STRESS])
def test_softmax_stress_bodies_on_the_emulator(emu, name, args):
    import test_softmax_stress_gpu
    getattr(test_softmax_stress_gpu, name)(CPU, *args)


# tests/test_norm_stress_gpu.py (prescribed rows: large offsets, one outlier channel, zero variance) at emulator sizes: every kernel of that module at least once at its
# smallest C / K / N, the patterns offset1024 / outlier_first / constant for each
_NSP = ("offset1024", "outlier_first", "constant")
_NORMSTRESS = [("test_layernorm_stress", (80, 37, _NSP)), ("test_layernorm_stress", (256, 77, _NSP)), ("test_row_stats_stress", (37, _NSP)),
               ("test_layernorm_planes_stress", (37, _NSP)), ("test_gemm_planes_layernorm_epilogue_stress", (False, 37, _NSP)),
               ("test_gemm_planes_layernorm_epilogue_stress", (True, 37, _NSP)), ("test_add_norm_stress", (768, 1, 5, _NSP)), ("test_add_norm_stress", (768, 4, 5, _NSP)),
               ("test_gemv_rms_fold_stress", (5, _NSP)), ("test_gemv_rms_fold_split_k_into_attention_stress", (5, _NSP)),
               ("test_gemv_layernorm_fold_stress", (768, 70, 5, _NSP)), ("test_gemv_layernorm_fold_stress", (768, 70, 1, _NSP)), ("test_gemv_layernorm_fold_stress", (768, 70, 33, _NSP)),
               ("test_gemv_row_layernorm_stress", (256, 3, 1, 70, _NSP)), ("test_gemv_row_layernorm_stress", (256, 4, 4, 70, _NSP)),
               ("test_layernorm_paths_agree_on_offset_rows", (768,)), ("test_stats_pool_stress", (1, _NSP)), ("test_stats_pool_stress", (3, _NSP)),
               ("test_stats_pool_stress", (512, _NSP))]


@pytest.mark.parametrize("name,args", _NORMSTRESS, ids=[f"{n}{list(a)}" for n, a in _NORMSTRESS])
def test_normstress_bodies_on_the_emulator(emu, name, args):
    import test_norm_stress_gpu
    getattr(test_norm_stress_gpu, name)(CPU, *args)


# tests/test_range_edges_gpu.py (both ends of the fp16 range: one prescribed outlier per launch and its twin, the flag contract C1 .. C4; operands far below 2^-14) at
# the GPU test's own shapes: every copy of the range check at least once -- the plain plane epilogue on a symmetric, a loader-wave, a 16-wave and the deferred forms
# (last element; the position sweep on tile 3), amax_df through folded tiles and the drain, the V^T store (plain and deferred), the LayerNorm epilogue, layernorm_planes
# (narrow and generic kernel), the split GEMM's three loaders and its LayerNorm fold, the split attention with fp32 and plane output.  The engine bodies need a GPU.
_RANGEEDGE = [("test_split_planes_range", ()),
              ("test_gemm_planes_plain_epilogue_range", (0, (1,), False)), ("test_gemm_planes_plain_epilogue_range", (3, (2,), True, ("gelu",))),
              ("test_gemm_planes_plain_epilogue_range", (21, (0,), False)), ("test_gemm_planes_plain_epilogue_range", (26, (1,), False)),
              ("test_gemm_planes_plain_epilogue_range", (32, (1, 2, 0), False)), ("test_gemm_planes_plain_epilogue_range", (35, (2,), False)),
              ("test_gemm_planes_plain_epilogue_range", (41, (2,), False)), ("test_gemm_planes_plain_epilogue_range", (42, (1,), False)),
              ("test_gemm_planes_deferred_epilogue_range", (41, 2, ((0, 0), (0, 1), (1, 1), (2, 1), (2, 2)))), ("test_gemm_planes_deferred_epilogue_range", (42, 1, ((0, 0), (1, 2), (2, 2)))),
              ("test_gemm_planes_transposed_range", (3, 36, 0, 1, slice(1, 4))), ("test_gemm_planes_transposed_range", (2, 132, 41, 2, slice(0, 4, 2))), ("test_gemm_planes_transposed_range", (3, 36, 42, 1)),
              ("test_gemm_planes_layernorm_epilogue_range", (False,)), ("test_gemm_planes_layernorm_epilogue_range", (True,)),
              ("test_layernorm_planes_range", (77,)), ("test_layernorm_planes_range", (37,)),
              ("test_split_gemm_linear_range", (129, 257, 320)), ("test_split_gemm_linear_range", (65, 100, 36)), ("test_split_gemm_layernorm_fold_range", ()),
              ("test_split_gemm_conv_range", ("fast_taps",)), ("test_split_gemm_conv_range", ("dilated",)), ("test_split_gemm_conv_range", ("upsample",)),
              ("test_split_gemm_conv_range", ("ragged",)), ("test_split_gemm_conv_range", ("transpose",)), ("test_precision16_shapes_on_the_exact_kernels_range", ()),
              ("test_split_flash_attn_range", (130, False, False)), ("test_split_flash_attn_range", (103, True, False)), ("test_split_flash_attn_range", (130, False, True)),
              ("test_split_flash_attn_range", (103, True, True)),
              ("test_lower_end_linear", (64, 96, 256)), ("test_lower_end_linear", (65, 100, 36)), ("test_lower_end_linear_planes", (9,)), ("test_lower_end_linear_planes", (35,)),
              ("test_lower_end_conv", ()), ("test_lower_end_attention_v", ())]


@pytest.mark.parametrize("name,args", _RANGEEDGE, ids=[f"{n}{list(a)}" for n, a in _RANGEEDGE])
def test_range_edge_bodies_on_the_emulator(emu, name, args):
    import test_range_edges_gpu
    getattr(test_range_edges_gpu, name)(CPU, *args)


# tests/test_vocoder_edges_gpu.py (vocoder_edges_common.py: the HiFT tail kernels and the conv forms of the vocoder at their edge shapes) at emulator sizes: the iSTFT
# geometry set and the ragged iSTFT (per-row frame counts: rows equal solo launches bit for bit, zeros beyond), the value case, the refusals, the f0 thresholds, the
# minimum STFT lengths, every row of the conv table at every precision it lists (the rows longer than T = 140 too: each takes under 2 s here).  The grid-stride second laps are left to the GPU.
def _vocoder_edge_cases():
    import vocoder_edges_common as V
    cases = [("check_istft_geometry", (fr, B, ldx)) for fr in V.ISTFT_FRAMES for B, ldx in ((1, 18), (3, 32))]
    cases += [("check_istft_geometry", (66, 1, 32)), ("check_istft_geometry", (66, 3, 18))]
    cases += [("check_istft_ragged", ()), ("check_istft_values", ()), ("check_istft_refusals", ()), ("check_source_thresholds", ())]
    cases += [("check_stft", (2, L, ld)) for L in (16, 20) for ld in (18, 32)]
    cases += [("check_conv_case", (c["name"], p)) for c in V.CONV_CASES for p in c["precisions"]]
    return cases


_VOCODER = _vocoder_edge_cases()


@pytest.mark.parametrize("name,args", _VOCODER, ids=[f"{n}{list(a)}" for n, a in _VOCODER])
def test_vocoder_edge_bodies_on_the_emulator(emu, name, args):
    import vocoder_edges_common as V
    from chatterbox_amd import ops
    getattr(V, name)(ops, CPU, *args)


# tests/test_smallest_shapes_gpu.py (smallest_shapes_common.py: the pipelined kernels where their prologues and drains run) -- a reduced matrix that keeps every branch:
# K walks of 1, 2, 3 K tiles at BK = 32 and BK = 64 (and 4, 6: the full Linear shape list) on the dispatcher's choice, a symmetric three-stage form of each K tile width
# (12, 45), loader-wave forms with one and four loaders (21, 33), the four-stage rings (25, 34), both deferred-epilogue forms with both df_kinds on tile walks (the
# `nk < PKT` arm) and one tile per workgroup (the drain), the LayerNorm epilogue at nk = 1, 2, 3, the conv and the transposed column range on a symmetric and a
# loader-wave form, every attention version at T = 7, 65, 129 (one, two and three KV tiles), the fp32-operand GEMMs in full, the K % 4 contract.
def _smallest_shape_cases():
    import smallest_shapes_common as S
    cases = [("check_linear_tile", (t, p)) for t, p in ((0, 2), (12, 2), (12, 0), (45, 2), (21, 2), (21, 0), (33, 2), (25, 2), (34, 0))]
    cases += [("check_deferred_epilogue", (t, pl, p, M, N)) for t, pl in ((41, 32), (42, 35)) for p, M, N in ((2, 300, 640), (0, 65, 512))]
    cases += [("check_layernorm_epilogue", (32, 2)), ("check_layernorm_epilogue", (64, 0)), ("check_layernorm_epilogue", (96, 2))]
    cases += [("check_conv_tile", (12, 2)), ("check_conv_tile", (21, 2)), ("check_conv_tile", (33, 0)), ("check_conv_tile", (43, 2))]
    cases += [("check_transposed_tile", (9, 2)), ("check_transposed_tile", (14, 2)), ("check_transposed_tile", (21, 0))]
    cases += [("check_attention", (v, (7, 65, 129))) for v in range(7)]
    cases += [("check_f32_linear", (1, S.F32_P1_M, S.F32_P1_N, S.F32_P1_K))] + [("check_f32_linear", (p, S.F32_SPLIT_M, S.F32_SPLIT_N, S.F32_SPLIT_K)) for p in (3, 6, 16)]
    cases += [("check_f32_layernorm_fold", ())] + [("check_k_multiple_of_4_contract", (p, M)) for p in (1, 16) for M in (1, 33)]
    return cases


_SMALLSHAPE = _smallest_shape_cases()


@pytest.mark.parametrize("name,args", _SMALLSHAPE, ids=["-".join([n] + [str(a).replace(" ", "") for a in args]) for n, args in _SMALLSHAPE])
def test_smallest_shape_bodies_on_the_emulator(emu, name, args):
    import smallest_shapes_common as S
    getattr(S, name)(CPU, *args)


@pytest.mark.parametrize("tile,persist", [(0, 1), (1, 0), (3, 8), (7, 1), (12, 0), (15, 8), (21, 1), (24, 8), (26, 0), (28, 1), (31, 8), (32, 1), (33, 0), (34, 8), (36, 1)])
def test_gemm_planes_tiles_small(emu, tile, persist):
    """tests/test_planes_gpu.py::test_gemm_planes_linear_tiles at emulator-sized shapes: symmetric, loader-wave (21+) and 16-wave (26+) tile
    forms, persistent and one-tile-per-workgroup grids, ragged M and N, bias + GELU + residual, fp32 and plane outputs."""
    from chatterbox_amd import ops
    from test_planes_gpu import _close, _planes_exact, _r
    try:
        emu.cbx_set_planes_tile(tile)
        emu.cbx_set_planes_persist(persist)
        for (M, N, K) in [(129, 258, 512), (333, 80, 256)]:
            x, w, b, r = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3), _r((M, N), 4)
            xP, wP = ops.split_planes(x), ops.split_planes(w)
            ref = F.gelu(F.linear(_planes_exact(x), _planes_exact(w), b.double())) + r.double()
            tol = 3e-5 * max(1.0, math.sqrt(K / 256))
            out, outP = r.clone(), ops.Planes(M, N, CPU, zero=True)
            ops.linear_planes(xP, wP, out=out, outp=outP, bias=b, act=ops.GELU_ERF, residual=out)
            _close(out, ref, tol, f"tile {tile} {M}x{N}x{K} (fp32 out)")
            _close(outP.float(), ref, tol, f"tile {tile} {M}x{N}x{K} (plane out)")
            assert (outP.float() - out).abs().max() <= 2.0 ** -21 * out.abs().max(), "plane output = split of the fp32 output"
    finally:
        emu.cbx_set_planes_tile(0)
        emu.cbx_set_planes_persist(1)


@pytest.mark.parametrize("tile,plain,persist", [(41, 32, 2), (42, 35, 1)])
def test_gemm_planes_deferred_epilogue_small(emu, tile, plain, persist):
    """tests/test_planes_gpu.py::test_gemm_planes_deferred_epilogue_equals_plain at emulator-sized shapes."""
    import test_planes_gpu
    test_planes_gpu.test_gemm_planes_deferred_epilogue_equals_plain(CPU, tile, plain, persist, shapes="small")


@pytest.mark.parametrize("M,K,res", [(333, 512, True), (64, 256, False)])
def test_gemm_planes_layernorm_epilogue_small(emu, M, K, res):
    """tests/test_planes_gpu.py::test_gemm_planes_layernorm_epilogue at emulator-sized shapes."""
    import test_planes_gpu
    test_planes_gpu.test_gemm_planes_layernorm_epilogue(CPU, M, K, res)


def test_gemm_planes_conv_and_transposed_columns_small(emu):
    """Causal 3-tap Conv1d on planes with ragged lengths, and q | k | V^T from one launch (ABI v8), at emulator-sized shapes."""
    from chatterbox_amd import ops
    from test_planes_gpu import _close, _planes_exact, _r
    B, T, cin, N = 2, 77, 64, 128
    x, w, b = _r((B, T, cin), 1), _r((N, cin, 3), 2, 1 / math.sqrt(3 * cin)), _r((N,), 3)
    lens = torch.tensor([77, 30], dtype=torch.int32)
    xm = x.clone()
    xm[1, 30:] = 0
    ref = F.conv1d(F.pad(_planes_exact(xm).transpose(1, 2), (2, 0)), _planes_exact(w), b.double()).transpose(1, 2)
    wp = w.permute(0, 2, 1).reshape(N, 3 * cin).contiguous()
    wide = ops.Planes(B * T, 128, CPU, zero=True)
    ops.split_planes(x.reshape(B * T, cin), wide.cols(32, cin))
    out, outP = torch.empty(B, T, N), ops.Planes(B * T, N, CPU)
    ops.conv1d_planes(wide.cols(32, cin), ops.split_planes(wp), B=B, T=T, taps=3, cin=cin, out=out, outp=outP, bias=b, pad_left=2, lens=lens)
    _close(out, ref, 6e-5, "conv3 with ragged lengths")
    _close(outP.float().view(B, T, N), ref, 6e-5, "conv3 plane output")
    Z, T2 = 2, 36
    M, K, Nn, n0 = Z * T2, 256, 1536, 1024
    Tp = (T2 + 7) // 8 * 8
    h, wq = _r((M, K), 4), _r((Nn, K), 5, 1 / 16)
    hP, wP = ops.split_planes(h), ops.split_planes(wq)
    qkP, vtP = ops.Planes(M, n0, CPU), ops.Planes(Z * 512, Tp, CPU, zero=True)
    ops.gemm_planes(hP, wP, M=M, N=Nn, K=K, P=qkP, PT=vtP, pt_n0=n0, pt_T=T2, pt_zs=512 * vtP.ld)
    ref = F.linear(_planes_exact(h), _planes_exact(wq))
    _close(qkP.float(), ref[:, :n0], 3e-5, "q | k columns")
    vt = vtP.float().view(Z, 512, Tp)
    _close(vt[:, :, :T2], ref[:, n0:].view(Z, T2, 512).transpose(1, 2), 3e-5, "V^T columns")
    assert float(vt[:, :, T2:].abs().max()) == 0.0, "pad keys of V^T stay zero"


@pytest.mark.parametrize("tile", [4, 9, 14])
def test_gemm_planes_transposed_walk_small(emu, tile):
    """q | k | V^T from one launch on a PERSISTENT grid of 2 workgroups: every workgroup walks 12+ tiles, transposed (V^T) tiles followed by
    q | k tiles.  Under CBX_EMU_DMA=deferred this is the case that exposed a too-weak counted wait behind the transposed epilogue (8-byte
    stores = half the operations the wait assumed): fixed in gemm_planes.hip (W_EPI0T); the body runs in both modes."""
    from chatterbox_amd import ops
    from test_planes_gpu import _close, _planes_exact, _r
    try:
        emu.cbx_set_planes_tile(tile)
        emu.cbx_set_planes_persist(2)
        Z, T = 2, 100
        M, K, N, n0, Tp = Z * T, 256, 1536, 1024, 104
        h, w = _r((M, K), 1), _r((N, K), 2, 1 / 16)
        hP, wP = ops.split_planes(h), ops.split_planes(w)
        qkP, vtP = ops.Planes(M, n0, CPU), ops.Planes(Z * 512, Tp, CPU, zero=True)
        ops.gemm_planes(hP, wP, M=M, N=N, K=K, P=qkP, PT=vtP, pt_n0=n0, pt_T=T, pt_zs=512 * vtP.ld)
        ref = F.linear(_planes_exact(h), _planes_exact(w))
        _close(qkP.float(), ref[:, :n0], 3e-5, f"q | k columns, tile {tile}")
        _close(vtP.float().view(Z, 512, Tp)[:, :, :T], ref[:, n0:].view(Z, T, 512).transpose(1, 2), 3e-5, f"V^T, tile {tile}")
    finally:
        emu.cbx_set_planes_tile(0)
        emu.cbx_set_planes_persist(1)


@pytest.mark.parametrize("version", [2, 1, 4, 5, 6])
def test_flash_attn_planes_small(emu, version):
    """tests/test_planes_gpu.py::test_flash_attn_planes at emulator-sized shapes (ragged key lengths incl. an empty utterance)."""
    import test_planes_gpu
    try:
        emu.cbx_set_attn_planes_version(version)
        test_planes_gpu.test_flash_attn_planes(CPU, version, 3, 200, [200, 130, 1])
        test_planes_gpu.test_flash_attn_planes(CPU, version, 1, 64, None)
    finally:
        emu.cbx_set_attn_planes_version(0)  # the library's automatic choice


def test_split_gemm_small(emu):
    """gemm_split.hip (encoder / HiFT / range-check fallback path): the three split precisions and the LayerNorm-folded loader, small shapes."""
    from chatterbox_amd import ops
    from test_ops_gpu import _close, _r
    M, N, K = 200, 96, 256
    x, w, b = _r((M, K), 1), _r((N, K), 2, 1 / 16), _r((N,), 3)
    ref = F.linear(x.double(), w.double(), b.double()).float()
    for prec, tol in ((3, 1e-4), (6, 3e-5), (16, 3e-5)):
        out = torch.empty(M, N)
        with ops.gemm_precision(prec):
            ops.linear(x, w, out, bias=b)
        _close(out, ref, tol * 4, f"split gemm precision {prec}")
    g, be = 1 + 0.1 * _r((K,), 4), 0.1 * _r((K,), 5)
    stats, out = torch.empty(M, 2), torch.empty(M, N)
    with ops.gemm_precision(16):
        assert ops.ln_fusable(M, K)
        ops.row_stats(x, stats)
        ops.linear(x, w, out, bias=b, ln=(stats, g, be))
    _close(out, F.linear(F.layer_norm(x, (K,), g, be, 1e-5), w, b), 1e-4, "LayerNorm folded into the A operand")


@pytest.fixture(scope="module")
def tiny_llama(emu):
    """2 layers of the real T3 width (1024 / 4096 / 16 heads), 4 rows (2 utterances x CFG), every packed image the tile variants need."""
    from chatterbox_amd import ops
    from oracle import ref_torch as O
    from test_ops_gpu import _r as g
    L, D, Fd, V, maxp = 2, 1024, 4096, 512, 64
    lw = [dict(ln1=1 + 0.1 * g((D,), 10 + i), ln2=1 + 0.1 * g((D,), 20 + i), wqkv=g((3 * D, D), 30 + i, 0.03), wo=g((D, D), 40 + i, 0.03),
               wg=g((Fd, D), 50 + i, 0.03), wu=g((Fd, D), 60 + i, 0.03), wd=g((D, Fd), 70 + i, 0.015)) for i in range(L)]
    for w in lw:
        w["wgu_pk"] = ops.pack_gemv_weight(torch.cat([w["wg"], w["wu"]], 0), swiglu=True)
        for name, tcs in (("wqkv", (16, 12)), ("wo", (16, 8, 4)), ("wd", (16, 8, 4))):
            for tc in tcs:
                w[f"{name}_pk{tc}"] = ops.pack_gemv_weight(w[name], half_tile=0 if tc == 16 else tc)
    m = dict(L=L, D=D, F=Fd, H=16, V=V, maxp=maxp, rows=4, B=2, lw=lw, emb=g((V, D), 1), pos_emb=g((maxp, D), 2, 0.1), norm=1 + 0.1 * g((D,), 3))
    m["head_pk"] = ops.pack_gemv_weight(g((V, D), 4, 0.03))
    cos, sin = O.rope_cos_sin(torch.arange(maxp), O.llama3_inv_freq())
    m["cos"], m["sin"] = cos.contiguous(), sin.contiguous()
    return m


def _tiny_state(m):
    from test_ops_gpu import _r as g
    L, rows, B, D, Fd, H, V, maxp = (m[k] for k in ("L", "rows", "B", "D", "F", "H", "V", "maxp"))
    st = dict(kc=g((L, rows, H, maxp, 64), 5), vc=g((L, rows, H, maxp, 64), 6), logits=torch.zeros(rows, V),
              seen=torch.zeros(B, V, dtype=torch.uint8), uniforms=torch.rand(B, 8, generator=torch.Generator().manual_seed(7)),
              step=torch.zeros(B, dtype=torch.int32), out_tokens=torch.zeros(B, 8, dtype=torch.int64), done=torch.zeros(B, dtype=torch.int32),
              n_generated=torch.zeros(B, dtype=torch.int32), next_ids=torch.tensor([5, 9, 5, 9]), next_pos_ids=torch.tensor([1, 1, 1, 1], dtype=torch.int32),
              positions=torch.tensor([20, 31, 20, 31], dtype=torch.int32), ctx_lens=torch.tensor([21, 32, 21, 32], dtype=torch.int32),
              samp=torch.tensor([[0.5, 0.8, 0.05, 1.0, 1.2, 0.0, -1.0, 0.0]] * B))
    ws = {k: torch.zeros(16, D) for k in ("x", "x2", "att")}
    ws.update(qkv=torch.zeros(rows, 3 * D), g=torch.zeros(16, Fd), pd=torch.zeros(4, 16, D))
    return st, ws


def _tiny_sampler_kw(m, st):
    return dict(logits=st["logits"], ld=m["V"], V=m["V"], B=m["B"], cfg=1, order=0, eos_token=m["V"] - 1, dev_params=st["samp"], seen=st["seen"],
                uniforms=st["uniforms"], max_steps=8, step=st["step"], out_tokens=st["out_tokens"], done=st["done"], n_generated=st["n_generated"],
                next_ids=st["next_ids"], next_pos_ids=st["next_pos_ids"], positions=st["positions"], ctx_lens=st["ctx_lens"])


def _tiny_step_launches(m, qtc, odtc, dks):
    """The token step launch by launch, as T3Engine._forward_decode_v2 + _sample issue it."""
    from chatterbox_amd import ops
    st, ws = _tiny_state(m)
    rows, D, Fd, V = m["rows"], m["D"], m["F"], m["V"]
    cur, nxt, pk = ws["x"], ws["x2"], dict(w_packed=True, x_packed=True, M=rows)
    qt, ot = (0 if qtc == 16 else qtc), (0 if odtc == 16 else odtc)
    ops.embed(st["next_ids"], m["emb"], cur, table2=m["pos_emb"], ids2=st["next_pos_ids"], out_packed=True)
    red = {}
    for i, w in enumerate(m["lw"]):
        ops.gemv(cur, w[f"wqkv_pk{qtc}"], ws["qkv"], N=3 * D, K=D, nw=8, norm_w=w["ln1"], half_tile=qt, **red, **pk)
        if red:
            cur, nxt = nxt, cur
        ops.decode_attn_rope(ws["qkv"], st["positions"], m["cos"], m["sin"], st["kc"][i], st["vc"][i], ws["att"], 0.125, out_packed=True)
        ops.gemv(ws["att"], w[f"wo_pk{odtc}"], cur, N=D, K=D, nw=8, res=cur, out_packed=True, half_tile=ot, **pk)
        ops.gemv(cur, w["wgu_pk"], ws["g"], N=Fd, K=D, swiglu=True, nw=8, norm_w=w["ln2"], out_packed=True, **pk)
        if dks > 1:
            ops.gemv(ws["g"], w[f"wd_pk{odtc}"], ws["pd"][:dks], N=D, K=Fd, ksplit=dks, nw=16, out_packed=True, half_tile=ot, **pk)
            red = dict(xpart=ws["pd"][:dks], x_out=nxt)
        else:
            ops.gemv(ws["g"], w[f"wd_pk{odtc}"], cur, N=D, K=Fd, nw=16, res=cur, out_packed=True, half_tile=ot, **pk)
    if red:
        red["x_out"] = None
    ops.gemv(cur, m["head_pk"], st["logits"], N=V, K=D, nw=8, norm_w=m["norm"], **red, **pk)
    ops.t3_sample(**_tiny_sampler_kw(m, st))
    return st


def _tiny_step_c(emu, m, qtc, odtc, dks):
    """The same step as ONE call of the stage-level C entry point (csrc/t3_step.hip)."""
    import ctypes

    from chatterbox_amd._lib import SamplerParams, T3Layer, T3Step
    st, ws = _tiny_state(m)
    layers = (T3Layer * m["L"])()
    for i, w in enumerate(m["lw"]):
        layers[i].ln1, layers[i].ln2, layers[i].wqkv = w["ln1"].data_ptr(), w["ln2"].data_ptr(), w[f"wqkv_pk{qtc}"].data_ptr()
        layers[i].wo, layers[i].wgu, layers[i].wd = w[f"wo_pk{odtc}"].data_ptr(), w["wgu_pk"].data_ptr(), w[f"wd_pk{odtc}"].data_ptr()
    sp = SamplerParams()
    for k, v in _tiny_sampler_kw(m, st).items():
        setattr(sp, k, v.data_ptr() if torch.is_tensor(v) else v)
    d = T3Step()
    d.n_layers, d.rows, d.dim, d.ffn, d.n_heads, d.vocab = m["L"], m["rows"], m["D"], m["F"], m["H"], m["V"]
    d.o_nw, d.gu_nw, d.d_nw, d.d_ksplit, d.w_bf16, d.eps, d.attn_scale = 8, 8, 16, dks, 0, 1e-5, 0.125
    d.half_tiles, d.qkv_tile = (0 if odtc == 16 else odtc), (0 if qtc == 16 else qtc)
    d.layers = layers
    d.speech_emb, d.speech_pos, d.final_norm, d.head = m["emb"].data_ptr(), m["pos_emb"].data_ptr(), m["norm"].data_ptr(), m["head_pk"].data_ptr()
    d.cos_t, d.sin_t, d.kc, d.vc = m["cos"].data_ptr(), m["sin"].data_ptr(), st["kc"].data_ptr(), st["vc"].data_ptr()
    d.kv_row_stride, d.kv_head_stride = st["kc"].stride(1), st["kc"].stride(2)
    d.next_ids, d.next_pos_ids, d.positions = st["next_ids"].data_ptr(), st["next_pos_ids"].data_ptr(), st["positions"].data_ptr()
    d.x_a, d.x_b, d.qkv, d.att, d.g, d.pd = (ws[k].data_ptr() for k in ("x", "x2", "qkv", "att", "g", "pd"))
    d.logits, d.ld_logits, d.sampler = st["logits"].data_ptr(), m["V"], ctypes.pointer(sp)
    assert emu.cbx_t3_decode_step(ctypes.byref(d), None) == 0, emu.cbx_last_error()
    return st


_STEP_KEYS = ("logits", "out_tokens", "next_ids", "positions", "ctx_lens", "kc", "vc", "seen", "n_generated")


def _tiny_step_reference(m):
    """fp64 torch restatement of the step (HF Llama decoder layer arithmetic, reference a5): logits (rows, V)."""
    from oracle import ref_torch as O
    st, _ = _tiny_state(m)
    D, H, rows = m["D"], m["H"], m["rows"]
    dd = lambda t: t.double()
    x = dd(m["emb"])[st["next_ids"]] + dd(m["pos_emb"])[st["next_pos_ids"].long()]
    rms = lambda v, w: v * torch.rsqrt((v * v).mean(-1, keepdim=True) + 1e-5) * dd(w)
    pos = st["positions"].long()
    c, s = dd(m["cos"])[pos][:, None], dd(m["sin"])[pos][:, None]
    for i, w in enumerate(m["lw"]):
        q, k, v = (rms(x, w["ln1"]) @ dd(w["wqkv"]).t()).view(rows, 3, H, 64).unbind(1)
        q, k = q * c + O._rot_half(q) * s, k * c + O._rot_half(k) * s
        att = torch.empty(rows, H, 64, dtype=torch.float64)
        for r in range(rows):
            kk = torch.cat([dd(st["kc"][i, r, :, : pos[r]]), k[r][:, None]], 1)
            vv = torch.cat([dd(st["vc"][i, r, :, : pos[r]]), v[r][:, None]], 1)
            p = torch.softmax(torch.einsum("hd,hkd->hk", q[r], kk) * 0.125, -1)
            att[r] = torch.einsum("hk,hkd->hd", p, vv)
        x = x + att.reshape(rows, D) @ dd(w["wo"]).t()
        h = rms(x, w["ln2"])
        x = x + (F.silu(h @ dd(w["wg"]).t()) * (h @ dd(w["wu"]).t())) @ dd(w["wd"]).t()
    from chatterbox_amd import ops  # the head image is only available packed: unpack through its row-major source is not kept, so rebuild
    from test_ops_gpu import _r as g
    return rms(x, m["norm"]) @ dd(g((m["V"], D), 4, 0.03)).t()


@pytest.mark.parametrize("qtc,odtc,dks", [(16, 8, 2), (12, 4, 1)])
def test_t3_decode_step_c_entry_point_and_tile_variants(emu, tiny_llama, qtc, odtc, dks):
    """cbx_t3_decode_step (csrc/t3_step.hip) against the same token step issued launch by launch from Python (t3.py::_forward_decode_v2 +
    _sample): identical logits, sampled ids and cache rows -- for the default geometry (16-column q/k/v tiles, 8-column o / down tiles,
    2 split-K partial images) and for the round-3 tile variants (12-column q/k/v tiles, 4-column o / down tiles, the down projection adding
    the residual itself: CBX_T3_TUNE="qkv_tc=12,od_tc=4,d_ks2=1").  Every variant also against an fp64 restatement of the step."""
    m = tiny_llama
    a = _tiny_step_launches(m, qtc, odtc, dks)
    b = _tiny_step_c(emu, m, qtc, odtc, dks)
    assert torch.isfinite(a["logits"]).all() and float(a["logits"].abs().max()) > 0
    for k in _STEP_KEYS:
        assert torch.equal(a[k], b[k]), f"cbx_t3_decode_step differs from the launch sequence in {k}"
    ref = _tiny_step_reference(m)
    err = (a["logits"].double() - ref).abs().max()
    assert err < 2e-4 * max(1.0, float(ref.abs().max())), f"logits vs fp64: {err:.3e}"
    assert torch.equal(a["positions"], torch.tensor([21, 32, 21, 32], dtype=torch.int32))


def _tiny_engine(m, tune, c_step):
    """A T3Engine object assembled around the tiny model (no checkpoint, no conditioning encoder: the decode step's own attributes)."""
    from chatterbox_amd.t3 import T3Engine
    eng = T3Engine.__new__(T3Engine)
    eng.dev, eng.L, eng.V, eng.weight_dtype, eng.decode_mode, eng.c_step = CPU, m["L"], m["V"], "fp32", "v2", c_step
    eng.layers = [dict(ln1=w["ln1"], ln2=w["ln2"], wqkv=w["wqkv"], wo=w["wo"], wd=w["wd"], wgu_pk=w["wgu_pk"], wqkv_pk=w["wqkv_pk16"], wo_pk=w["wo_pk16"],
                       wd_pk=w["wd_pk16"], wo_pk8=w["wo_pk8"], wd_pk8=w["wd_pk8"]) for w in m["lw"]]
    eng.norm, eng.head_pk, eng.speech_emb, eng.speech_pos, eng.cos, eng.sin = m["norm"], m["head_pk"], m["emb"], m["pos_emb"], m["cos"], m["sin"]
    eng.tune, eng._state, eng.knobs = dict(T3Engine._TUNE, **tune), {}, T3Engine._env_knobs()
    return eng


def test_t3_token_loop_equals_python_steps_on_the_emulator(emu, tiny_llama):
    """cbx_t3_loop_run of n steps == n token steps issued launch by launch from Python (T3Engine._forward_decode_v2 + _sample on the default geometry: split-K
    q/k/v, column-tile head) from the same mid-utterance state of ONE utterance (its CFG row pair) -- logits, sampler state and KV cache bit for bit;
    *steps_run reports the steps issued, and with every utterance flagged done a polled run stops at its first poll (the Llama twin of
    tests/test_turbo_stream_host.py::test_gpt2_token_loop_equals_python_steps_on_the_emulator)."""
    import ctypes
    m = tiny_llama
    eng = _tiny_engine(m, {}, False)  # c_step off: _decode_step is the Python launch sequence; the loop goes through cbx_t3_decode_step whatever it says
    eng._prepare_tune()
    ref_st, _ = _tiny_state(m)
    st = eng._get_state(1, m["maxp"], 8)
    assert st["rows"] == 2 and not eng._use_c_step(st)
    pair = [0, m["B"]]  # utterance 0 of the 2-utterance reference state: its conditional and its unconditional row
    for k in ("kc", "vc"):
        st[k].copy_(ref_st[k][:, pair])
    for k in ("next_ids", "next_pos_ids", "positions", "ctx_lens"):
        st[k].copy_(ref_st[k][pair])
    st["uniforms"].copy_(ref_st["uniforms"][:1])
    st["samp_dev"].copy_(ref_st["samp"][:1])
    tensors = lambda: [(d, k) for d in (st, st["dws"]) for k, v in d.items() if torch.is_tensor(v)]
    snap = [(d, k, d[k].clone()) for d, k in tensors()]
    for _ in range(3):
        eng._decode_step(st)
    keys = ("logits", "out_tokens", "n_generated", "next_ids", "next_pos_ids", "positions", "ctx_lens", "kc", "vc", "seen", "step", "done")
    want = {k: st[k].clone() for k in keys}
    assert torch.isfinite(want["logits"]).all() and float(want["logits"].abs().max()) > 0 and int(want["n_generated"].min()) == 3
    assert "cstep" not in st and "cloop" not in st
    for d, k, v in snap:
        d[k].copy_(v)
    assert eng._run_c_loop(st, 3, 0) == 3
    for k in keys:
        assert torch.equal(want[k], st[k]), f"cbx_t3_loop_run differs from the Python steps in {k}"
    # the EOS poll: everything flagged done, 12 steps asked for with a poll every 4 -> the loop stops after the first poll
    st["done"].fill_(1)
    ran = ctypes.c_int(-1)
    assert emu.cbx_t3_loop_run(eng._c_loop(st), 12, 4, None, ctypes.byref(ran)) == 0, emu.cbx_last_error()
    assert ran.value == 4 and torch.equal(st["step"], want["step"]), "finished utterances are no-ops in the sampler; the loop ended at the first poll"


@pytest.mark.parametrize("tune,c_step", [(dict(qkv_tc=12, od_tc=4, d_ks2=1), True), (dict(qkv_tc=12, od_tc=4, d_ks2=1, d_nw2=8), False)])  # the default tune: the e2e test below
def test_t3_engine_decode_step_code_on_the_emulator(emu, tiny_llama, tune, c_step, monkeypatch):
    """chatterbox_amd/t3.py's own decode-step code (T3Engine._prepare_tune / _tiles / _image / _forward_decode_v2 / _decode_step_c) driven on
    the emulator: an engine object assembled around the tiny model, one token step, against the hand-written launch sequence above."""
    m = tiny_llama
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: type("S", (), {"cuda_stream": None})())
    eng = _tiny_engine(m, tune, c_step)
    qtc, odtc = eng._tiles()
    assert (qtc, odtc) == ((12, 4) if tune else (16, 8))
    eng._prepare_tune()
    assert all(f"wqkv_pk{qtc}" in lw or qtc == 16 for lw in eng.layers)
    ref_st, _ = _tiny_state(m)
    st = eng._get_state(m["B"], m["maxp"], 8)
    for k in ("kc", "vc", "uniforms", "next_ids", "next_pos_ids", "positions", "ctx_lens"):
        st[k].copy_(ref_st[k])
    st["samp_dev"].copy_(ref_st["samp"])
    eng._decode_step(st)
    want = _tiny_step_launches(m, qtc, odtc, eng.tune["d_ks2"]) if eng.tune["d_nw2"] == 16 else None
    if want is not None:
        for k in ("logits", "next_ids", "kc", "vc", "positions"):
            assert torch.equal(st[k], want[k]), f"T3Engine decode step differs from the reference launch sequence in {k}"
    else:  # another wave count of the down projection: a different (valid) summation order
        ref = _tiny_step_reference(m)
        assert (st["logits"].double() - ref).abs().max() < 2e-4 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("tune", [dict(), dict(row_path=0), dict(row_path=0, qkv_tc=12, od_tc=4, d_ks=1, d_nw=8)], ids=["few_row_path", "mfma_path", "mfma_qkv12_od4_nopartials"])
def test_t3_turbo_engine_samples_the_oracles_tokens_on_the_emulator(emu, tune):
    """The WHOLE T3-Turbo path of chatterbox_amd/t3_turbo.py on the emulator -- conditioning, prefill (exact fp32 GEMMs + flash attention),
    the 5-launch GPT-2 decode step with the LayerNorm-folded GEMVs, the device sampler (top-k / top-p bisection, repetition penalty) -- on a
    1-layer, 256-wide model with two utterances of different text length and voice: sampled ids identical to the CPU oracle's
    (oracle/ref_torch.py::t3_inference_turbo, itself pinned against the reference).  Second case: the round-3 decode tile variants."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    from oracle import ref_torch as O
    samp = dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2)
    L, d, steps = 1, 256, 5
    sd = synth.t3_turbo_state_dict(L, d, 0)
    texts = [synth.turbo_text_tokens(n, seed=s) for n, s in ((7, 1), (12, 2))]
    conds = [synth.t3_cond(seed=s, prompt_len=24) for s in (2, 3)]
    u = synth.rand((2, steps + 1), seed=11)
    eng = T3TurboEngine(sd, CPU)
    eng.tune.update(tune)
    toks = eng.generate(conds, texts, max_gen_len=steps, uniforms=u, ban_eos=True, use_graph=False, **samp)
    for b in range(2):
        ref = O.t3_inference_turbo(sd, L, d // 64, conds[b], texts[b], steps, u[b], ban_eos=True, **samp)
        assert toks[b].tolist() == ref.tolist(), f"utterance {b}: {toks[b].tolist()} vs oracle {ref.tolist()}"


@pytest.mark.skipif(os.environ.get("CBX_EMU_SLOW") != "1", reason="model-level emulator runs take minutes to half an hour each: CBX_EMU_SLOW=1")
@pytest.mark.parametrize("name,args", [("test_flow_vs_reference_golden", (None,)), ("test_hift_vs_reference_golden", ()), ("test_meanflow_vs_reference_golden", ()),
                                       ("test_flow_batched_ragged_vs_oracle", ()), ("test_hift_batched_ragged_vs_oracle", ()),
                                       ("test_flow_and_vocoder_with_one_voice_per_utterance", ()), ("test_minimum_sizes_vs_oracle", ()),
                                       ("test_end_to_end_batch_vs_oracle", ()), ("test_encoder_flash_relpos_modes_match_the_materialised_encoder", ())])
def test_model_level_golden_bodies_on_the_emulator(emu, name, args):
    """tests/test_models_gpu.py bodies against the REFERENCE's golden vectors, executed by the emulator: the whole S3Gen flow (conformer encoder
    + 10-step CFG CFM on the plane-format estimator, 56 transformer blocks) reproduces the reference's mel at the fp32 tolerances on the CPU
    (measured: flow golden 31 min before the emulator's MFMA fast path, HiFT golden 140 s, meanflow golden 59 s; all three pass; under CBX_EMU_SCHED=random CBX_EMU_DMA=deferred the ragged-batch flow / HiFT bodies
    and the mixed-voice batch pass against the oracle in 4 / 3 / 7 min).  Opt-in."""
    import test_models_gpu
    import test_zz_abi_v9_gpu
    (getattr(test_models_gpu, name, None) or getattr(test_zz_abi_v9_gpu, name))(CPU, *args)


def _rerun(env, select):
    """A fresh pytest process of THIS file under emulator switches that are read when the emulated library loads."""
    import subprocess
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", select], env=e, capture_output=True, text=True,
                       cwd=os.path.dirname(HERE))
    return r.returncode, (r.stdout + r.stderr)[-1500:]


_DMA_TESTS = ("gemm_planes_tiles_small or flash_attn_planes_small or conv_and_transposed_columns or transposed_walk or layernorm_epilogue or deferred_epilogue "
              "or smallest_shape")


def test_counted_waits_of_the_lds_dma_pipelines_are_sufficient(emu):
    """CBX_EMU_DMA=deferred: every LDS-DMA lands only when its lane's own explicit `s_waitcnt vmcnt(n)` (or a __syncthreads / the kernel's
    end) retires it -- as late as the sources' counted waits allow, with the epilogue's buffer loads / stores occupying their slots of the
    in-order counter.  The plane GEMM (symmetric, loader-wave, persistent, 2-4 stage rings), the plane attention (three versions) and the
    fused MLP must still be exact: their waits do not lean on timing.  Self-check: with every wait weakened by ONE operation
    (CBX_EMU_DMA_SLACK=1) the same tests must fail."""
    rc, out = _rerun({"CBX_EMU_DMA": "deferred"}, _DMA_TESTS)
    assert rc == 0, out
    rc, out = _rerun({"CBX_EMU_DMA": "deferred", "CBX_EMU_DMA_SLACK": "1"}, "gemm_planes_tiles_small and 21-1")
    assert rc != 0, "weakened waits went unnoticed: the deferred-DMA mode is not effective\n" + out
    # ... and the short K walks notice it too (nk = 1 .. 3 against a three-stage ring; a loader-wave form)
    for sel in ("smallest_shape and check_linear_tile-12-2", "smallest_shape and check_linear_tile-21-2"):
        rc, out = _rerun({"CBX_EMU_DMA": "deferred", "CBX_EMU_DMA_SLACK": "1"}, sel)
        assert rc != 0, f"weakened waits went unnoticed by the short-walk cases ({sel})\n" + out


def test_results_do_not_depend_on_the_lane_schedule(emu):
    """CBX_EMU_SCHED=random: the scheduler resumes the lanes of a workgroup in a fresh random order every sweep, so lanes and waves overtake
    each other wherever no barrier (or exchange) forbids it; a kernel with a missing barrier then reads LDS that has not been written.
    The workgroups of a launch run in a shuffled order too (the split-context decode attention must merge in split order whoever arrives last).
    Self-check: with the first barrier of every thread dropped (CBX_EMU_DROP_BARRIER=0) the same selection must fail."""
    sel = ("test_sampler or test_layernorm_rmsnorm or test_flash_attn or decode_attn_rope_fused or split_context or test_hift or (gemm_planes_tiles_small and 21-1) "
           "or (gemm_planes_tiles_small and 3-8) or (gemm_planes_tiles_small and 32-1) or (test_gemv_packed_rms_fused and False) or flash_attn_planes_small or layernorm_epilogue "
           "or (smallest_shape and (check_deferred_epilogue or check_linear_tile-21 or check_linear_tile-33 or check_linear_tile-25))")  # DF and loader-wave forms on short K walks
    rc, out = _rerun({"CBX_EMU_SCHED": "random:5"}, sel)
    assert rc == 0, out
    rc, out = _rerun({"CBX_EMU_SCHED": "random:5", "CBX_EMU_DROP_BARRIER": "0"}, "test_gemv_decode or test_linear")  # the K-slice reduction through LDS
    assert rc != 0, "a dropped barrier went unnoticed\n" + out


_SLOW2 = pytest.mark.skipif(os.environ.get("CBX_EMU_SLOW") != "1", reason="80 s (2 layers at the real width): CBX_EMU_SLOW=1")


@pytest.mark.parametrize("tune", [dict(), dict(qkv_ks=4, qkv_ct=3, head_ct=2), pytest.param(dict(qkv_tc=12, od_tc=4, d_ks2=1, d_nw2=8), marks=_SLOW2)],
                         ids=["default", "qkv_splitk_head_ct2", "qkv12_od4_nopartials"])
def test_t3_llama_engine_samples_the_oracles_tokens_on_the_emulator(emu, tune):
    """The WHOLE Multilingual T3 path of chatterbox_amd/t3.py on the emulator at the real width (1024 / 4096 / 16 heads, ONE layer): conditioning
    encoder + Perceiver, the ragged batched prefill (exact fp32 GEMMs, flash attention, RoPE + cache fill), CFG row pairs, the decode steps
    through the stage-level C entry point (the product default), the device sampler with the reference's processor order -- two utterances of
    different text length and voice: sampled ids identical to the CPU oracle's (oracle/ref_torch.py::t3_inference, pinned against the
    reference's T3.inference by tests/golden)."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3 import T3Engine
    from oracle import ref_torch as O
    samp = dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    L, steps = (2 if tune else 1), 3  # (2 layers: the second q/k/v GEMV folds the first layer's down-projection partial images)
    sd = synth.t3_state_dict(L, 0)
    eng = T3Engine(sd, CPU)
    assert eng.c_step and eng.decode_mode == "v2"
    eng.tune.update(tune)
    texts = [synth.text_tokens(n, seed=s) for n, s in ((3, 1), (5, 2))]
    conds = [synth.t3_cond(seed=s, prompt_len=20) for s in (2, 3)]
    u = synth.rand((2, steps), seed=11)
    toks = eng.generate(conds, texts, max_new_tokens=steps, uniforms=u, ban_eos=True, use_graph=False, **samp)
    st = next(iter(eng._state.values()))
    assert "cstep" in st, "the decode steps go through cbx_t3_decode_step"
    for b in range(2):
        ref = O.t3_inference(sd, L, conds[b], torch.stack([texts[b], texts[b]]), steps, u[b], ban_eos=True, **samp)
        assert toks[b].tolist() == ref.tolist(), f"utterance {b}: {toks[b].tolist()} vs oracle {ref.tolist()}"


def test_t3_prefill_c_entry_point_on_the_emulator(emu):
    """tests/test_zz_abi_v9_gpu.py::test_t3_prefill_through_the_c_entry_point_equals_the_python_sequence on the emulator: one layer at the real width, two
    ragged utterances, two token steps (the ragged 3-utterance, 2-layer body of the GPU test would take minutes here)."""
    import test_zz_abi_v9_gpu
    test_zz_abi_v9_gpu.test_t3_prefill_through_the_c_entry_point_equals_the_python_sequence(CPU, layers=1, lens=(3, 5), steps=2)


@pytest.mark.parametrize("name", ["test_s3_log_mel_vs_reference", "test_mel24k_vs_reference"])
def test_frontend_bodies_against_the_references_golden_vectors_on_the_emulator(emu, name):
    """tests/test_frontend_gpu.py bodies on the emulator: the S3 tokenizer's log-mel and the 24 kHz prompt mel (framed DFT as an exact fp32
    GEMM over the waveform, mel filterbank, log maps) against tests/golden/frontend.npz -- outputs of the UNMODIFIED reference."""
    import numpy as np
    import test_frontend_gpu
    getattr(test_frontend_gpu, name)(CPU, np.load(os.path.join(test_frontend_gpu.GOLD, "frontend.npz")))


@pytest.mark.skipif(os.environ.get("CBX_EMU_SLOW") != "1", reason="minutes each: CBX_EMU_SLOW=1")
@pytest.mark.parametrize("name", ["test_voice_encoder_vs_reference", "test_campplus_vs_reference", "test_s3tokenizer_quantize_vs_oracle"])
def test_frontend_model_bodies_on_the_emulator(emu, name):
    """The voice-encoder LSTM and CAMPPlus against the reference's golden vectors, the S3 tokenizer against the oracle (28 s / 170 s / 44 s under
    the hazard modes; all pass)."""
    import numpy as np
    import test_frontend_gpu
    fn = getattr(test_frontend_gpu, name)
    fn(CPU) if name.endswith("oracle") else fn(CPU, np.load(os.path.join(test_frontend_gpu.GOLD, "frontend.npz")))


@pytest.mark.skipif(os.environ.get("CBX_EMU_SLOW") != "1", reason="2 min on the emulator (13 real token steps at the real width): CBX_EMU_SLOW=1; the adoption rules "
                    "alone are covered by tests/test_host_logic.py::test_decode_autotuner_adoption_rules")
def test_t3_decode_autotuner_on_the_emulator(emu, monkeypatch):
    """chatterbox_amd/autotune.py driven on the emulator (in-process, eager steps): every candidate geometry runs one real token step of a 1-layer
    Llama T3 at the real width; the narrow-tile and pipelined-attention candidates reproduce the current geometry's logits BIT FOR BIT, the
    candidates that sum the down projection in another order are flagged (`reorders`) and are not `best`; with the clock replaced by a table the
    adoption rule is checked (fastest identical candidate = best, tile geometry first, attention knobs, then the GEMV epilogue prefetch on top, confirmed back to back; the fastest
    candidate overall = best_any, adopted only because the validate callback -- here: the engine samples the ORACLE's tokens on it -- says so)."""
    from chatterbox_amd import autotune as at, synth
    from chatterbox_amd.t3 import T3Engine
    from oracle import ref_torch as O
    L, steps = 1, 3
    sd = synth.t3_state_dict(L, 0)
    eng = T3Engine(sd, CPU)
    reorder = dict(od_tc=4, d_ks2=1, d_nw2=8)
    key = lambda v: tuple(sorted(v.items()))
    fake = {(): 1.0, key(dict(qkv_tc=12)): 0.8, key(dict(od_tc=4)): 0.9, key(reorder): 0.3, key(dict(qkv_tc=12, da_pipe=3)): 0.7,
            key(dict(reorder, da_pipe=3)): 0.25, key(dict(qkv_tc=12, da_pipe=3, pre_epi=1)): 0.65, key(dict(reorder, da_pipe=3, pre_epi=1)): 0.2}
    real = T3Engine.measure_decode

    def measure(self, **kw):
        _, logits = real(self, **dict(kw, steps=0))  # one real token step per call; the clock is the table above
        k = {k: v for k, v in self.tune.items() if v != T3Engine._TUNE[k]}
        k.update({k: v for k, v in self.knobs.items() if v != at.LIB_KNOBS[k]})
        return fake[key(k)], logits

    monkeypatch.setattr(T3Engine, "measure_decode", measure)
    samp = dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    texts = [synth.text_tokens(n, seed=s) for n, s in ((3, 1), (5, 2))]
    conds = [synth.t3_cond(seed=s, prompt_len=20) for s in (2, 3)]
    u = synth.rand((2, steps), seed=11)
    seen_geometry = []

    def validate():  # runs on the engine with best_any applied
        seen_geometry.append((dict(eng.tune), dict(eng.knobs)))
        toks = eng.generate(conds, texts, max_new_tokens=steps, uniforms=u, ban_eos=True, use_graph=False, **samp)
        return all(toks[b].tolist() == O.t3_inference(sd, L, conds[b], torch.stack([texts[b], texts[b]]), steps, u[b], ban_eos=True, **samp).tolist()
                   for b in range(2))

    try:
        rep = eng.autotune(B=1, ctx=12, steps=1, reps=1, in_child=False, tiles=(dict(), dict(qkv_tc=12), dict(od_tc=4), reorder), attn=(dict(da_pipe=3),),
                           validate=validate)
        rows = {key(r["variant"]): r for r in rep["candidates"] if "variant" in r}
        assert all("error" not in r for r in rows.values()), rows
        for k in (dict(qkv_tc=12), dict(od_tc=4), dict(qkv_tc=12, da_pipe=3), dict(qkv_tc=12, da_pipe=3, pre_epi=1)):
            assert rows[key(k)]["identical"], f"{k}: logits differ from the current geometry's by {rows[key(k)]['max_abs_diff']:.3e}"
        for k in (reorder, dict(reorder, da_pipe=3), dict(reorder, da_pipe=3, pre_epi=1)):  # another fp32 summation order: valid, fastest on the fake clock, never `best`
            assert rows[key(k)]["reorders"] and rows[key(k)]["valid"] and rows[key(k)]["max_abs_diff"] > 0, rows[key(k)]
        assert rep["best"] == dict(qkv_tc=12, da_pipe=3, pre_epi=1) and rep["ms_per_token"] == 0.65
        assert rep["best_any"] == dict(reorder, da_pipe=3, pre_epi=1) and rep["ms_per_token_any"] == 0.2
        assert len(seen_geometry) == 1 and seen_geometry[0][0]["d_ks2"] == 1 and seen_geometry[0][1]["da_pipe"] == 3 and seen_geometry[0][1]["pre_epi"] == 1
        assert rep["best_any_validated"] is True and rep["adopted"] == rep["best_any"], rep  # the oracle's tokens on the reordered geometry
        assert eng.tune["od_tc"] == 4 and eng.tune["d_ks2"] == 1 and eng.tune["qkv_tc"] == 0 and eng.knobs["da_pipe"] == 3 and eng.knobs["pre_epi"] == 1
        assert "wd_pk4" in eng.layers[0] and not [k for k in eng._state if k[3] == 7]
    finally:
        eng.apply_variant(dict(T3Engine._TUNE), dict(at.LIB_KNOBS))


@pytest.mark.skipif(os.environ.get("CBX_EMU_SLOW") != "1", reason="2 min on the emulator: CBX_EMU_SLOW=1")
def test_autotuner_child_entry_point_on_the_emulator(emu, monkeypatch, capsys):
    """`python -m chatterbox_amd.autotune` is what bench.py's child process runs: its main() here, on the emulator, with a short candidate list --
    argument parsing, engine construction, every stage of tune_decode, and the one-line JSON report the parent parses."""
    import json
    from chatterbox_amd import autotune as at
    orig = at.tune_decode
    monkeypatch.setattr(at, "tune_decode", lambda eng, **kw: orig(eng, tiles=(dict(), dict(qkv_tc=12)), attn=(dict(da_pipe=5),), epi=at.EPI_VARIANTS, **kw))
    at.main(["--layers", "1", "--batch", "1", "--ctx", "12", "--steps", "1", "--reps", "1"], device=CPU)
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    rows = {tuple(sorted(r["variant"].items())): r for r in rep["candidates"] if "variant" in r}
    assert all("error" not in r for r in rows.values()), rows
    for knob in ("qkv_tc", "da_pipe", "pre_epi"):  # (what a knob is tried on top of depends on the emulator's "clock")
        hit = [r for r in rows.values() if r["variant"].get(knob) and not r["variant"].get("d_ks2")]
        assert hit and all(r["identical"] for r in hit), (knob, hit)


_SLOW = pytest.mark.skipif(os.environ.get("CBX_EMU_SLOW") != "1", reason="half a minute each: CBX_EMU_SLOW=1")


@pytest.mark.parametrize("meanflow,T,fused_qkv,fused_ln", [(False, 20, True, 2), pytest.param(True, 34, True, 1, marks=_SLOW), pytest.param(False, 18, True, 1, marks=_SLOW),
                                                           pytest.param(True, 36, True, 0, marks=_SLOW), pytest.param(False, 20, True, 0, marks=_SLOW)])
def test_cfm_solve_c_entry_point_on_the_emulator(emu, meanflow, T, fused_qkv, fused_ln):
    """tests/test_zzz_stage_seams_gpu.py on the emulator: cbx_cfm_solve (ABI v12) against FlowEngine.cfm's own launch sequence, bit for bit -- one utterance,
    one mid stage, two Euler steps, CFG with the fused q | k | V^T projection; opt-in (CBX_EMU_SLOW=1, all pass): meanflow, the separate projection
    (T % 4 != 0)."""
    import test_zzz_stage_seams_gpu as S
    S.test_cfm_solve_through_the_c_entry_point_equals_the_python_sequence(CPU, meanflow, T, fused_qkv, fused_ln, n_mid=1, B=1, n_steps=2)


@pytest.mark.parametrize("ragged,fade,precision", [(True, True, 16), pytest.param(False, False, 1, marks=_SLOW)])
def test_hift_decode_c_entry_point_on_the_emulator(emu, ragged, fade, precision):
    """cbx_hift_decode (ABI v12) against HiFTEngine.decode's own launch sequence on the emulator, bit for bit (2 rows of 3 mel frames)."""
    import test_zzz_stage_seams_gpu as S
    S.test_hift_decode_through_the_c_entry_point_equals_the_python_sequence(CPU, ragged, fade, precision, T=3, B=2)


def test_s3gen_encode_c_entry_point_on_the_emulator(emu):
    """cbx_s3gen_encode (ABI v12) against FlowEngine._encode_rows' own launch sequence (flash rel-pos form), bit for bit: a ragged batch of 2 x 10 tokens, one
    conformer layer before and one after the upsampling (20 rows take the skinny GEMM, the 40 upsampled rows the split-operand kernel)."""
    import test_zzz_stage_seams_gpu as S
    S.test_s3gen_encode_through_the_c_entry_point_equals_the_python_sequence(CPU, B=2, N=10, n_enc=1, n_up=1)


def test_hift_f0_source_c_entry_point_on_the_emulator(emu):
    """cbx_hift_f0_source (ABI v12) against HiFTEngine.f0_predict + source, bit for bit (the source signal of a ragged batch of 2 x 4 mel frames)."""
    import test_zzz_stage_seams_gpu as S
    S.test_hift_f0_source_through_the_c_entry_point_equals_the_python_sequence(CPU, B=2, T=4)


@_SLOW
def test_vocode_with_every_stage_seam_on_the_emulator(emu):
    """ChatterboxEngine.vocode (S3Gen flow + HiFT) for a ragged batch of two utterances with cbx_s3gen_encode, cbx_cfm_solve, cbx_hift_f0_source and
    cbx_hift_decode switched on against the Python sequencing of the same launches: mel and waveforms bit for bit (3.5 min; passes)."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine
    eng = ChatterboxEngine(synth.t3_state_dict(1, 0), synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1), CPU, n_t3_layers=1)
    eng.last_timing = {}
    P = 6
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    st = [synth.speech_tokens(12, seed=1), synth.speech_tokens(9, seed=2)]
    z = synth.randn((2, 2 * (P + 12), 80), seed=7)
    phase = synth.rand((2, 9), seed=5) * 6.28 - 3.14
    phase[:, 0] = 0
    noise = synth.randn((2, 9, 480 * 24), seed=8)
    out = {}
    for seam in (False, True):
        eng.flow.c_seam = eng.hift.c_seam = seam
        wavs, mel = eng.vocode(st, ref, z=z, phase=phase, noise=noise, n_cfm_timesteps=2, sync=False)
        out[seam] = ([w.clone() for w in wavs], mel.clone())
    assert torch.equal(out[False][1], out[True][1]), "mel differs"
    for a, b in zip(out[False][0], out[True][0]):
        assert a.numel() > 0 and torch.equal(a, b), f"max |diff| {(a - b).abs().max().item():.3e}"


def test_t3_turbo_batch1_row_path_samples_the_oracles_tokens_on_the_emulator(emu):
    """Batch 1 of T3-Turbo runs on the single-row kernels (T3TurboEngine._forward_decode_row): sampled ids == the CPU oracle's."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    from oracle import ref_torch as O
    samp = dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2)
    L, d, steps = 1, 256, 5
    sd = synth.t3_turbo_state_dict(L, d, 0)
    text, cond = synth.turbo_text_tokens(9, seed=4), synth.t3_cond(seed=5, prompt_len=24)
    u = synth.rand((1, steps + 1), seed=12)
    eng = T3TurboEngine(sd, CPU)
    assert eng.tune["row_path"]
    calls = []
    orig = eng._forward_decode_row
    eng._forward_decode_row = lambda st: (calls.append(1), orig(st))[1]
    toks = eng.generate(cond, [text], max_gen_len=steps, uniforms=u, ban_eos=True, use_graph=False, **samp)
    ref = O.t3_inference_turbo(sd, L, d // 64, cond, text, steps, u[0], ban_eos=True, **samp)
    assert len(calls) == steps and toks[0].tolist() == ref.tolist(), (len(calls), toks[0].tolist(), ref.tolist())
