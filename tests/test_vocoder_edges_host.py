"""Host side of tests/test_vocoder_edges_gpu.py: what the cases of vocoder_edges_common.py are chosen for is what they claim (no GPU, no kernel)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import vocoder_edges_common as V  # noqa: E402


def test_the_conv_table_reaches_every_dispatch_form_the_vocoder_can_reach():
    """expected_form mirrors cbx_gemm_f32 and cbx_gemm_split_dispatch; every reachable form is reached by a named (case, precision), every other form is listed
    with its reason.  The listing is printed (pytest -s)."""
    reached = V.form_coverage()
    for form in sorted(reached, key=str):
        print(form, "<-", ", ".join(f"{n} @ p{p}" for n, p in reached[form][:4]), "..." if len(reached[form]) > 4 else "")
    for form, why in V.UNREACHED_FORMS.items():
        print(form, "not reached:", why)
        assert form not in reached and why
    # the cases the issue names land where the table says
    E = lambda n, p: V.expected_form(V.CASES[n], p)
    assert E("conv_pre_T5", 0) == E("conv_pre_T32", 16) == E("resblock_k11_d5_T20", 6) == E("up2_k5_T10", 3) == ("skinny",)
    assert E("conv_pre_T33", 0) == E("conv_pre_T33", 16) == ("fast16",), "cin 80 is no multiple of the split kernel's 32-wide K tile: exact fp32 at every precision"
    assert E("k64_form_k7_d3", 0) == ("fast64",) and E("k64_form_k11", 0) == ("n64",)
    assert E("split_tile_128x64", 16) == ("split", 12864, 2) and E("split_tile_64", 16) == ("split", 64, 2)
    assert E("up2_k5_ragged", 0) == ("generic",) and E("up2_k5_ragged", 3) == ("split", 64, 0)
    assert E("conv_post", 0) == ("n64",) and E("source_down_1x1_wide", 6) == ("split", 12864, 1)


def test_the_conv_table_holds_the_geometries_it_is_meant_to():
    c = V.CASES
    assert V.out_rows(c["source_down_s15_ragged"], 601) == 40 and [V.out_rows(c["source_down_s15_ragged"], n) for n in (300, 16)] == [(300 + 14 - 30) // 15 + 1, 1]
    assert V.out_rows(c["resblock_k11_d5_ragged"], 1) == 1 and V.out_rows(c["resblock_k11_d5_ragged"], 0) == 0 and V.out_rows(c["resblock_k11_d5_T20"], 20) == 20 < 51
    assert V.out_rows(c["up2_k5_ragged"], 31) == 62 and V.out_rows(c["ups_k11_s5_ragged"], 17) == 85
    assert V.gemm_shape(c["conv_post"])[1] == 18 and c["conv_post"]["ldc"] == 32
    assert V.gemm_shape(c["k64_form_k7_d3"])[2] >= 1024 and c["k64_form_k7_d3"]["cin"] % 64 == 0
    ragged = [x for x in V.CONV_CASES if x["lens"] is not None]
    assert {(x["dil"] > 1, x["stride"] > 1, x["up"] > 1, x["kind"]) for x in ragged} >= {(True, False, False, "conv"), (False, True, False, "conv"), (False, False, True, "conv"),
                                                                                         (False, True, False, "convT")}


def test_the_istft_sets_cover_what_they_claim():
    assert [4 * (f - 1) for f in V.ISTFT_FRAMES] == [4, 8, 64, 256, 260, 480, 1440]
    n_clipped, n = V.value_case_claims()
    print(f"value case: {n_clipped} of {n} reference samples hit the +-0.99 clamp")
    x = V.ragged_istft_input()
    for b, k in enumerate(V.RAGGED_LENS):
        assert bool(x[b, k:].isnan().all()) and bool(x[b, :, 18:].isnan().all()) and not bool(x[b, :k, :18].isnan().any())
    worst = V.measure_torch_fp32_ratio()
    print(f"torch's own fp32 istft against fp64: worst ratio {worst:.3f} (recorded {V.C_TORCH_FP32}); the kernel is allowed {V.ISTFT_C:.2f}")
    # the recorded constant IS this measurement, rounded up to two decimals: not below it, and not stale above it (5 % covers another CPU's vector libm)
    assert worst <= V.C_TORCH_FP32, f"torch's own fp32 reaches {worst:.3f} here, above the recorded {V.C_TORCH_FP32}"
    assert worst >= 0.95 * V.C_TORCH_FP32, f"torch's own fp32 reaches only {worst:.3f} here: the recorded {V.C_TORCH_FP32} (and with it the kernel's allowance) is too generous"
    assert V.ISTFT_C == 2.0 * V.C_TORCH_FP32


def test_the_source_lap_excludes_a_handful_of_samples():
    import torch
    f0 = torch.rand(3, 800, generator=torch.Generator().manual_seed(1)) * 300
    f0[:, 5:9] = 3.0
    excl = V.source_lap_exclusions(f0)
    assert excl.shape == (3, 384000) and excl.numel() > 4096 * 256
    share = float(excl.double().mean())
    print(f"excluded: {int(excl.sum())} of {excl.numel()} samples ({share:.2e})")
    assert share <= V.SOURCE_LAP_EXCLUDED_MAX
