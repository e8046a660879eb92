"""GPU (-m gpu): the decode forms above 16 rows and their boundaries against the CPU oracle (bodies: tests/wide_batch_common.py; the kernel bodies and the
Turbo engine at B = 16 / 17 also run on the emulator, tests/test_simt_kernels.py).

T3TurboEngine at every row regime -- few-row kernels (B = 2), packed 5-launch layer (3, 16), the 7-launch form (17 .. 64: one row in the second MFMA row tile,
the three-tile case served by the four-tile kernel, the fourth tile, the full batch), sub-batches (65) -- and T3Engine above its 16-row seam (18, 34, 48, 50
rows; 33 utterances in two sub-batches): sampled tokens equal the oracle's, raw logits within the project's 1e-3, eagerly and from the captured
graph.  Kernel level: cbx_gemv_f32 with a packed weight, a row-major strided x, bias / gelu / split-K at M > 16, and the LayerNorm form of cbx_add_norm_f32
above 16 rows, against fp64.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wide_batch_common as W  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", W.TURBO_ROWS)
def test_turbo_engine_samples_the_oracles_tokens_at_every_row_regime(dev, B):
    """L = 1, d = 256.  Measured on one MI355X, worst |logit - oracle| over the utterances (bound 1e-3): prefill 4.17e-6 (B = 2, 3, 16), 4.29e-6 (B = 17 .. 49),
    4.53e-6 (B = 64); decode steps 1.55e-6 (B = 2, few-row kernels), 2.15e-6 / 2.86e-6 (B = 3 / 16, packed layer), 2.38e-6 at every B of the 7-launch form.  The
    emulator gives 4.05e-6 / 2.38e-6.  Every token is the oracle's, eagerly and from the captured graph."""
    W.check_turbo_engine_vs_oracle(dev, B)


def test_turbo_engine_real_width_above_16_rows(dev):
    """Nano width (d = 768: ks_o = 2, 3 K blocks per wave in c_attn / c_fc), two layers, B = 17.  Measured on one MI355X: prefill 1.50e-5, decode 1.17e-5
    (bound 1e-3); the longest test of this module there, 0.95 s."""
    W.check_turbo_engine_vs_oracle(dev, 17, L=2, d=768)


def test_turbo_engine_fills_the_kv_cache_to_its_last_slot(dev):
    """B = 17, max_gen_len = 22, longest text 15 tokens: S + n_samples = 41 + 23 = 64 = max_ctx.  generate() never feeds its last sampled token back, so its own
    steps append up to position max_ctx - 2; the body then issues the one further forward the sampler has prepared, which appends at max_ctx - 1 and attends over
    all 64 slots, and compares it with the oracle's next step.  Measured on one MI355X: prefill 4.29e-6, decode 2.38e-6, the last-slot step 1.91e-6 (bound 1e-3)."""
    W.check_turbo_last_cache_slot(dev)


def test_turbo_engine_chunked_decoding_above_16_rows(dev):
    W.check_turbo_chunked_decoding(dev)


def test_turbo_engine_sub_batches_beyond_max_batch(dev):
    W.check_turbo_sub_batches(dev)


@pytest.mark.parametrize("B", W.LLAMA_B)
def test_llama_engine_above_16_rows(dev, B):
    """Two layers at the real width.  Measured on one MI355X, worst |logit - oracle| over the three oracle utterances (bound 1e-3): prefill 1.86e-5 / 2.07e-5 /
    1.91e-5 / 2.07e-5 and decode 1.34e-5 / 1.29e-5 / 1.29e-5 / 1.29e-5 at B = 9 / 17 / 24 / 25; every other utterance equals its batch-1 run."""
    W.check_llama_engine_above_16_rows(dev, B)


def test_llama_engine_sub_batches_beyond_max_batch(dev):
    W.check_llama_sub_batches(dev)


@pytest.mark.parametrize("N,K,ks,nw", W.GEMV_SHAPES)
@pytest.mark.parametrize("M", W.GEMV_M)
def test_gemv_wide_rows_packed_weight(dev, M, N, K, ks, nw):
    """Measured on one MI355X: worst error 1.47e-6 (M 17, K 768, 4 waves, bias + gelu_new) against the bound 3e-5 * max(1, sqrt(K / 256)) * (1 + |ref|); 1.5e-6 on
    the emulator."""
    W.check_gemv_wide_rows_packed_weight(dev, M, N, K, ks, nw)


@pytest.mark.parametrize("rows,ks", W.ADD_NORM_CASES)
def test_add_norm_layernorm_form_above_16_rows(dev, rows, ks):
    """Measured on one MI355X: worst error 1.55e-6 (residual stream, 17 rows, 8 partial images) against 2e-5 * (1 + |ref|)."""
    W.check_add_norm_layernorm_wide(dev, rows, ks)
