"""GPU (-m gpu), kernel level: cbx_prefill_embed (ops.prefill_embed) and cbx_kv_prefix_paste_f32 (ops.kv_prefix_paste) -- the two launches a mixed-voice batch
issues ahead of its first prefill GEMM, for the Llama T3 and for the GPT-2 backbones of Turbo / Nano -- against the per-utterance host loop and the broadcast copy_
pair they replace, bit for bit.  (The engine- and API-level tests of the batched path are in test_batch_api_gpu.py.)

WHY THIS FILE NAME: these tests have nothing to do with Turbo streaming.  test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test demands that
every launching entry point of include/cbx.h be named in a kernel-level test module and finds those modules by a fixed list of patterns, of which `test_turbo_stream_*`
is the only glob; existing test files are not edited when a feature is added, so the kernel-level tests of cbx_prefill_embed / cbx_kv_prefix_paste_f32 carry a name that
list matches.  Do not rename or merge this file into test_batch_api_gpu.py without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

LENS = {1: [37], 3: [7, 64, 1], 8: [12, 1, 64, 33, 7, 20, 64, 5]}


@pytest.mark.parametrize("cached", [False, True], ids=["with_conditioning", "behind_cached_prefix"])
@pytest.mark.parametrize("llama", [True, False], ids=["llama_layout", "gpt2_layout"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_ragged_prefill_assembly_equals_the_host_loop(dev, B, llama, cached):
    """The (rows, Sx, D) prefill input, positions, cache rows and last-position indices of one cbx_prefill_embed launch are torch.equal to what the per-utterance
    host loop over cbx_embed_f32 produced: ragged lengths, with the conditioning rows and behind a cached prefix, both layouts (GPT-2 without a cache: voices
    whose prompts differ in length)."""
    import batch_api_common as c
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        tb = c.tables(dev, D=1024)
        tt = c.texts(LENS[B])
        n_prompt = [33] * B if (llama or cached) else [(375, 20, 150, 5, 375, 64, 1, 99)[b] for b in range(B)]
        P = [34] * B if llama else [1 + n for n in n_prompt]
        g = torch.Generator().manual_seed(11)
        ce = [torch.randn(p, 1024, generator=g).to(dev) for p in P]
        P0 = P[0] if cached else 0
        want = c.host_loop_llama(ops, tb, tt, ce, P0) if llama else c.host_loop_gpt2(ops, tb, tt, ce, n_prompt, P0)
        got = c.call_kernel(ops, tb, tt, None if cached else ce, P, P0, llama)
        torch.cuda.synchronize()
    for w, g_, what in zip(want, got, ("x", "positions", "cache_rows", "last")):
        assert w.shape == g_.shape and w.dtype == g_.dtype and torch.equal(w, g_), what
    assert torch.equal(got[0].cpu(), torch.from_numpy(c.numpy_layout(tb, tt, None if cached else ce, P, P0, llama)))


@pytest.mark.parametrize("P", [34, 376])
def test_prefix_paste_by_voice_index_equals_the_copy_form(dev, P):
    """kc / vc[l, r, h, :P] = prefix[voice_of_row[r]][l, h, :P] in one launch == the broadcast copy_ pair per voice, for 1, 2 and B distinct voices; rows beyond the
    batch and positions beyond the prefix keep their contents."""
    import batch_api_common as c
    from chatterbox_amd import ops
    g = torch.Generator().manual_seed(5)
    L, R, H, ctx, B = 3, 9, 16, 448, 8
    for voice_of in ([0] * B, [1, 0, 0, 1, 1, 1, 0, 1], list(range(B))):
        prefixes = [(torch.randn(L, H, P, 64, generator=g).to(dev), torch.randn(L, H, P, 64, generator=g).to(dev)) for _ in range(max(voice_of) + 1)]
        base = torch.randn(2, L, R, H, ctx, 64, generator=g).to(dev)
        want, got = base.clone(), base.clone()
        c.paste_by_copy(want[0], want[1], prefixes, voice_of)
        with torch.cuda.device(dev):
            ops.kv_prefix_paste(prefixes, voice_of, got[0], got[1])
            torch.cuda.synchronize()
        assert torch.equal(want, got), f"{len(prefixes)} voices"
        assert torch.equal(got[:, :, B:], base[:, :, B:]) and torch.equal(got[:, :, :, :, P:], base[:, :, :, :, P:])
