"""Shared by tests/test_batch_api_host.py (SIMT emulator, CPU tensors) and the GPU tests of the batched API: the per-utterance HOST LOOP that assembled the
prefill input before cbx_prefill_embed existed (T3Engine.generate / T3TurboEngine.generate of the parent commit, restated launch for launch on ops.embed), a NumPy
restatement of the same layout, and the broadcast copy_ form of the prefix paste.  Not a test module."""
import numpy as np
import torch

BOS = 6561


def tables(dev, D=256, text_vocab=97, speech_vocab=BOS + 2, n_pos=600, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(n, D, generator=g).to(dev)
    return dict(text_emb=mk(text_vocab), text_pos=mk(n_pos), speech_emb=mk(speech_vocab), speech_pos=mk(n_pos), wpe=mk(n_pos))


def texts(lens, vocab=97, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n in lens]


def host_loop_llama(ops, tb, text_tokens, ce, P0):
    """The parent's loop (Llama layout): rows b and B + b; ce: list of B (34, D) conditioning embeddings (unused when P0 = 34)."""
    dev, B, D = tb["text_emb"].device, len(text_tokens), tb["text_emb"].shape[1]
    rows = 2 * B
    tl = [int(t.numel()) for t in text_tokens]
    s0 = [34 + n + 2 for n in tl]
    S = max(s0)
    Sx = S - P0
    x = torch.zeros(rows, Sx, D, device=dev)
    bos = torch.full((2,), BOS, dtype=torch.int64, device=dev)
    zero2 = torch.zeros(2, dtype=torch.int32, device=dev)
    for b in range(B):
        ids = text_tokens[b].to(dev).long().view(-1)
        pos = torch.arange(tl[b], dtype=torch.int32, device=dev)
        for r, scale in ((b, 1.0), (B + b, 0.0)):
            if P0 == 0:
                x[r, :34] = ce[b]
            ops.embed(ids, tb["text_emb"], x[r, 34 - P0:34 - P0 + tl[b]], table2=tb["text_pos"], ids2=pos, scale=scale)
            ops.embed(bos, tb["speech_emb"], x[r, 34 - P0 + tl[b]:s0[b] - P0], table2=tb["speech_pos"], ids2=zero2)
    pos = torch.arange(P0, S, dtype=torch.int32, device=dev).repeat(rows)
    crow = torch.arange(rows, dtype=torch.int32, device=dev).repeat_interleave(Sx)
    last = torch.tensor([r * Sx + s0[r % B] - P0 - 1 for r in range(rows)], device=dev)
    return x, pos, crow, last


def host_loop_gpt2(ops, tb, text_tokens, ce, n_prompt, P0):
    """The parent's loop (GPT-2 layout): ce[b] the (1 + n_prompt[b], D) conditioning rows [speaker + wpe[0] | prompt embeddings + wpe] (unused when P0 > 0)."""
    dev, B, D = tb["text_emb"].device, len(text_tokens), tb["text_emb"].shape[1]
    tl = [int(t.numel()) for t in text_tokens]
    s0 = [1 + n_prompt[b] + tl[b] + 1 for b in range(B)]
    S = max(s0)
    Sx = S - P0
    x = torch.zeros(B, Sx, D, device=dev)
    for b in range(B):
        pos = torch.arange(s0[b], dtype=torch.int32, device=dev)
        if P0 == 0:
            x[b, :1 + n_prompt[b]] = ce[b]
        a, e = 1 + n_prompt[b], 1 + n_prompt[b] + tl[b]
        ops.embed(text_tokens[b].to(dev).long().view(-1), tb["text_emb"], x[b, a - P0:e - P0], table2=tb["wpe"], ids2=pos[a:e])
        ops.embed(torch.full((1,), BOS, dtype=torch.int64, device=dev), tb["speech_emb"], x[b, e - P0:e - P0 + 1], table2=tb["wpe"], ids2=pos[e:e + 1])
    posr = torch.arange(P0, S, dtype=torch.int32, device=dev).repeat(B)
    crow = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(Sx)
    last = torch.tensor([b * Sx + s0[b] - P0 - 1 for b in range(B)], device=dev)
    return x, posr, crow, last


def numpy_layout(tb, text_tokens, ce, cond_lens, P0, llama):
    """The same tensor from the definition of the layout (float32 NumPy; x * 1 + y and x * 0 + y are exact, so this is bit-exact too)."""
    t = {k: v.cpu().numpy() for k, v in tb.items()}
    B, D = len(text_tokens), t["text_emb"].shape[1]
    n_bos = 2 if llama else 1
    S = max(cond_lens[b] + int(text_tokens[b].numel()) + n_bos for b in range(B))
    rows = 2 * B if llama else B
    x = np.zeros((rows, S, D), np.float32)
    for r in range(rows):
        b, P = r % B, cond_lens[r % B]
        ids = text_tokens[b].numpy()
        x[r, :P] = ce[b].cpu().numpy()[:P] if ce is not None else 0
        for i, tok in enumerate(ids):
            scale = np.float32(0.0 if (llama and r >= B) else 1.0)
            x[r, P + i] = t["text_emb"][tok] * scale + (t["text_pos"][i] if llama else t["wpe"][P + i])
        for j in range(n_bos):
            p = P + len(ids) + j
            x[r, p] = t["speech_emb"][BOS] + (t["speech_pos"][0] if llama else t["wpe"][p])
    return x[:, P0:]


def call_kernel(ops, tb, text_tokens, ce, cond_lens, P0, llama):
    """ops.prefill_embed with one conditioning slot per utterance (or none behind a cached prefix)."""
    cond = None
    if P0 == 0:
        cond = torch.zeros(len(ce), max(c.shape[0] for c in ce), ce[0].shape[1], device=ce[0].device)
        for i, c in enumerate(ce):
            cond[i, :c.shape[0]] = c
    kw = dict(text_emb=tb["text_emb"], speech_emb=tb["speech_emb"], bos_id=BOS, cond_lens=cond_lens, cond=cond, cond_slots=list(range(len(text_tokens))), pos0=P0)
    if llama:
        return ops.prefill_embed(text_tokens, text_pos=tb["text_pos"], speech_pos=tb["speech_pos"], n_bos=2, cfg=True, abs_pos=False, **kw)
    return ops.prefill_embed(text_tokens, text_pos=tb["wpe"], speech_pos=tb["wpe"], n_bos=1, cfg=False, abs_pos=True, **kw)


def paste_by_copy(kc, vc, prefixes, voice_of_row):
    """The broadcast copy_ form (VoicePrefixCache._paste_voice_prefix of the parent), one pair of copies per voice."""
    for v, (k, val) in enumerate(prefixes):
        rows = [r for r, w in enumerate(voice_of_row) if w == v]
        if rows:
            P = k.shape[2]
            idx = torch.tensor(rows, device=kc.device)
            kc[:, idx, :, :P] = k[:, None]
            vc[:, idx, :, :P] = val[:, None]
