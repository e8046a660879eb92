"""GPU (-m gpu), kernel level: the two alignment-guard kernels against the restatements of guard_common.py, and the real sampler on what the update leaves.

cbx_guard_text_mass_f32 (ops.guard_text_mass): |err| <= 2e-5 (1 + |ref|) against the fp64 restatement, MASS_TOL of word_times_common.py -- the project's bound for
this same definition.  Text lengths 1, 2, 63, 64, 65, 1024; contexts at which the text is just visible (34 + t_len), 255 / 256 / 257 around the 256 keys a
workgroup covers per pass, and 4608, the cap; q as 0, 2 and 4 split-K parts; heads 0 and 15 of 16, a repeated head; B = 1, 3, 8, 9; rows at one position and
rows each at its own; a done row and the columns beyond t_len keep a sentinel; NaN in the cache beyond the context, in the unconditional rows' q and, in device
memory right behind the view the kernel gets, in the unused parts of the 4-part qkv / ssq buffers changes no bit.
cbx_guard_update_f32 (ops.guard_update): history row, state, sums, trace, ban column and forced logits compared EXACTLY with the fp32 state machine, step by step
over the designed trajectories of test_guard_host.py, at V = 8194 in logit rows padded to 8200 (the padding keeps its sentinel), m = 1, 3, 6, 64, 65, 1024.
The sampler (ops.t3_sample, unchanged): while the ban column holds EOS it is never sampled from logits peaked on it; from forced logits it is sampled for the
uniforms 0 and 0.999999 at temperatures 0.05 and 5, cfg_weight 0 and 3, repetition penalty 2.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added.  Do not rename this file without extending
_KERNEL_LEVEL_MODULES there."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import guard_common as G  # noqa: E402

pytestmark = pytest.mark.gpu

# (t_len of row 0, context, q parts, B, H, heads)
MASS = [
    (1, 35, 0, 1, 4, [0]),
    (2, 36, 2, 3, 4, [3, 3, 1]),          # a repeated head
    (63, 255, 4, 8, 4, [0, 3]),
    (64, 256, 0, 3, 16, [0, 15]),
    (65, 257, 2, 8, 16, [15, 0]),
    (65, 34 + 65, 4, 1, 4, [2]),          # the text just visible
    (1024, 34 + 1024, 0, 1, 4, [1]),
    (1024, 4608, 2, 1, 16, [0, 15]),      # both caps
    (63, 4608, 4, 3, 4, [3]),
    (40, [300, 74, 255, 256, 257, 1000, 99, 512, 40], 2, 9, 4, [1, 2]),   # ragged: every row at its own position; B = 9
    (7, [41, 300, 64], 0, 3, 4, [0]),
]


@pytest.mark.parametrize("t_len,ctx,nparts,B,H,heads", MASS, ids=[f"t{c[0]}_ctx{c[1] if isinstance(c[1], int) else 'ragged'}_p{c[2]}_B{c[3]}" for c in MASS])
def test_guard_text_mass_is_the_restated_softmax_slice(dev, t_len, ctx, nparts, B, H, heads):
    """The poisoned and the clean inputs differ in what the kernel must not read: the cache beyond each row's context, the unconditional rows' q, and -- in
    DEVICE memory right behind the view the kernel is given -- the parts >= nparts of the 4-part qkv and ssq buffers and the ssq entries of rows >= B."""
    from chatterbox_amd import ops
    ctxs = [ctx] * B if isinstance(ctx, int) else ctx
    tl = [t_len] + [1, 2, t_len, 5, t_len, 1, 2, t_len][: B - 1]
    tl = [min(t, c - 34) for t, c in zip(tl, ctxs)]
    done = [0] * B
    if B >= 3:
        done[B - 1] = 1
    kw, seed = dict(max_ctx=min(max(ctxs) + 3, 4608)), 31 * t_len + ctxs[0] + nparts
    c = G.mass_case(B, H, ctx, tl, nparts, seed, **kw)
    clean = G.mass_case(B, H, ctx, tl, nparts, seed, poison=False, **kw)
    assert np.isnan(c["qkv"][max(nparts, 1):]).all() and np.isnan(c["ssq"][max(nparts, 1):]).all() and np.isnan(c["ssq"][:, B:]).all() and not np.isnan(clean["qkv"]).any()
    with torch.cuda.device(dev):
        p = G.run_mass(ops, dev, c, heads, done=done, slots=len(heads) + 1)
        again = G.run_mass(ops, dev, c, heads, done=done, slots=len(heads) + 1)
        unpoisoned = G.run_mass(ops, dev, clean, heads, done=done, slots=len(heads) + 1)
    print(f"t_len {tl}, context {ctx}, {nparts} parts, heads {heads}: worst err / (1 + |ref|) = {G.check_mass(p, c, heads, done=done):.3g} (bound {G.MASS_TOL})")
    assert np.array_equal(p, again), "two runs are bit-identical"
    assert np.array_equal(p, unpoisoned), "NaN beyond the context, in the unconditional rows or in unused parts reached a result"


def test_guard_text_mass_takes_wide_scores_and_rows_without_rope(dev):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for nparts, rope in ((0, False), (4, True)):
            c = G.mass_case(2, 4, 300, [65, 9], nparts, 9 + nparts, spread=27.0 * (0.5 if nparts else 1), rope=rope)   # scores of about +-80 (the sum of 4 parts doubles the spread)
            for b in range(2):  # text column 2 of head 1 points along q: the row's largest score, so a text probability near 1 is among those compared
                q = G.guard_q64(c["qkv"], c["nparts"], c["ssq"], c["rms_dim"], c["rms_eps"], c["cos"], c["sin"], b, 1, 299, 4)
                c["kc"][b, 1, G.T0 + 2] = (3.0 * q / np.abs(q).max()).astype(np.float32)
            worst = G.check_mass(G.run_mass(ops, dev, c, [1, 2]), c, [1, 2])
            ref = G.guard_mass_ref(c["qkv"], c["nparts"], c["ssq"], c["rms_dim"], c["rms_eps"], c["cos"], c["sin"], c["kc"], c["positions"], [1], c["t_len"], G.T0, 0.125, 4)
            print(f"wide scores, {nparts} parts, rope {rope}: worst {worst:.3g}; largest text probability {max(float(r.max()) for r in ref[0]):.3g}")
        c = G.mass_case(2, 2, 40, [6, 7], 2, 10)
        c["t_len"][1] = 8                       # 34 + 8 > 41: not yet visible to the query -- the row writes nothing
        p = G.run_mass(ops, dev, c, [0])
    assert (p[0, 1] == -7.0).all() and (p[0, 0, :6] != -7.0).all()


@pytest.mark.parametrize("m", [1, 3, 6, 64, 65, 1024])
def test_guard_update_is_the_state_machine(dev, m):
    from chatterbox_amd import ops
    toks = list(range(100, 400))
    walk = list(range(min(6, m - 1), m - 1, 6)) + [m - 1]   # steps of `ahead` to the last token
    if m == 1024:
        walk = [1000, 1006, 1012, 1018, 1023]               # (the position starts wherever the window allows: back = 0 .. ahead = 1023)
    with torch.cuda.device(dev):
        far = dict(ahead=1023) if m == 1024 else {}
        assert G.drive(ops, dev, walk + [m - 1] * 6, m, G.thr_row(tail=2.0, min_text=0, **far), toks) is not None, "tail"
        if m > 8:
            assert G.drive(ops, dev, walk + [2] * 5, m, G.thr_row(repeat=1.5, **far), toks, n_sel=3) is not None, "repeat"
            assert G.drive(ops, dev, [1, 2, 3, 4, 5], m, G.thr_row(), [7, 7, 8, 8, 8, 8, 1]) == 5, "run; the steps 1, 2 < token_run cannot fire"
            assert G.drive(ops, dev, [1, 2, 20, 3, 0, 40], m, G.thr_row(), toks, n_sel=1) is None, "jumps outside the window"
            assert G.drive(ops, dev, [1, 2, 3], m, G.thr_row(), toks, tie=True) is None, "an argmax tie takes the lowest t"


def test_guard_update_rows_that_are_done_or_have_fired_do_nothing(dev):
    from chatterbox_amd import ops
    st = G.new_state(3)
    st["state"][2, 3] = 2     # row 2 has fired before
    a = G.peaked(6, [1, 2, 3])
    with torch.cuda.device(dev):
        d = G.run_update(ops, dev, a, [6, 6, 6], [1, 1, 1], [G.thr_row()] * 3, st, [[5, 6]] * 3, done=[1, 0, 0])
    assert (d["trace"][[0, 2]] == -9).all() and d["trace"][1, 1] == (2 | 1 << 17) and (d["dp"][[0, 2]] == 0.25).all() and d["dp"][1, 6] == G.EOS
    assert (d["mass"][[0, 2]] == d["sentinel"]).all() and st["state"][0].tolist() == [0] * 8 and st["state"][2].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]
    assert (d["logits"] == 1.5).all()


def _sample(ops, dev, logits, dp, uniform, B):
    """ONE real ops.t3_sample launch (the Llama engine's arguments: CFG row pairs, the reference's processor order) at step 1 -> the B sampled ids"""
    ms = 4
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    seen = torch.zeros(B, G.V, dtype=torch.uint8, device=dev)
    seen[:, G.EOS] = 1    # the repetition penalty applies to EOS itself
    out = torch.zeros(B, ms, dtype=torch.int64, device=dev)
    done, step = i32(B), i32(B) + 1
    ops.t3_sample(logits=logits, ld=logits.stride(0), V=G.V, B=B, cfg=1, order=0, eos_token=G.EOS, dev_params=dp, seen=seen, uniforms=torch.full((B, ms), float(uniform), device=dev),
                  max_steps=ms, step=step, out_tokens=out, done=done, n_generated=i32(B), next_ids=torch.zeros(2 * B, dtype=torch.int64, device=dev), next_pos_ids=i32(2 * B),
                  positions=i32(2 * B), ctx_lens=i32(2 * B))
    return out[:, 1].tolist(), done.tolist()


@pytest.mark.parametrize("temperature", [0.05, 5.0])
@pytest.mark.parametrize("cfg_weight", [0.0, 3.0])
def test_the_sampler_obeys_the_ban_and_samples_eos_from_forced_logits(dev, temperature, cfg_weight):
    from chatterbox_amd import ops
    B, m = 2, 12
    g = torch.Generator().manual_seed(5)
    with torch.cuda.device(dev):
        for uniform in (0.0, 0.999999):
            # ---- held: the update bans EOS (not complete, m >= min_text); the logits are peaked on EOS in both CFG rows
            logits = torch.randn(2 * B, G.V + 6, generator=g).to(dev)
            logits[:, G.EOS] = 40.0
            st = G.new_state(B)
            d = G.run_update(ops, dev, G.peaked(m, [1, 1]), [m] * B, [1] * B, [G.thr_row()] * B, st, [[5, 6]] * B, logits=logits)
            dp = torch.tensor([[cfg_weight, temperature, 0.05, 1.0, 2.0, 0.0, 0.0, 0.0]] * B, device=dev)
            dp[:, 6] = torch.from_numpy(d["dp"][:, 6]).to(dev)
            assert dp[:, 6].tolist() == [float(G.EOS)] * B
            toks, done = _sample(ops, dev, logits, dp, uniform, B)
            assert all(t != G.EOS for t in toks) and done == [0] * B, (toks, "EOS was sampled under the ban")
            # ---- forced: a text of 3 tokens is complete at once and tail = 0 then holds; both rows become the pattern, the ban is lifted, and the sampler
            # writes EOS and sets done
            st = G.new_state(B)
            d = G.run_update(ops, dev, G.peaked(3, [1, 1]), [3] * B, [1] * B, [G.thr_row(tail=0.0)] * B, st, [[5, 6]] * B, logits=logits)
            assert (d["trace"][:, 1] >> 18 == 1).all() and (d["dp"][:, 6] == -1).all()
            dp[:, 6] = -1.0
            toks, done = _sample(ops, dev, logits, dp, uniform, B)
            assert toks == [G.EOS] * B and done == [1] * B, (toks, uniform)
