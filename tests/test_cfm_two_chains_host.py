"""Host side of the two-chain CFM solve (no GPU): the row order FlowEngine.cfm lays a batch out in for cbx_cfm_t.b_split, the descriptor field itself,
and -- on the SIMT emulator, which runs the two half-batches one after the other -- the row slicing of cbx_cfm_solve against the one-chain solve."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("B", range(1, 10))
def test_layout_then_gather_is_the_identity_and_each_half_pairs_its_own_rows(B, cfg):
    from chatterbox_amd.s3gen import cfm_halves, cfm_result_rows, cfm_row_order
    per = 2 if cfg else 1
    assert cfm_halves(B, cfg, 1) == [(0, B, 0)] and cfm_result_rows(B, cfg, 1) == list(range(B))
    assert cfm_row_order(B, cfg, 1) == [(b, False) for b in range(B)] + ([(b, True) for b in range(B)] if cfg else [])
    halves, order, res = cfm_halves(B, cfg, 2), cfm_row_order(B, cfg, 2), cfm_result_rows(B, cfg, 2)
    if B == 1:
        assert halves == cfm_halves(B, cfg, 1), "one utterance is not split"
        return
    (u0, n0, r0), (u1, n1, r1) = halves
    assert (u0, r0, u1, r1) == (0, 0, n0, per * n0) and n0 == (B + 1) // 2 and n0 + n1 == B and n1 >= 1, "ceil(B / 2) and floor(B / 2), contiguous in the rows"
    assert len(order) == per * B and sorted(order) == sorted((b, u) for b in range(B) for u in ([False, True] if cfg else [False])), "every row once"
    assert [order[r] for r in res] == [(b, False) for b in range(B)], "gathering the result rows gives the utterances' cond rows in order"
    for u, n, r in halves:  # cbx_cfm_euler_f32 on a half pairs row i with row n + i
        for i in range(n):
            assert order[r + i] == (u + i, False) and (not cfg or order[r + n + i] == (u + i, True))


def test_b_split_sits_in_the_alignment_slot_of_the_descriptor():
    """The field took the 4 bytes in front of cbx_cfm_t.T: no size or offset of the v16 descriptor moved (tests/test_host_logic.py compares every offset
    with the C compiler's), so the ABI number stays, and a zeroed descriptor is the one-chain call."""
    import ctypes
    from chatterbox_amd import _lib
    C = _lib.CfmSolve
    assert C.fused_ln.offset == 24 and C.b_split.offset == 28 and C.T.offset == 32 and ctypes.sizeof(C) % 8 == 0
    assert C().b_split == 0
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    assert "#define CBX_ABI_VERSION 16" in hdr and _lib.ABI_VERSION == 16
    assert "zero-initialised" in hdr and "zero-initialise" in open(os.path.join(ROOT, "INTEGRATION.md")).read(), "what the reuse of padding bytes asks of a C host"
    assert "cbx_cfm_two_chain_solves" not in hdr, "the fork counter of the tests is exported, but no part of the public header"
    assert _lib.lib.cbx_cfm_two_chain_solves() >= 0


def test_the_automatic_choice_is_two_chains_inside_the_schedule_that_asks_for_them_only():
    """cfm_chains = 0 follows the measurement: two chains while `two_chain_schedule` is set -- engine.synthesize_pipelined sets it for
    its run and clears it --, one otherwise; co_resident() has no say; 1 and 2 are what they say."""
    from chatterbox_amd.s3gen import FlowEngine
    eng = object.__new__(FlowEngine)
    eng.cfm_chains, eng.two_chain_schedule = 0, False
    for on in (False, True):
        eng.co_resident(on)
        assert eng.chains() == 1
    eng.two_chain_schedule = True
    assert eng.chains() == 2
    for c in (1, 2):
        eng.cfm_chains = c
        for flag in (False, True):
            eng.two_chain_schedule = flag
            assert eng.chains() == c
    eng.cfm_chains = 3
    with pytest.raises(ValueError):
        eng.chains()
    src = open(os.path.join(ROOT, "chatterbox_amd", "engine.py")).read()
    assert src.count("self.flow.two_chain_schedule = False") == 2 and src.count("self.flow.two_chain_schedule = ") == 3, "set once, cleared on both ways out"


@pytest.fixture(scope="module")
def emu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import harness
    with harness.emulated() as lib:
        yield lib


def test_half_batch_slices_on_the_emulator(emu, meanflow=False, B=3, T=32):
    """cbx_cfm_solve with b_split (the emulator has no streams: half 0, then half 1) against the one-chain solve, bit for bit: an odd split of a ragged
    batch with CFG, the smaller half of exactly CFM_HALF_MIN_ROWS rows.  Fresh plane buffers hold NaNs on the emulator, so a half that read rows the other
    one owns would show."""
    from chatterbox_amd import ops, synth
    from chatterbox_amd.s3gen import FlowEngine
    CPU = torch.device("cpu")
    eng = FlowEngine(synth.s3gen_state_dict(0, meanflow=meanflow, n_mid=1, n_enc=1, n_up_enc=1), CPU, meanflow=meanflow)
    mu, cond, z = (synth.randn((B, T, 80), seed=s) for s in (1, 2, 3))
    cond[:, T // 3:] = 0
    spk, lens = synth.randn((B, 80), seed=4), torch.tensor([T, T - 7, 2], dtype=torch.int32)
    out, splits, inner = {}, [], eng._cfm_solve_c
    eng._cfm_solve_c = lambda *a, **k: (splits.append(k.get("b_split", 0)), inner(*a, **k))[1]
    for chains in (1, 2):
        eng.cfm_chains = chains
        with ops.gemm_precision(16), torch.inference_mode():
            out[chains] = eng.cfm(mu, lens, spk, cond, z, n_steps=2).clone()
    assert splits == [0, 2] and emu.cbx_cfm_two_chain_solves() == 0, "the descriptor carried the split; the emulator forks nothing"
    assert torch.isfinite(out[1]).all() and out[1].abs().max() > 0
    assert torch.equal(out[1], out[2]), f"max |diff| {(out[1] - out[2]).abs().max().item():.3e}"
