"""The CFM solve as two interleaved half-batch chains (-m gpu; cbx_cfm_t.b_split, FlowEngine.cfm_chains): `cbx_cfm_solve` runs a batch of B >= 2
utterances as two independent solves over row slices, the second on a stream of the library's own between one fork and one join event.  Every kernel
of the solve works per utterance (GEMM rows, attention per row group and head, LayerNorm per row, the Euler update per cond / uncond pair), so the mel
must be BIT-identical to the one-chain solve -- and the caller's stream must order everything after the call, as it does with one chain.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(dev, meanflow):
    """The full-depth synthetic FlowEngine (12 mid blocks), built once per numerics and shared."""
    from chatterbox_amd import synth
    from chatterbox_amd.s3gen import FlowEngine
    if meanflow not in _ENGINES:
        _ENGINES[meanflow] = FlowEngine(synth.s3gen_state_dict(0, meanflow=meanflow, n_enc=1, n_up_enc=1), dev, meanflow=meanflow)
        assert _ENGINES[meanflow].n_mid == 12 and _ENGINES[meanflow].c_seam
    return _ENGINES[meanflow]


def _inputs(dev, B, T, seed=0):
    """A ragged batch: full rows, a shorter one, and -- from B = 3 on -- one row of the minimum length (one token = 2 mel frames)."""
    from chatterbox_amd import synth
    mu, cond, z = (synth.randn((B, T, 80), seed=seed + s).to(dev) for s in (1, 2, 3))
    cond[:, T // 3:] = 0
    spk = synth.randn((B, 80), seed=seed + 4).to(dev)
    lens = torch.tensor([T, T - 7, 2, T - 1, T // 2][:B], dtype=torch.int32, device=dev)
    return mu, lens, spk, cond, z


def _solve(eng, chains, args, n_steps):
    """(mel, two-chain solves the call made)"""
    from chatterbox_amd import ops
    from chatterbox_amd._lib import lib
    eng.cfm_chains = chains
    n0 = lib.cbx_cfm_two_chain_solves()
    with ops.gemm_precision(16), torch.inference_mode():
        out = eng.cfm(*args, n_steps=n_steps).clone()
    return out, lib.cbx_cfm_two_chain_solves() - n0


@pytest.mark.parametrize("meanflow", [False, True])
@pytest.mark.parametrize("B,T", [(2, 40), (3, 38), (5, 66), (2, 64), (5, 300)])
def test_two_chains_give_the_mel_of_one_chain_bit_for_bit(dev, meanflow, B, T):
    """With CFG (3 steps) and without (the meanflow engine, 2 steps): an even split, an odd split of a ragged batch with a minimum-length row (T % 4 != 0:
    the separate q | k and V^T projections), halves of 3 and 2 utterances; a half of exactly CFM_HALF_MIN_ROWS rows without CFG (a smaller half keeps the
    call on one chain: (2, 40) and (3, 38) without CFG); and, with CFG, a batch above whose halves are below the grid sizes at which the plane attention
    (128 workgroups) and the wide plane GEMMs (128 tiles) change their automatic form."""
    from chatterbox_amd.s3gen import CFM_HALF_MIN_ROWS, cfm_halves
    eng, args, n_steps = _engine(dev, meanflow), _inputs(dev, B, T), 2 if meanflow else 3
    one, n_one = _solve(eng, 1, args, n_steps)
    two, n_two = _solve(eng, 2, args, n_steps)
    forks = int(min((1 if meanflow else 2) * n * T for _, n, _ in cfm_halves(B, not meanflow, 2)) >= CFM_HALF_MIN_ROWS)
    assert forks == (0 if meanflow and (B, T) in ((2, 40), (3, 38)) else 1)
    assert (n_one, n_two) == (0, forks), "cfm_chains = 1 forks nothing, cfm_chains = 2 forks once where both halves are large enough"
    assert one.shape == two.shape == (B, T, 80) and torch.isfinite(one).all() and one.abs().max() > 0
    assert torch.equal(one, two), f"max |diff| {(one - two).abs().max().item():.3e}"


@pytest.mark.parametrize("meanflow", [False, True])
def test_one_utterance_takes_the_one_chain_path(dev, meanflow):
    eng, args = _engine(dev, meanflow), _inputs(dev, 1, 40)
    one, n_one = _solve(eng, 1, args, 2)
    two, n_two = _solve(eng, 2, args, 2)
    assert (n_one, n_two) == (0, 0), "B = 1 is not split"
    assert torch.equal(one, two)


def test_the_default_forks_inside_the_two_chain_schedule_only(dev, B=3, T=38):
    """cfm_chains = 0, the default: one chain as the engine is built and after co_resident(True); two once the schedule's flag is set -- on the
    co-resident forms, where the two-chain mel is the one-chain mel, too."""
    eng, args = _engine(dev, False), _inputs(dev, B, T)
    try:
        assert _solve(eng, 0, args, 2)[1] == 0
        eng.co_resident(True)
        one, n_one = _solve(eng, 0, args, 2)
        eng.two_chain_schedule = True
        auto, n_auto = _solve(eng, 0, args, 2)
        assert (n_one, n_auto) == (0, 1) and torch.equal(one, auto)
    finally:
        eng.co_resident(False)
        eng.two_chain_schedule = False


@pytest.mark.parametrize("priority", [0, -1])
def test_back_to_back_calls_on_a_side_stream_are_ordered_by_that_stream(dev, priority, B=3, T=38):
    """Fork: the second chain must not start before what the caller's stream holds (the inputs are written on it right before the call).  Join: a copy
    enqueued on the caller's stream right behind the call must see both halves' rows.  Two calls with different inputs, nothing synchronised in between;
    at normal and at high stream priority (the side stream and its events exist once per priority)."""
    from chatterbox_amd import ops
    from chatterbox_amd._lib import lib
    eng = _engine(dev, False)
    a, b = _inputs(dev, B, T, seed=10), _inputs(dev, B, T, seed=20)
    want = [_solve(eng, 1, x, 2)[0] for x in (a, b)]
    torch.cuda.synchronize()
    eng.cfm_chains = 2
    st, n0 = torch.cuda.Stream(device=dev, priority=priority), lib.cbx_cfm_two_chain_solves()
    host = [torch.empty(B, T, 80, pin_memory=True) for _ in range(2)]
    with torch.cuda.stream(st), ops.gemm_precision(16), torch.inference_mode():
        for x, h in zip((a, b), host):
            fresh = tuple(t.clone() for t in x)  # written on `st` in front of the call: the fork has to order them for the second chain too
            h.copy_(eng.cfm(*fresh, n_steps=2), non_blocking=True)
    st.synchronize()
    assert lib.cbx_cfm_two_chain_solves() - n0 == 2
    for h, w in zip(host, want):
        assert torch.equal(h, w.cpu()), f"max |diff| {(h - w.cpu()).abs().max().item():.3e}"


@pytest.mark.parametrize("guard", ["engine", "library"])
def test_a_call_inside_a_capture_forks_nothing(dev, guard, monkeypatch, B=3, T=38):
    """A fork inside a capture would give the graph parallel branches.  `engine`: FlowEngine.cfm sees the capture and passes b_split = 0, the one-chain
    launches.  `library`: with the engine's look at the capture switched off the descriptor carries the split, and cbx_cfm_solve itself finds the stream
    capturing and launches the halves one after the other on it.  The capture is ended and dropped, never replayed."""
    from chatterbox_amd import ops
    from chatterbox_amd._lib import lib
    eng, args = _engine(dev, False), _inputs(dev, B, T)
    _solve(eng, 2, args, 2)  # (everything the engine builds lazily exists before the capture)
    torch.cuda.synchronize()
    eng.cfm_chains = 2
    splits, inner = [], eng._cfm_solve_c
    monkeypatch.setattr(eng, "_cfm_solve_c", lambda *a, **k: (splits.append(k.get("b_split", 0)), inner(*a, **k))[1])
    n0, g = lib.cbx_cfm_two_chain_solves(), torch.cuda.CUDAGraph()
    with ops.gemm_precision(16), torch.inference_mode(), torch.cuda.graph(g):
        if guard == "library":
            monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        eng.cfm(*args, n_steps=2)
        monkeypatch.undo()
    del g
    torch.cuda.synchronize()
    assert splits == [0 if guard == "engine" else 2]
    assert lib.cbx_cfm_two_chain_solves() == n0, "no fork while the stream was capturing"
    assert _solve(eng, 2, args, 2)[1] == 1, "and two chains again after it"


@pytest.mark.parametrize("B", [2, 3])
def test_vocode_through_the_engine_gives_the_same_waveforms(dev, B, P=6):
    """ChatterboxEngine.vocode (encoder, CFM, vocoder) for a ragged batch: the waveforms with two chains are those with one."""
    import math
    from chatterbox_amd import synth
    from chatterbox_amd._lib import lib
    from chatterbox_amd.engine import ChatterboxEngine
    if "voc" not in _ENGINES:
        _ENGINES["voc"] = ChatterboxEngine(synth.t3_state_dict(2, 0), synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1), dev, n_t3_layers=2)
    eng, ns = _ENGINES["voc"], [12, 9, 5][:B]
    ref, toks = synth.s3gen_ref(n_prompt_tokens=P), [synth.speech_tokens(n, seed=30 + n) for n in ns]
    z = synth.randn((B, 2 * (P + max(ns)), 80), seed=5).to(dev)
    phase = (synth.rand((B, 9, 1), seed=6) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = synth.randn((B, 9, 960 * max(ns)), seed=7)
    out = {}
    for chains in (1, 2):
        eng.flow.cfm_chains, n0 = chains, lib.cbx_cfm_two_chain_solves()
        wavs, mel = eng.vocode(toks, ref, z=z, phase=phase, noise=noise, n_cfm_timesteps=2)
        assert lib.cbx_cfm_two_chain_solves() - n0 == chains - 1
        out[chains] = ([w.clone() for w in wavs], mel.clone())
    assert torch.equal(out[1][1], out[2][1])
    for w1, w2, n in zip(out[1][0], out[2][0], ns):
        assert w1.numel() == w2.numel() >= 480 * n and w1.abs().max() > 0 and torch.equal(w1, w2)


@pytest.mark.parametrize("host_threads", [True, False])
def test_the_throughput_schedule_asks_for_two_chains_and_hands_one_back(dev, host_threads, L=2, steps=10, P=6):
    """synthesize_pipelined in its default form (co-resident forms, T3 enqueued by a second host thread) solves every job's CFM as two chains; its
    one-thread form, which was not measured, keeps one; either way the flag is down again when the schedule returns.  (That the schedule's results are the
    serial ones is tests/test_models_gpu.py::test_pipelined_equals_serial.)"""
    from chatterbox_amd import synth
    from chatterbox_amd._lib import lib
    from chatterbox_amd.engine import ChatterboxEngine
    if "voc" not in _ENGINES:
        _ENGINES["voc"] = ChatterboxEngine(synth.t3_state_dict(2, 0), synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1), dev, n_t3_layers=2)
    eng, cond, ref = _ENGINES["voc"], synth.t3_cond(), synth.s3gen_ref(n_prompt_tokens=P)
    eng.flow.cfm_chains = 0
    jobs = [dict(text_tokens=[synth.text_tokens(8 + j, seed=10 + j), synth.text_tokens(12, seed=20 + j)], t3_conds=cond, gen_ref=ref,
                 uniforms=synth.rand((2, steps), seed=30 + j).to(dev)) for j in range(2)]
    n0, flags = lib.cbx_cfm_two_chain_solves(), []
    for _ in eng.synthesize_pipelined(jobs, host_threads=host_threads, max_new_tokens=steps, ban_eos=True, ban_from=6561, n_cfm_timesteps=2,
                                      temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0):
        flags.append(eng.flow.two_chain_schedule)
    assert lib.cbx_cfm_two_chain_solves() - n0 == (2 if host_threads else 0), "T = 2 (P + steps) = 32: each half has 2 rows x 32 = 64 rows"
    assert flags[0] == host_threads and eng.flow.two_chain_schedule is False and eng.flow.chains() == 1
