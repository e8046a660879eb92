"""GPU (-m gpu): `speed=` through the engines and the public API on synthetic 2-layer models -- speed None / 1.0 is bitwise the call without the argument, a scaled
vocode() is bitwise the chain flow.inference -> ops.mel_time_scale -> hift.inference(lens=O) composed in the test, every waveform has max(1, floor(K / s)) * 480
samples where speed 1 gives K * 480, a request's audio at a (seed, speed) does not depend on the batch around it (the comparison and the tolerance of
test_seeded_api_gpu.py), and a bad speed raises before anything is launched.  The kernel-level tests are in test_turbo_stream_mel_speed_kernels_gpu.py."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_seeded_api_gpu as A  # noqa: E402  (read-only import: _check_compositions, the recording wrapper, the stand-in tokenizer, TOL_WAV_E2E_8S behind them)

pytestmark = pytest.mark.gpu

P, NS = 6, (12, 20, 16)          # prompt tokens; speech tokens per utterance
SPEEDS = [0.8, 1.25, 1.0]


def _floor_len(K, s):
    """the trim rule, restated: max(1, floor(K / s)) frames of 480 samples"""
    return max(1, int(math.floor(K / s)))


@pytest.fixture(scope="module")
def voc(dev):
    """One engine, its inputs and the unscaled call, shared (and left unchanged) by the vocode tests."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine
    eng = ChatterboxEngine(synth.t3_state_dict(2, 0), synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1), dev, n_t3_layers=2)
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate(NS)]
    B, Nmax = len(NS), max(NS)
    z = synth.randn((B, 2 * (P + Nmax), 80), seed=5).to(dev)
    phase = (synth.rand((B, 9), seed=6) * 2 - 1) * math.pi
    phase[:, 0] = 0
    noise = synth.randn((B, 9, 960 * Nmax), seed=7)
    base, mel = eng.vocode(st, ref, z=z, phase=phase, noise=noise, n_cfm_timesteps=2)
    return dict(eng=eng, ref=ref, st=st, z=z, phase=phase, noise=noise, base=base, mel=mel)


def test_speed_none_and_one_are_bitwise_the_call_without_the_argument(dev, voc):
    eng, kw = voc["eng"], dict(z=voc["z"], phase=voc["phase"], noise=voc["noise"], n_cfm_timesteps=2)
    assert [w.numel() for w in voc["base"]] == [960 * n for n in NS]
    for speed in (None, 1.0, [1.0, None, 1]):
        wavs, mel = eng.vocode(voc["st"], voc["ref"], speed=speed, **kw)
        assert torch.equal(mel, voc["mel"])
        for b, (w, w0) in enumerate(zip(wavs, voc["base"])):
            assert w.shape == w0.shape and torch.equal(w, w0), f"speed={speed!r}, utterance {b}"


@pytest.mark.parametrize("drop_last_token", [False, True])
def test_scaled_vocode_equals_the_composed_chain_and_follows_the_trim_rule(dev, voc, drop_last_token):
    """vocode(speed=[0.8, 1.25, 1.0]) with z, phase and noise injected (noise at the stretched mel's size) is torch.equal to flow.inference -> ops.mel_time_scale
    over M_b = 2 n_b frames -> hift.inference(lens=O_b) composed here from the same inputs, cut to max(1, floor(K_b / s_b)) * 480 samples, K_b from the call
    without speed; the returned mel is the unscaled flow mel."""
    from chatterbox_amd import ops, synth
    eng, st, ref = voc["eng"], voc["st"], voc["ref"]
    B, Nmax = len(NS), max(NS)
    base, _ = eng.vocode(st, ref, z=voc["z"], phase=voc["phase"], noise=voc["noise"], n_cfm_timesteps=2, drop_last_token=drop_last_token)
    K = [w.numel() // 480 for w in base]
    assert all(w.numel() == 480 * k for w, k in zip(base, K)) and K == [2 * (n - 1) if drop_last_token else 2 * n for n in NS]
    O = [_floor_len(2 * n, s) for n, s in zip(NS, SPEEDS)]
    assert O == [30, 32, 32]
    noise = synth.randn((B, 9, 480 * max(O)), seed=8)
    got, mel = eng.vocode(st, ref, z=voc["z"], phase=voc["phase"], noise=noise, n_cfm_timesteps=2, drop_last_token=drop_last_token, speed=SPEEDS)
    assert torch.equal(mel, voc["mel"]), "the returned mel stays the unscaled flow mel"
    with torch.cuda.device(dev), torch.inference_mode():
        tok = torch.zeros(B, Nmax, dtype=torch.long)
        for b, t in enumerate(st):
            tok[b, : NS[b]] = t
        fmel = eng.flow.inference(tok.to(dev), torch.tensor(NS, dtype=torch.int32).to(dev), ref, z=voc["z"], n_steps=2)
        assert torch.equal(fmel, voc["mel"])
        smel, out_lens = ops.mel_time_scale(fmel, SPEEDS, in_lens=[2 * n for n in NS])
        assert out_lens.tolist() == O and smel.shape == (B, max(O), 80)
        wav, _ = eng.hift.inference(smel, phase=voc["phase"], noise=noise, lens=out_lens, fade=True)
        torch.cuda.synchronize()
    for b in range(B):
        n = 480 * _floor_len(K[b], SPEEDS[b])
        assert got[b].shape == (n,), f"utterance {b}: {got[b].numel()} samples, the rule gives {n}"
        assert torch.equal(got[b], wav[b, :n]), f"utterance {b}"
    assert torch.equal(smel[2, : 2 * NS[2]], fmel[2, : 2 * NS[2]]), "rate 1.0 inside a scaled batch is the identity map"


def test_seeded_scaled_vocode_sizes_its_noise_from_the_stretched_mel(dev, voc):
    """Nothing injected but z: the seeded phase / noise are filled at the stretched mel's size (ops.seeded_noise over 480 * max O_b samples), and a row at rate 1.0
    inside a scaled batch reads the very noise columns its unscaled call reads."""
    from chatterbox_amd import ops
    eng, st, ref = voc["eng"], voc["st"], voc["ref"]
    seeds = [11, 2 ** 40, 13]
    O = [_floor_len(2 * n, s) for n, s in zip(NS, SPEEDS)]
    a, _ = eng.vocode(st, ref, z=voc["z"], n_cfm_timesteps=2, seeds=seeds, speed=SPEEDS)
    b, _ = eng.vocode(st, ref, z=voc["z"], n_cfm_timesteps=2, phase=ops.seeded_phase(seeds, dev), noise=ops.seeded_noise(seeds, 480 * max(O), dev), speed=SPEEDS)
    assert [w.numel() for w in a] == [480 * o for o in O] and all(torch.equal(x, y) for x, y in zip(a, b))
    c, _ = eng.vocode(st[2:], ref, z=voc["z"][2:, : 2 * (P + NS[2])], n_cfm_timesteps=2, seeds=seeds[2:])
    err = A._rmse(a[2].cpu(), c[0].cpu())
    print(f"rate 1.0 inside a scaled batch vs its own unscaled call: RMSE {err:.3e}")
    assert err <= A.TOL_WAV_E2E_8S


# ----------------------------------------------------------------------------- the public classes
N_TOK = 16
API_SPEEDS = [1.25, 0.8, 1.0]


def _check_class(rec, single, batch, set_max_batch):
    """generate(seed=7, speed=1.25) has the length the rule gives from generate(seed=7) and other audio in its first half second; then per request
    generate_batch(seeds=, speed=) in two request orders, as one device batch and as sub-batches of two, against the single calls (A._check_compositions)."""
    w1, w125 = single(0, seed=7, speed=1.0), single(0, seed=7, speed=1.25)
    assert w1.shape[1] % 480 == 0 and w1.shape[1] >= 480 * 12
    assert w125.shape[1] == 480 * _floor_len(w1.shape[1] // 480, 1.25), (w1.shape, w125.shape)
    n = min(12000, w125.shape[1])
    assert not torch.equal(w125[:, :n], w1[:, :n]), "the first half second at speed 1.25 must not be the unscaled audio"
    assert len(rec) == 1 and rec[7][0] == rec[7][1], "with a seed the tokens do not depend on the speed"
    A._check_compositions(rec, lambda order: batch(order, [API_SPEEDS[k] for k in order]), lambda k: single(k, seed=A.SEEDS[k], speed=API_SPEEDS[k]), set_max_batch, n=3)


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"])
def test_tts_speed_length_rule_and_batch_equals_singles(dev, cls_name, monkeypatch):
    from chatterbox_amd import api, synth
    turbo = cls_name == "ChatterboxTurboTTS"
    monkeypatch.setattr(A, "N_TOK", N_TOK)
    cls = getattr(api, cls_name)
    m = cls.from_synthetic(dev, t3_layers=2)
    m.tokenizer = A._Tok(50000 if turbo else cls._TEXT_VOCAB)
    rec = A._bound_and_record(m.engine, "max_gen_len" if turbo else "max_new_tokens")
    va, vb = A._two_voices(api, synth, turbo=turbo)
    conds = [va, vb, va]
    langs = ["en", "fr", "de"] if cls_name == "ChatterboxMultilingualTTS" else None

    def single(k, seed, speed):
        m.conds = conds[k]
        return m.generate(A.TEXTS[k], *([langs[k]] if langs else []), temperature=A.PER["temperature"][k], top_p=A.PER["top_p"][k], seed=seed, speed=speed)

    def batch(order, speeds):
        pick = lambda v: [v[k] for k in order]
        return m.generate_batch(pick(A.TEXTS), *([pick(langs)] if langs else []), conds=pick(conds), seeds=pick(A.SEEDS), speed=speeds,
                                **{k: pick(v) for k, v in A.PER.items()})

    _check_class(rec, single, batch, lambda mb: setattr(m, "max_batch", mb))


def test_vc_speed_length_rule_and_batch_equals_singles(dev):
    from chatterbox_amd import api, synth
    m = api.ChatterboxVC.from_synthetic(dev)
    rec = A._bound_and_record(m.engine, None)
    toks = [synth.speech_tokens(n, seed=k) for k, n in enumerate((20, 12, 16))]
    refs = [synth.s3gen_ref(seed=11), synth.s3gen_ref(seed=12)]
    ref_of = [refs[0], refs[1], refs[0]]

    def single(k, seed, speed):
        m.ref_dict = ref_of[k]
        return m.generate(s3_tokens=toks[k], seed=seed, speed=speed)

    def batch(order, speeds):
        pick = lambda v: [v[k] for k in order]
        return m.generate_batch(s3_tokens=pick(toks), ref_dicts=pick(ref_of), seeds=pick(A.SEEDS), speed=speeds)

    _check_class(rec, single, batch, lambda mb: setattr(m, "MAX_BATCH", mb or 8))


def test_a_bad_speed_raises_before_anything_is_launched(dev, voc, monkeypatch):
    """Every call into the library goes through ops.lib: a counting proxy in its place sees none while the bad values are refused by vocode, synthesize, and
    generate / generate_batch of a TTS class and of ChatterboxVC -- and sees calls again for a good value."""
    from chatterbox_amd import api, ops, synth
    real, calls = ops.lib, []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)

    eng, st, ref = voc["eng"], voc["st"], voc["ref"]
    tts = api.ChatterboxTTS(eng, A._Tok(704), dev, api.Conditionals(api.T3Cond(**synth.t3_cond()), ref))
    vc = api.ChatterboxVC(eng, dev, ref)
    monkeypatch.setattr(ops, "lib", Spy())
    bad = ((0.49, ValueError), (2.01, ValueError), (float("nan"), ValueError), (True, TypeError), ("1", TypeError), ([1.0, 1.2], ValueError))
    for v, err in bad:
        with pytest.raises(err, match="speed"):
            eng.vocode(st, ref, speed=v)
        with pytest.raises(err, match="speed"):
            eng.synthesize([synth.text_tokens(12)] * 3, synth.t3_cond(), ref, max_new_tokens=4, speed=v)
        with pytest.raises(err, match="speed"):
            tts.generate_batch(["One.", "Two.", "Three."], speed=v)
        with pytest.raises(err, match="speed"):
            vc.generate_batch(s3_tokens=st, speed=v)
        if not isinstance(v, list):
            with pytest.raises(err, match="speed"):
                tts.generate("One.", speed=v)
            with pytest.raises(err, match="speed"):
                vc.generate(s3_tokens=st[0], speed=v)
    assert calls == [], f"refused calls reached the library: {calls[:5]}"
    eng.vocode(st[:1], ref, n_cfm_timesteps=2, speed=1.5)
    assert "cbx_mel_time_scale_f32" in calls
