"""CPU (-m "not gpu"): per-request seeds -- the NumPy Philox4x32-10 restatement against published-algorithm known answers, cbx_rng_fill_f32 on the SIMT emulator
against it, its C ABI, and the host plumbing of `seed=` / `seeds=` on the public classes over a recording engine (nothing is launched)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import seeded_rng_common as R  # noqa: E402

CPU = torch.device("cpu")
TOL_NORMAL = 1e-5  # |n| <= sqrt(48 ln 2) = 5.77; rounding 2 pi u2 to fp32 moves the angle by <= 2^-22 near 2 pi (1.4e-6), plus a few ulp of logf / sqrtf / sincosf


# ----------------------------------------------------------------------------- the restatement itself
def test_numpy_philox_reproduces_the_known_answers():
    for ctr, key, want in R.KAT:
        got = R.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
        assert tuple(int(g[0]) for g in got) == want, (ctr, key)


def test_helper_addressing_is_per_column():
    """A slice of the helper's own fill equals the helper evaluated at that slice (any col0), and the uniform of column 0 of key 0 is the first known answer."""
    assert R.uniform(0, 0, 0, 0, 4).tolist() == [(w >> 8) * 2.0 ** -24 for w in R.KAT[0][2]]
    full_u, full_n = R.uniform(12345, 3, 1, 0, 64), R.normal(12345, 3, 1, 0, 64)
    for col0 in (1, 6, 27):
        assert np.array_equal(R.uniform(12345, 3, 1, col0, 9), full_u[col0: col0 + 9]) and np.array_equal(R.normal(12345, 3, 1, col0, 9), full_n[col0: col0 + 9])
    u = R.uniform(7, 0, 0, 0, 4096)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)


# ----------------------------------------------------------------------------- host helpers
def test_check_seeds_and_key_layout():
    from chatterbox_amd import _lib, ops
    assert ops.check_seeds(None, 3) is None and ops.check_seeds(5, 3) == [5, 5, 5] and ops.check_seeds((1, 2 ** 64 - 1), 2) == [1, 2 ** 64 - 1]
    for bad, err in (([1, 2], ValueError), ([1, 2, -1], ValueError), ([1, 2, 2 ** 64], ValueError), ([1, 2.0, 3], TypeError), ([1, True, 3], TypeError),
                     (1.5, TypeError), ("7", TypeError), (torch.tensor([1, 2, 3]), TypeError), (-1, ValueError), (True, TypeError)):
        with pytest.raises(err):
            ops.check_seeds(bad, 3)
    with pytest.raises(ValueError, match="generator"):
        ops.request_seeds([1], 1, torch.Generator())
    assert (_lib.RNG_T3_UNIFORMS, _lib.RNG_CFM_Z, _lib.RNG_VOC_PHASE, _lib.RNG_VOC_NOISE) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    for name, val in (("CBX_RNG_STREAM_T3_UNIFORMS", 0), ("CBX_RNG_STREAM_CFM_Z", 1), ("CBX_RNG_STREAM_VOC_PHASE", 2), ("CBX_RNG_STREAM_VOC_NOISE", 3),
                      ("CBX_RNG_UNIFORM", 0), ("CBX_RNG_NORMAL", 1)):
        assert f"#define {name} {val}" in hdr, name
    k = ops.rng_keys([0, 2 ** 63 + 7], ops.RNG_VOC_NOISE, substreams=range(9))
    assert k.shape == (18, 4) and k.dtype == torch.int32
    words = k.numpy().view(np.uint32)
    assert words[9 + 4].tolist() == [7, 2 ** 31, 4, 3] and words[2].tolist() == [0, 0, 2, 3]
    assert torch.equal(R.key_tensor([(2 ** 63 + 7, h, 3) for h in range(9)]), k[9:])


# ----------------------------------------------------------------------------- C ABI
def test_rng_entry_point_is_declared_exported_and_bound():
    import ctypes
    import re
    from chatterbox_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cbx.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "chatterbox_amd", "libcbx_hip.so"))
    assert re.search(r"^int cbx_rng_fill_f32\(", hdr, re.M) and hasattr(lib, "cbx_rng_fill_f32") and "cbx_rng_fill_f32" in _lib._SIGS
    assert _lib.lib.cbx_abi_version() == 16, "a new function only: no version step"
    f = _lib.lib.cbx_rng_fill_f32
    buf = (ctypes.c_float * 8)()
    keys = (ctypes.c_int * 4)()
    p, k = ctypes.addressof(buf), ctypes.addressof(keys)
    assert f(None, 8, k, 1, 8, 0, 0, None) == -22 and f(p, 8, None, 1, 8, 0, 0, None) == -22       # null pointers
    assert f(p, 4, k, 1, 8, 0, 0, None) == -22 and f(p, 8, k, -1, 8, 0, 0, None) == -22              # ld_out < n, rows < 0
    assert f(p, 8, k, 1, -1, 0, 0, None) == -22 and f(p, 8, k, 1, 8, 0, 2, None) == -22              # n < 0, unknown distribution
    assert f(p, 8, k, 1, 0, 0, 0, None) == 0 and f(p, 8, k, 0, 8, 0, 1, None) == 0                   # nothing to do: no launch


# ----------------------------------------------------------------------------- the kernel on the SIMT emulator
@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


KEYS = [(0, 0, 0), (12345, 2, 1), (2 ** 63 + 7, 8, 3)]


@pytest.mark.parametrize("n", [1, 5, 4101])
@pytest.mark.parametrize("col0", [0, 3])
def test_rng_fill_on_the_emulator(emu, n, col0):
    """Three rows (seeds 0, 12345, 2^63 + 7), ld_out = n + 3: uniforms bit-equal to the restatement, normals within 1e-5 of its float64 evaluation, padding untouched."""
    from chatterbox_amd import ops
    keys = R.key_tensor(KEYS)
    for normal in (False, True):
        out = torch.full((3, n + 3), float("nan"))
        ops.rng_fill(out, keys, n=n, col0=col0, normal=normal)
        assert out[:, n:].isnan().all(), "columns [n, ld_out) must not be written"
        got, want = out[:, :n].double().numpy(), R.fill(KEYS, col0, n, normal)
        err = float(np.abs(got - want).max())
        print(f"n={n} col0={col0} {'normal' if normal else 'uniform'}: max |err| {err:.3e}")
        if normal:
            assert np.isfinite(got).all() and err <= TOL_NORMAL
        else:
            assert np.array_equal(got, want)


def test_seeded_draw_helpers_on_the_emulator(emu):
    """ops.seeded_z / seeded_phase / seeded_noise: the stream ids, the z layout (column = frame * 80 + channel), the phase scaling and its zeroed entry, one
    substream per harmonic -- and a later window of z / noise equals the same window of the full fill."""
    import math
    from chatterbox_amd import ops
    seeds = [3, 2 ** 40 + 1]
    z = ops.seeded_z(seeds, 6, CPU)
    assert z.shape == (2, 6, 80) and np.abs(z.view(2, -1).double().numpy() - R.fill([(s, 0, 1) for s in seeds], 0, 480, True)).max() <= TOL_NORMAL
    assert torch.equal(ops.seeded_z(seeds, 2, CPU, frame0=3), z[:, 3:5])
    ph = ops.seeded_phase(seeds, CPU)
    u = torch.from_numpy(R.fill([(s, 0, 2) for s in seeds], 0, 9, False)).float()
    want = (u * 2 - 1) * math.pi
    want[:, 0] = 0
    assert ph.shape == (2, 9) and torch.equal(ph, want) and float(ph.abs().max()) <= math.pi
    nz = ops.seeded_noise(seeds, 50, CPU)
    assert nz.shape == (2, 9, 50) and np.abs(nz.view(18, 50).double().numpy() - R.fill([(s, h, 3) for s in seeds for h in range(9)], 0, 50, True)).max() <= TOL_NORMAL
    assert torch.equal(ops.seeded_noise(seeds, 13, CPU, col0=21), nz[:, :, 21:34])


# ----------------------------------------------------------------------------- the public classes over a recording engine (nothing is launched)
class _FakeT3:
    MAX_BATCH = 4


class _FakeSerialEngine:
    dev = CPU

    def __init__(self):
        self.t3, self.calls = _FakeT3(), []

    def synthesize(self, text_tokens, t3_conds, gen_ref, **kw):
        self.calls.append(("synthesize", dict(text_tokens=text_tokens, **kw)))
        return [torch.full((3,), float(t.numel())) for t in text_tokens], None


class _FakeEngine(_FakeSerialEngine):
    def synthesize_pipelined(self, jobs, **kw):
        self.calls.append(("pipelined", dict(jobs=jobs, **kw)))
        for job in jobs:
            yield [torch.full((3,), float(t.numel())) for t in job["text_tokens"]], None, 0.0


class _Tok:
    def text_to_tokens(self, text, language_id=None):
        return torch.arange(len(text), dtype=torch.int32).unsqueeze(0)

    def __call__(self, text, **kw):
        return type("E", (), {"input_ids": torch.arange(len(text)).unsqueeze(0)})()


def _tts(cls, engine):
    from chatterbox_amd import api, synth
    m = cls.__new__(cls)
    m.engine, m.tokenizer, m.device, m.analyzer, m.watermarker, m.model_label = engine, _Tok(), CPU, None, None, "Turbo"
    m.conds = api.Conditionals(api.T3Cond(**synth.t3_cond()), synth.s3gen_ref(n_prompt_tokens=8))
    return m


def _sub_batches(calls):
    """[(text lengths, seeds), ...] of the sub-batches the engine was given, in execution order"""
    jobs = [j for kind, kw in calls for j in (kw["jobs"] if kind == "pipelined" else [kw])]
    return [([int(t.numel()) for t in j["text_tokens"]], j.get("seeds")) for j in jobs]


LENS = [9, 2, 5, 7, 30]   # characters; the texts end in punctuation, so the normalisers add nothing
SEEDS = [101, 2 ** 64 - 1, 0, 104, 2 ** 33]


@pytest.mark.parametrize("cls_name,extra", [("ChatterboxTTS", 2), ("ChatterboxMultilingualTTS", 2), ("ChatterboxTurboTTS", 0)])
@pytest.mark.parametrize("max_batch", [None, 2])
def test_seeds_follow_their_requests_through_the_batch_plan(cls_name, extra, max_batch):
    from chatterbox_amd import api
    eng = _FakeEngine() if cls_name != "ChatterboxTurboTTS" else _FakeSerialEngine()
    m = _tts(getattr(api, cls_name), eng)
    m.max_batch = max_batch
    texts = ["x" * (n - 1) + "." for n in LENS]
    args = (texts, "en") if cls_name == "ChatterboxMultilingualTTS" else (texts,)
    out = m.generate_batch(*args, seeds=SEEDS)
    assert [int(w[0, 0]) for w in out] == [n + extra for n in LENS], "waveforms come back in the caller's order"
    subs = _sub_batches(eng.calls)
    assert [len(s[0]) for s in subs] == ([4, 1] if max_batch is None else [2, 2, 1])
    seed_of_len = {n + extra: s for n, s in zip(LENS, SEEDS)}
    for lens, seeds in subs:
        assert seeds == [seed_of_len[n] for n in lens], "a sub-batch carries the seeds of ITS requests, in its row order"
    eng.calls.clear()
    m.generate_batch(*args, seeds=77)   # an int: the same seed for every request
    assert [s for _, s in _sub_batches(eng.calls)] == [[77] * len(l) for l, _ in _sub_batches(eng.calls)]
    eng.calls.clear()
    m.generate_batch(*args)             # no seeds: the jobs are exactly the unseeded ones
    assert all(s is None for _, s in _sub_batches(eng.calls)) and all("seeds" not in kw for kind, kw in eng.calls if kind == "synthesize")


@pytest.mark.parametrize("cls_name", ["ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS"])
def test_seed_arguments_are_validated_before_the_engine_is_called(cls_name):
    from chatterbox_amd import api
    eng = _FakeEngine()
    m = _tts(getattr(api, cls_name), eng)
    texts = ["aaaa.", "bb.", "cccccc."]
    lang = ("en",) if cls_name == "ChatterboxMultilingualTTS" else ()
    for bad, err in (([1, 2], ValueError), ([1, 2, 3, 4], ValueError), ([1, -2, 3], ValueError), ([1, 2, 2 ** 64], ValueError), ([1, 2.5, 3], TypeError),
                     ("12", TypeError), (1.0, TypeError), (torch.tensor([1, 2, 3]), TypeError), (-5, ValueError)):
        with pytest.raises(err, match="seeds"):
            m.generate_batch(texts, *lang, seeds=bad)
    with pytest.raises(ValueError, match="generator"):
        m.generate_batch(texts, *lang, seeds=[1, 2, 3], generator=torch.Generator())
    for bad, err in ((-1, ValueError), (2 ** 64, ValueError), (1.0, TypeError), ([3], TypeError), (True, TypeError)):
        with pytest.raises(err, match="seed"):
            m.generate("aaaa.", *lang, seed=bad)
        with pytest.raises(err, match="seed"):
            m.generate_stream("aaaa.", *lang, seed=bad)
    assert eng.calls == []
    m.generate("aaaa.", *lang, seed=2 ** 64 - 1)
    assert eng.calls[-1][0] == "synthesize" and eng.calls[-1][1]["seeds"] == [2 ** 64 - 1]
    m.generate("aaaa.", *lang)
    assert "seeds" not in eng.calls[-1][1], "without a seed the engine call is exactly the unseeded one"


def test_vc_seeds_follow_their_requests_and_are_validated():
    from chatterbox_amd import api, synth

    class Voc:
        def __init__(self):
            self.calls = []

        def vocode(self, toks, refs, **kw):
            self.calls.append(([int(t.numel()) for t in toks], kw))
            return [torch.full((2,), float(t.numel())) for t in toks], None

    vc = api.ChatterboxVC.__new__(api.ChatterboxVC)
    vc.engine, vc.device, vc.ref_dict, vc.analyzer, vc.watermarker = Voc(), CPU, synth.s3gen_ref(n_prompt_tokens=8), None, None
    vc.MAX_BATCH = 2
    toks = [synth.speech_tokens(n) for n in (30, 10, 20)]
    for bad, err in (([1, 2], ValueError), ([1, 2, -3], ValueError), ([1, 2, "3"], TypeError), (2 ** 64, ValueError)):
        with pytest.raises(err, match="seeds"):
            vc.generate_batch(s3_tokens=toks, seeds=bad)
    with pytest.raises(TypeError, match="seed"):
        vc.generate(s3_tokens=toks[0], seed=1.5)
    with pytest.raises(ValueError, match="seed"):
        vc.generate_stream(s3_tokens=toks[0], seed=-1)
    assert vc.engine.calls == []
    out = vc.generate_batch(s3_tokens=toks, seeds=[7, 8, 9])
    assert [int(w[0, 0]) for w in out] == [30, 10, 20]
    assert [(l, kw.get("seeds")) for l, kw in vc.engine.calls] == [([10, 20], [8, 9]), ([30], [7])]
    vc.engine.calls.clear()
    vc.generate(s3_tokens=toks[1], seed=8)
    vc.generate(s3_tokens=toks[1])
    assert vc.engine.calls[0][1] == dict(seeds=[8]) and vc.engine.calls[1][1] == {}
