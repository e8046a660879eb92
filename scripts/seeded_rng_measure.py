"""What per-request seeds cost on one MI355X, one process:

  fill    ops.rng_fill (cbx_rng_fill_f32) against torch.rand / torch.randn on the three shapes it replaces at the benchmark batch (B = 8, 250 prompt tokens, 250
          sampled tokens): the (8, 1000) sampling uniforms, the (8, 1000, 80) CFM noise, the (8, 9, 240000) vocoder source noise.  Interleaved in one process,
          HIP events around each call, median of `reps` after a warm-up; achieved store bandwidth from the bytes written.
  stream  time to the first audio of engine.synthesize_stream with a 1000-token budget and window=200 at B = 1: unseeded (z and the 34.6 MB of source noise of
          the whole budget are drawn before the first round) against seeded (a round fills what it reads), interleaved, median of 5 after a warm-up.

    python scripts/seeded_rng_measure.py [fill] [stream]        (default: both; one JSON line per row)"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import ops, synth  # noqa: E402

dev = torch.device("cuda", 0)
what = set(sys.argv[1:]) or {"fill", "stream"}
say = lambda **kw: print(json.dumps(kw), flush=True)


def event_ms(fn, reps=30, warm=5):
    ts = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1))
    return ts


if "fill" in what:
    B, P, N = 8, 250, 250
    seeds = list(range(100, 100 + B))
    shapes = (("t3 uniforms", (B, 1000), False, ops.rng_keys(seeds, ops.RNG_T3_UNIFORMS, device=dev)),
              ("cfm z", (B, 2 * (P + N) * 80), True, ops.rng_keys(seeds, ops.RNG_CFM_Z, device=dev)),
              ("vocoder noise", (B * 9, 480 * 2 * N), True, ops.rng_keys(seeds, ops.RNG_VOC_NOISE, substreams=range(9), device=dev)))
    for name, shape, normal, keys in shapes:
        out = torch.empty(shape, device=dev)
        ours, theirs = [], []
        for _ in range(3):  # interleave the two in blocks
            ours += event_ms(lambda: ops.rng_fill(out, keys, normal=normal), reps=10)
            theirs += event_ms((lambda: out.normal_()) if normal else (lambda: out.uniform_()), reps=10)
        mb = out.numel() * 4 / 1e6
        mo, mt = statistics.median(ours), statistics.median(theirs)
        say(part="fill", shape=name, rows=shape[0], n=shape[1], normal=normal, MB=round(mb, 2), rng_fill_us=round(1e3 * mo, 1), torch_us=round(1e3 * mt, 1),
            rng_fill_GBps=round(mb / mo, 1), torch_GBps=round(mb / mt, 1), rng_fill_min_us=round(1e3 * min(ours), 1), torch_min_us=round(1e3 * min(theirs), 1))

if "stream" in what:
    from chatterbox_amd.engine import ChatterboxEngine
    L, N = 30, 1000
    eng = ChatterboxEngine(synth.t3_state_dict(L, 0), synth.s3gen_state_dict(0), dev, n_t3_layers=L)
    t3c, gen = synth.t3_cond(prompt_len=150), synth.s3gen_ref()
    texts = [synth.text_tokens(64, seed=0)]

    def first_audio(seeded, rep):
        kw = dict(seeds=[1000 + rep]) if seeded else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = eng.synthesize_stream(texts, t3c, gen, max_new_tokens=N, ban_eos=True, ban_from=6561, window=200, **kw)
        next(it)
        f = time.perf_counter() - t0
        it.close()
        torch.cuda.synchronize()
        return f

    res = {False: [], True: []}
    for rep in range(6):
        for seeded in (False, True):
            f = first_audio(seeded, rep)
            if rep:
                res[seeded].append(f)
    say(part="stream", budget_tokens=N, window=200, B=1, first_audio_ms_unseeded=round(1e3 * statistics.median(res[False]), 1),
        first_audio_ms_seeded=round(1e3 * statistics.median(res[True]), 1), runs_unseeded=[round(1e3 * x, 1) for x in res[False]],
        runs_seeded=[round(1e3 * x, 1) for x in res[True]])
