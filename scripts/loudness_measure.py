"""Loudness normalisation on the configs[2] shape, one process on one box: eight requests (Multilingual, synthetic 30-layer weights, 64 text tokens, 250 sampled
tokens = 10 s each, 3 voices) through generate_batch, the variants ALTERNATING inside every repetition:
  i    the default call (uses nothing newer than generate_batch, so it also runs from a checkout of the parent commit: `... i`)
  ii   loudness=-16
  iii  loudness=-16, sample_rate=8000, encoding="mulaw" (the meter and the gain in front of the format launch)
Prints one JSON line: wall seconds per variant and repetition.

    python scripts/loudness_measure.py [variants, default i,ii,iii] [repetitions, default 5]
    python scripts/loudness_measure.py kernel [rows8x240000 | rows1x960000]   # the meter and the gain alone on 8 x 240 000 and / or 1 x 960 000 samples (device
                                                   # events and the host's time to enqueue here; run it under rocprofv3 --kernel-trace for the launches' own times)
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, synth  # noqa: E402

dev = torch.device("cuda:0")
CALLS = dict(i={}, ii=dict(loudness=-16), iii=dict(loudness=-16, sample_rate=8000, encoding="mulaw"))


def kernel_only(reps=20):
    from chatterbox_amd import ops
    out = {}
    shapes = dict(rows8x240000=(8, 240000), rows1x960000=(1, 960000))
    for name, (R, n) in shapes.items():
        if len(sys.argv) > 2 and sys.argv[2] != name:
            continue
        wav = torch.rand(R, n, device=dev) * 0.2 - 0.1
        rows = [wav[b] for b in range(R)]
        res = {}
        for what, fn in (("meter", lambda: ops.wave_loudness(rows, [-16.0] * R)), ("gain", lambda: ops.wave_gain(rows, one)), ("both", lambda: ops.wave_normalize(rows, [None] * R))):
            one = torch.ones(R, device=dev)
            fn()
            torch.cuda.synchronize()
            us, host_us = [], []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                fn()
                host_us.append((time.perf_counter() - t0) * 1e6)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            res[what] = dict(median_us_between_events=round(statistics.median(us), 1), median_host_us_to_enqueue=round(statistics.median(host_us), 1))
        stats, _ = ops.wave_loudness(rows, [-16.0] * R)
        res["L_of_row_0"] = round(float(stats[0, 0]), 4)
        out[name] = res
    print(json.dumps(dict(kernel_only=out, gpu=torch.cuda.get_device_name(0))), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "kernel":
    kernel_only()
    sys.exit(0)

variants = (sys.argv[1] if len(sys.argv) > 1 else "i,ii,iii").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
m = api.ChatterboxMultilingualTTS.from_synthetic(dev, t3_layers=30)


class Tok:
    def text_to_tokens(self, text, language_id=None):
        return synth.text_tokens(62, seed=len(text)).int().unsqueeze(0)   # + SOT / EOT = 64 text tokens


m.tokenizer = Tok()
gen = m.engine.t3.generate
m.engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **dict(kw, max_new_tokens=250, ban_eos=True))
voices = [api.Conditionals(api.T3Cond(**synth.t3_cond(seed=s)), synth.s3gen_ref(seed=s)) for s in (11, 12, 13)]
conds = [voices[k % 3] for k in range(8)]
texts = ["x" * (10 + k) + "." for k in range(8)]
run = lambda v: m.generate_batch(texts, "en", conds=conds, **CALLS[v])

for v in variants:
    run(v)
secs = {v: [] for v in variants}
for _ in range(reps):
    for v in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(v)
        torch.cuda.synchronize()
        secs[v].append(round(time.perf_counter() - t0, 4))
extra = {}
if "ii" in variants:
    st = m.engine.last_loudness.cpu()
    extra = dict(last_loudness_L=[round(float(v), 3) for v in st[:, 0]], last_loudness_gain=[round(float(v), 4) for v in st[:, 2]])
print(json.dumps(dict(variants=variants, seconds=secs, median_s={v: round(statistics.median(t), 4) for v, t in secs.items()},
                      spread_s={v: round(max(t) - min(t), 4) for v, t in secs.items()}, gpu=torch.cuda.get_device_name(0), **extra)), flush=True)
