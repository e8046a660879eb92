"""Long-form streaming, one process on one box: a synthetic Multilingual model (30-layer T3), a text of 24 chunks, every chunk 64 text tokens and 250 sampled
tokens (10 s; the budget is spent, EOS banned).  The variants ALTERNATE inside every repetition:
  a  generate_long: total
  b  generate_long_stream(first_batch=None) -- the same jobs as a: time to the first piece, total
  c  generate_long_stream() with the default ramp (first_batch=1, batch_growth=2.0): time to the first piece, total
  d  c with loudness=-16, sample_rate=16000, encoding="s16": time to the first piece, total, pieces
  g  generate() of the first chunk alone (what the first piece of c has to wait for at the least)
Prints one JSON line: wall seconds per variant and repetition, medians and spreads (max - min).

    python scripts/long_stream_measure.py [repetitions, default 5] [chunks, default 24] [max_batch, default 8: the benchmark's device batch; 0: the T3 engine's 32]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, synth  # noqa: E402

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 24
m = api.ChatterboxMultilingualTTS.from_synthetic(dev, t3_layers=30)
m.max_batch = (int(sys.argv[3]) if len(sys.argv) > 3 else 8) or None


class Tok:
    def text_to_tokens(self, text, language_id=None):
        return synth.text_tokens(62, seed=len(text)).int().unsqueeze(0)   # + SOT / EOT = 64 text tokens


m.tokenizer = Tok()
gen = m.engine.t3.generate
m.engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **dict(kw, max_new_tokens=250, ban_eos=True))
sentences = ["Sentence number %02d%s." % (k, " x" * (k % 7)) for k in range(n_chunks)]
TEXT, KW = " ".join(sentences), dict(max_chars=max(len(s) for s in sentences), seed=7)
LOUD = dict(loudness=-16, sample_rate=16000, encoding="s16")
LAST = []   # engine.last_loudness of the last d run: L, peak, gain, blocks used


def whole():
    t0 = time.perf_counter()
    wav = m.generate_long(TEXT, "en", **KW)
    torch.cuda.synchronize()
    return dict(total=time.perf_counter() - t0, samples=wav.shape[1])


def plan_sizes(**ramp):
    a = api._long_args(KW["max_chars"], 0.15, 0.4, 40.0, 2, 240, 7, 1.0, False)
    return [len(j["chunks"]) for j in api.long_stream_plan(api.split_text(TEXT, KW["max_chars"]), int(m.max_batch or m.engine.t3.MAX_BATCH), a, **ramp)]


def stream(**kw):
    t0 = time.perf_counter()
    first, n, pieces = None, 0, 0
    for w in m.generate_long_stream(TEXT, "en", **KW, **kw):
        first = first if first is not None else time.perf_counter() - t0
        n, pieces = n + w.shape[1], pieces + 1
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    if "loudness" in kw:
        LAST[:] = [round(float(v), 4) for v in m.engine.last_loudness.cpu().view(-1)]
    return dict(first=first, total=total, samples=n, pieces=pieces)


def one():
    t0 = time.perf_counter()
    wav = m.generate(sentences[0], "en", seed=7)
    return dict(total=time.perf_counter() - t0, samples=wav.shape[1])


RUN = dict(a=whole, b=lambda: stream(first_batch=None), c=stream, d=lambda: stream(**LOUD), g=one)
for v in RUN:
    RUN[v]()
res = {v: [] for v in RUN}
for _ in range(reps):
    for v in RUN:
        torch.cuda.synchronize()
        res[v].append(RUN[v]())
out = dict(gpu=torch.cuda.get_device_name(0), chunks=n_chunks, max_batch=int(m.max_batch or m.engine.t3.MAX_BATCH), repetitions=reps,
           batches_a_b=plan_sizes(first_batch=None), batches_c_d=plan_sizes())
for v, rows in res.items():
    for key in ("first", "total"):
        if key in rows[0]:
            t = [round(r[key], 4) for r in rows]
            out[f"{v}_{key}_s"] = dict(all=t, median=round(statistics.median(t), 4), spread=round(max(t) - min(t), 4))
    out[f"{v}_samples"] = rows[-1]["samples"]
    if "pieces" in rows[-1]:
        out[f"{v}_pieces"] = rows[-1]["pieces"]
out["d_minus_c_total_per_piece_ms"] = round(1e3 * (out["d_total_s"]["median"] - out["c_total_s"]["median"]) / max(1, out["d_pieces"]), 3)
out["last_loudness"] = LAST
print(json.dumps(out), flush=True)
