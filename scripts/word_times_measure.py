"""Word timestamps on the bench shape (8 utterances x 250 speech tokens = 10 s each, 64 text tokens, synthetic 30-layer weights), one process on one box, the
variants ALTERNATING inside every repetition.

    python scripts/word_times_measure.py engine [variants, default i,ii] [repetitions, default 5]
        ChatterboxEngine.synthesize of the batch, wall seconds around a synchronise, with the engine's own last_timing:
          i    the call without words (uses nothing newer than synthesize, so it also runs from a checkout of the parent commit: `... engine i`)
          ii   words=dict(heads=None): the alignment pass (T3Engine.align, the default ALIGN_HEADS) between T3 and the vocoder; reports align_s, its share of the
               same request's t3_s, and the device time of the pass's own two kernels (events around every ops.attn_text_mass / ops.align_path call)
    python scripts/word_times_measure.py api [variants, default i,ii,iii] [repetitions, default 5]
        ChatterboxMultilingualTTS.generate_batch of 8 requests through the public API, copies to the host included:
          i    without the argument (`... api i` runs from the parent commit)   ii   word_times=False   iii  word_times=True
Prints one JSON line."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, ops, synth  # noqa: E402

dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "engine"
variants = (sys.argv[2] if len(sys.argv) > 2 else ("i,ii" if mode == "engine" else "i,ii,iii")).split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B, N, TEXT = 8, 250, 64


class Tok:
    """stand-in tokenizer of the synthetic model: ids from the characters, pieces() = the characters"""
    SPACE = "[SPACE]"

    def __init__(self):
        self.seen = {}

    def text_to_tokens(self, text, language_id=None):
        ids = torch.tensor([(7 * ord(c) + 3 * i) % 2000 + 300 for i, c in enumerate(text)], dtype=torch.int32)
        self.seen[tuple(ids.tolist())] = [self.SPACE if c == " " else c for c in text]
        return ids.unsqueeze(0)

    def pieces(self, ids):
        return ["[START]"] + self.seen[tuple(ids[1:-1])] + ["[STOP]"]


def timed(run, extra=None):
    for v in variants:
        run(v)
    secs, more = {v: [] for v in variants}, {v: [] for v in variants}
    for _ in range(reps):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(v)
            torch.cuda.synchronize()
            secs[v].append(round(time.perf_counter() - t0, 4))
            if extra is not None:
                more[v].append(extra(v))
    out = dict(mode=mode, variants=variants, seconds=secs, median_s={v: round(statistics.median(t), 4) for v, t in secs.items()},
               spread_s={v: round(max(t) - min(t), 4) for v, t in secs.items()}, gpu=torch.cuda.get_device_name(0))
    if extra is not None:
        out["per_call"] = more
    return out


m = api.ChatterboxMultilingualTTS.from_synthetic(dev, t3_layers=30)
m.watermarker, m.tokenizer = None, Tok()
eng = m.engine
if mode == "engine":
    texts = [synth.text_tokens(TEXT, seed=b) for b in range(B)]
    t3c, gen = m.conds.t3.as_dict(), m.conds.gen
    events = []
    if "ii" in variants:
        def watched(fn, name):
            def call(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn(*a, **kw)
                e1.record()
                events.append((name, e0, e1))
                return r
            return call
        ops.attn_text_mass, ops.align_path = watched(ops.attn_text_mass, "attn_text_mass"), watched(ops.align_path, "align_path")

    def run(v):
        events.clear()
        eng.synthesize(texts, t3c, gen, max_new_tokens=N, ban_eos=True, ban_from=6561, seeds=list(range(B)), drop_last_token=True,
                       **({} if v == "i" else dict(words=dict(heads=None))))

    def extra(v):
        t = dict(eng.last_timing)
        rec = dict(t3_s=round(t["t3_s"], 4), total_s=round(t["total_s"], 4))
        if "align_s" in t:
            per = {}
            for name, e0, e1 in events:
                per.setdefault(name, []).append(round(e0.elapsed_time(e1) * 1e3, 1))
            rec.update(align_s=round(t["align_s"], 4), align_share_of_t3=round(t["align_s"] / t["t3_s"], 4), kernel_us_between_events=per)
        return rec
    res = timed(run, extra)
else:
    texts = [("Word times for request %d of the batch, a sentence of some length. " % b) * 1 for b in range(B)]
    syn = eng.synthesize
    eng.synthesize = lambda *a, **kw: syn(*a, **{**kw, "max_new_tokens": N, "ban_eos": True})
    pip = eng.synthesize_pipelined
    eng.synthesize_pipelined = lambda jobs, **kw: pip(jobs, **{**kw, "max_new_tokens": N, "ban_eos": True})
    kw = lambda v: {} if v == "i" else dict(word_times=(v == "iii"))
    res = timed(lambda v: m.generate_batch(texts, "en", seeds=list(range(B)), **kw(v)))
print(json.dumps(res), flush=True)
