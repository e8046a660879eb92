"""Pause control on the bench shape, one process on one box, the variants ALTERNATING inside every repetition.

    python scripts/pauses_measure.py vocode [variants, default i,ii] [repetitions, default 5]
        ChatterboxEngine.vocode of B = 8 utterances of 250 tokens (10 s) on synthetic full-depth S3Gen weights, wall seconds around a synchronise:
          i    the call without pauses (uses nothing newer than vocode, so it also runs from a checkout of the parent commit: `... vocode i`)
          ii   pauses=dict(keep=[2] * 8, db=3): synthetic weights make no real pauses, so frames under half the loudest frame's power count as silent
    python scripts/pauses_measure.py pipelined [variants, default i,ii] [repetitions, default 3]
        synthesize_pipelined over 4 batches of 8 x 64 text tokens x 250 sampled tokens (Multilingual, synthetic 30-layer T3), seconds per batch; i / ii as above
    python scripts/pauses_measure.py kernel
        ops.wave_squeeze alone on 8 x 240 000 and 1 x 960 000 samples with a 25-frame pause every 100 frames (us between device events around one call from
        Python, and the host's time to enqueue it); run it under rocprofv3 --kernel-trace --stats for the three launches' own times
Prints one JSON line."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, ops, synth  # noqa: E402

dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "vocode"
PAUSES = dict(keep=[2] * 8, db=3.0)


def kernel_only(reps=20):
    out = {}
    for name, (R, n) in dict(rows8x240000=(8, 240000), rows1x960000=(1, 960000)).items():
        wav = torch.rand(R, n, device=dev) * 0.2 - 0.1
        fr = wav.view(R, n // 480, 480)
        for f0 in range(50, n // 480 - 30, 100):
            fr[:, f0: f0 + 25] *= 1e-4
        rows = [wav[b] for b in range(R)]
        res = {}
        for what, fn in (("squeeze", lambda: ops.wave_squeeze(rows, [15] * R)), ("edges_for_scale", lambda: ops.wave_edges(rows, 40.0))):
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
        res["stats_of_row_0"] = ops.wave_squeeze(rows, [15] * R)["stats"][0].tolist()
        out[name] = res
    print(json.dumps(dict(kernel_only=out, gpu=torch.cuda.get_device_name(0))), flush=True)


def timed(variants, reps, run, per=1):
    for v in variants:
        run(v)
    secs = {v: [] for v in variants}
    for _ in range(reps):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(v)
            torch.cuda.synchronize()
            secs[v].append(round((time.perf_counter() - t0) / per, 4))
    return dict(mode=mode, variants=variants, seconds=secs, median_s={v: round(statistics.median(t), 4) for v, t in secs.items()},
                spread_s={v: round(max(t) - min(t), 4) for v, t in secs.items()}, gpu=torch.cuda.get_device_name(0))


if mode == "kernel":
    kernel_only()
    sys.exit(0)

variants = (sys.argv[2] if len(sys.argv) > 2 else "i,ii").split(",")
kw = lambda v: {} if v == "i" else dict(pauses=PAUSES)
if mode == "vocode":
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    m = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
    toks = [synth.speech_tokens(250, seed=k) for k in range(8)]
    res = timed(variants, reps, lambda v: m.engine.vocode(toks, m.ref_dict, seeds=list(range(8)), **kw(v)))
    if "ii" in variants:
        res["last_pauses"] = m.engine.last_pauses.cpu().tolist()
else:
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    m = api.ChatterboxMultilingualTTS.from_synthetic(dev, t3_layers=30)
    n_jobs = 4
    jobs = lambda v: [dict(text_tokens=[synth.text_tokens(64, seed=8 * j + k) for k in range(8)], t3_conds=m.conds.t3.as_dict(), gen_ref=m.conds.gen,
                           seeds=[100 * j + k for k in range(8)], **kw(v)) for j in range(n_jobs)]
    res = timed(variants, reps, lambda v: list(m.engine.synthesize_pipelined(jobs(v), max_new_tokens=250, ban_eos=True)), per=n_jobs)
    if "ii" in variants:
        res["last_pauses"] = m.engine.last_pauses.cpu().tolist()
print(json.dumps(res), flush=True)
