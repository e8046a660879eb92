"""Pitch control on the bench shape, one process on one box, the variants ALTERNATING inside every repetition.

    python scripts/pitch_measure.py vocode [variants, default i,ii,iii] [repetitions, default 5]
        ChatterboxEngine.vocode of B = 8 utterances of 250 tokens (10 s) on synthetic full-depth S3Gen weights, wall seconds around a synchronise:
          i    the call without pitch (uses nothing newer than vocode, so it also runs from a checkout of the parent commit: `... vocode i`)
          ii   pitch=3: the mel stretched at 1 / r, the vocoder on it, the pitch launch
          iii  speed = 1 / r and no pitch: what ii does without its new launch
    python scripts/pitch_measure.py generate [variants, default i,ii,iii] [repetitions, default 5]
        ChatterboxVC.generate of one 250-token source (10 s) through the public API, copy to the host included; i / ii / iii as above (`... generate i` runs from the
        parent commit)
    python scripts/pitch_measure.py kernel
        ops.wave_pitch alone on the 8 source rows a 10 s request has at p = +3, -3, +12 and -12 semitones (us between device events around one call from Python, and
        the host's time to enqueue it); run it under rocprofv3 --kernel-trace --stats for the launch's own time
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
PITCH = 3.0


def kernel_only(reps=20):
    out = {}
    K = 500  # frames of a 10 s request
    for p in (3.0, -3.0, 12.0, -12.0):
        r = ops.pitch_ratio(p)
        n_src, N = 480 * ops.scaled_len(K, 1.0 / r), 480 * K
        wav = torch.rand(8, n_src, device=dev) * 0.2 - 0.1
        rows = [wav[b] for b in range(8)]
        fn = lambda: ops.wave_pitch(rows, [r] * 8, [N] * 8)
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
        out[f"p{p:+g}"] = dict(step=round(r, 6), source_samples=n_src, outputs=N, median_us_between_events=round(statistics.median(us), 1),
                               median_host_us_to_enqueue=round(statistics.median(host_us), 1))
    print(json.dumps(dict(kernel_only=out, rows=8, gpu=torch.cuda.get_device_name(0))), flush=True)


def timed(variants, reps, run):
    for v in variants:
        run(v)
    secs = {v: [] for v in variants}
    for _ in range(reps):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(v)
            torch.cuda.synchronize()
            secs[v].append(round(time.perf_counter() - t0, 4))
    return dict(mode=mode, variants=variants, seconds=secs, median_s={v: round(statistics.median(t), 4) for v, t in secs.items()},
                spread_s={v: round(max(t) - min(t), 4) for v, t in secs.items()}, gpu=torch.cuda.get_device_name(0))


if mode == "kernel":
    kernel_only()
    sys.exit(0)

variants = (sys.argv[2] if len(sys.argv) > 2 else "i,ii,iii").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
kw = lambda v: {} if v == "i" else dict(pitch=PITCH) if v == "ii" else dict(speed=1.0 / 2.0 ** (PITCH / 12.0))
m = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
m.watermarker = None
if mode == "vocode":
    toks = [synth.speech_tokens(250, seed=k) for k in range(8)]
    res = timed(variants, reps, lambda v: m.engine.vocode(toks, m.ref_dict, seeds=list(range(8)), **kw(v)))
else:
    src = synth.speech_tokens(250, seed=0)
    res = timed(variants, reps, lambda v: m.generate(s3_tokens=src, seed=7, **kw(v)))
print(json.dumps(res), flush=True)
