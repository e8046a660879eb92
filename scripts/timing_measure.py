"""Timing control on the bench shape (B = 8 utterances of 250 tokens, 10 s), one process on one box, the variants ALTERNATING inside every repetition.

    python scripts/timing_measure.py launch [repetitions, default 200]
        ops.mel_time_warp beside ops.mel_time_scale on the same (8, 500, 80) mel at rate 0.8 (625 output frames per row), us between device events around one call
        from Python and the host's time to enqueue it: `scale` the launch of the parent commit, `warp1` the one-segment table (0, 0.0, 0.8), which computes the
        same bits, `warp100` a 100-segment table of the same total length whose rates alternate around 0.8.  Warm-up 20 calls each; median, and the spread as the
        5th .. 95th percentile.  Run it under rocprofv3 --kernel-trace --stats for the kernels' own time.
    python scripts/timing_measure.py duration [repetitions, default 7]
        ChatterboxVC.generate of one 250-token source (10 s) through the public API, copy to the host included: `plain`, `speed` = 0.8 and `duration` = 12.5 s
        (the same rate, so the same stretch through the other kernel)
    python scripts/timing_measure.py timing [repetitions, default 5]
        ChatterboxEngine.synthesize of B = 8 utterances with a 250-token budget (EOS banned) on synthetic full-depth weights: `words` the call with the alignment
        pass (what generate(word_times=True) runs), `timing` the same with every text token's start moved to 1.25 times its natural frame (what generate(timing=)
        adds: the plan on the host and the warp launch)
Prints one JSON line; appends it to profiles/timing_measure.log."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import api, ops, synth  # noqa: E402

dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "launch"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else dict(launch=200, duration=7, timing=5)[mode]


def spread(v):
    v = sorted(v)
    return [round(v[int(0.05 * (len(v) - 1))], 2), round(v[int(0.95 * (len(v) - 1) + 0.5)], 2)]


def emit(res):
    line = json.dumps(dict(res, mode=mode, gpu=torch.cuda.get_device_name(0)))
    print(line, flush=True)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "timing_measure.log"), "a") as f:
        f.write(line + "\n")


def launch():
    B, M, s = 8, 500, 0.8
    O = ops.scaled_len(M, s)
    mel = (torch.randn(B, M, 80, device=dev) * 3 - 5).contiguous()
    out = torch.empty(B, O, 80, device=dev)
    anchors = [(5 * k, int(5 * k / s + 0.5) + (k % 2)) for k in range(1, 100)]  # 100 segments of 5 input frames, 6 or 7 output frames in turn
    plan = ops.warp_plan(M, anchors, end=O)
    assert len(plan["table"]) == 100 and plan["frames"] == O and not plan["clamped"]
    fns = dict(scale=lambda: ops.mel_time_scale(mel, [s] * B, in_lens=[M] * B, out=out),
               warp1=lambda: ops.mel_time_warp(mel, [[(0, 0.0, s)]] * B, in_lens=[M] * B, out=out, out_lens=[O] * B),
               warp100=lambda: ops.mel_time_warp(mel, [plan["table"]] * B, in_lens=[M] * B, out=out, out_lens=[O] * B))
    a = ops.mel_time_scale(mel, [s] * B, in_lens=[M] * B)[0]
    b = ops.mel_time_warp(mel, [[(0, 0.0, s)]] * B, in_lens=[M] * B, out_lens=[O] * B)[0]
    assert torch.equal(a, b), "the one-segment table computes the stretch's bits"
    for fn in fns.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    us, host = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            host[k].append((time.perf_counter() - t0) * 1e6)
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    emit(dict(shape=[B, M, 80], out_frames=O, repetitions=reps, bytes_moved=B * (M + O) * 80 * 4,
              us_between_events={k: dict(median=round(statistics.median(v), 2), p5_p95=spread(v)) for k, v in us.items()},
              host_us_to_enqueue={k: dict(median=round(statistics.median(v), 2), p5_p95=spread(v)) for k, v in host.items()}))


def timed(variants, run):
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
    return dict(variants=variants, repetitions=reps, seconds=secs, median_s={v: round(statistics.median(t), 4) for v, t in secs.items()},
                spread_s={v: round(max(t) - min(t), 4) for v, t in secs.items()})


if mode == "launch":
    launch()
elif mode == "duration":
    m = api.ChatterboxVC.from_synthetic(dev, tokenizer_layers=1)
    m.watermarker = None
    src = synth.speech_tokens(250, seed=0)
    kw = dict(plain={}, speed=dict(speed=0.8), duration=dict(duration=12.5))
    res = timed(list(kw), lambda v: m.generate(s3_tokens=src, seed=7, **kw[v]))
    assert m.generate(s3_tokens=src, seed=7, duration=12.5).shape == m.generate(s3_tokens=src, seed=7, speed=0.8).shape
    emit(res)
else:
    m = api.ChatterboxTTS.from_synthetic(dev)
    eng = m.engine
    text = [torch.cat([torch.tensor([255]), torch.randint(1, 600, (40,), generator=torch.Generator().manual_seed(k)), torch.tensor([0])]) for k in range(8)]
    base = dict(max_new_tokens=250, ban_eos=True, seeds=list(range(8)), drop_last_token=False, words=dict(heads=None))
    _, _, al = eng.synthesize(text, m.conds.t3.as_dict(), m.conds.gen, **base)
    starts = []
    for a in al:  # every text token's start moved to 1.25 times its natural mel frame (nondecreasing; a start at frame 0 stays)
        starts.append(dict(starts=[None if f0 == 0 else int(1.25 * 2 * f0 + 0.5) for f0, _ in a["frames"]], end=int(1.25 * 2 * a["n_frames"] + 0.5)))
    kw = dict(words={}, timing=dict(warp=starts))
    res = timed(list(kw), lambda v: eng.synthesize(text, m.conds.t3.as_dict(), m.conds.gen, **base, **kw[v]))
    res["segments"] = [len(f["table"]) for f in eng.last_fit]
    res["clamped"] = [len(f["clamped"]) for f in eng.last_fit]
    emit(res)
