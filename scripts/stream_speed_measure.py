"""What `speed=` costs a windowed streaming round on one MI355X, one process: ChatterboxEngine.vocode_stream on the T3-less engine ChatterboxVC builds (full-depth
S3Gen, 10 CFM steps, synthetic voice), 1000 source tokens, window=200, default schedule, B = 1 and B = 8, with speed None and 1.25.

  round   wall time of every round (the generator's next(), which ends in the round's D2H copy), streams at the two speeds ALTERNATED, `reps` of each after one
          warm-up of each; reported: the median over the steady rounds (the window has slid: tokens per round constant) of the per-round medians over the reps.
          speed=None is the stream of the parent commit launch for launch.  At 1.25 a steady round vocodes fewer frames, so the figure is the cost of the whole
          round at that rate, not of the stretch launch alone.
  launch  ops.mel_time_scale_window alone on a steady round's window (B, 508, 80), HIP events around each call (the wrapper's H2D copy included).

    python scripts/stream_speed_measure.py [round] [launch]        (default: both; one JSON line per row)"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import ops, synth  # noqa: E402
from chatterbox_amd.api import ChatterboxVC  # noqa: E402
from chatterbox_amd.engine import stream_speed_schedule  # noqa: E402

dev = torch.device("cuda", 0)
what = set(sys.argv[1:]) or {"round", "launch"}
say = lambda **kw: print(json.dumps(kw), flush=True)
N, W, REPS, SPEEDS = 1000, 200, 3, (None, 1.25)

if "round" in what:
    eng = ChatterboxVC._engine(synth.s3gen_state_dict(0), dev)
    gen = synth.s3gen_ref()
    for B in (1, 8):
        toks = [synth.speech_tokens(N, seed=k) for k in range(B)]
        times = {s: [] for s in SPEEDS}
        for rep in range(REPS + 1):
            for s in SPEEDS:
                per, it = [], eng.vocode_stream(toks, gen, window=W, **({} if s is None else dict(speed=s)))
                while True:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if next(it, None) is None:
                        break
                    per.append(time.perf_counter() - t0)
                if rep:
                    times[s].append(per)
        for s in SPEEDS:
            sched = stream_speed_schedule(N, s, window=W)
            n_tok = [n - a for a, n, _, _ in sched]
            steady = [r for r in range(1, len(sched) - 1) if sched[r][0] > 0 and n_tok[r] == max(n_tok)]
            med = [statistics.median(run[r] for run in times[s]) for r in range(len(sched))]
            say(part="round", B=B, tokens=N, window=W, speed=s, rounds=len(sched), tokens_per_steady_round=max(n_tok), steady_rounds=len(steady),
                steady_round_ms=round(1e3 * statistics.median(med[r] for r in steady), 2), steady_round_min_ms=round(1e3 * min(min(run[r] for run in times[s]) for r in steady), 2),
                steady_round_max_ms=round(1e3 * max(max(run[r] for run in times[s]) for r in steady), 2), first_round_ms=round(1e3 * med[0], 2),
                stream_ms=round(1e3 * statistics.median(sum(run) for run in times[s]), 1))

if "launch" in what:
    for B in (1, 8):
        mel = torch.randn(B, 508, 80, device=dev) * 3 - 5
        ts = []
        for i in range(35):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, _ = ops.mel_time_scale_window(mel, 1.25, 641, 800, [502] * B, [400] * B)
            e1.record()
            e1.synchronize()
            if i >= 5:
                ts.append(e0.elapsed_time(e1))
        say(part="launch", B=B, frames_in=502, frames_out=400, median_us=round(1e3 * statistics.median(ts), 1), min_us=round(1e3 * min(ts), 1))
