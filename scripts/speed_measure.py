"""What `speed=` costs on one MI355X, one process: the serial ChatterboxEngine.vocode at the benchmark shape (B = 8 utterances of 250 speech tokens, the synthetic
voice of bench.py, full-depth S3Gen, 10 CFM steps) with speed in {None, 0.8, 1.25}.

  vocode  wall time of the call and its flow / vocoder stage times (engine.last_timing; the stretch launch is inside the vocoder's share), interleaved over the
          three speeds, median of `reps` after a warm-up.  speed=None is launch for launch the path of the parent commit; the vocoder's time at 0.8 / 1.25 follows
          the stretched mel's length (625 / 400 frames against 500).
  launch  ops.mel_time_scale alone on the (8, 500, 80) flow mel, HIP events around each call (the wrapper's three small H2D copies included), median and minimum.

Engine-level calls only, so the `vocode` part also runs from a checkout of an older commit (there it measures speed=None alone): that is how the parent's number
is taken, on the same box, in the same session.

    python scripts/speed_measure.py [vocode] [launch]        (default: both; one JSON line per row)"""
import inspect
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import ops, synth  # noqa: E402
from chatterbox_amd.engine import ChatterboxEngine  # noqa: E402

dev = torch.device("cuda", 0)
what = set(sys.argv[1:]) or {"vocode", "launch"}
say = lambda **kw: print(json.dumps(kw), flush=True)
B, N, REPS = 8, 250, 5
has_speed = "speed" in inspect.signature(ChatterboxEngine.vocode).parameters

if "vocode" in what:
    eng = ChatterboxEngine.__new__(ChatterboxEngine)  # flow + vocoder only, as ChatterboxVC builds it
    from chatterbox_amd.hift import HiFTEngine
    from chatterbox_amd.s3gen import FlowEngine
    s3 = synth.s3gen_state_dict(0)
    eng.dev, eng.t3, eng.flow, eng.hift, eng.last_timing = dev, None, FlowEngine(s3, dev), HiFTEngine(s3, dev), {}
    ref = synth.s3gen_ref()
    st = [synth.speech_tokens(N, seed=k) for k in range(B)]
    speeds = [None, 0.8, 1.25] if has_speed else [None]
    res = {s: [] for s in speeds}
    for rep in range(REPS + 2):
        for s in speeds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wavs, _ = eng.vocode(st, ref, **({} if s is None else dict(speed=s)))
            torch.cuda.synchronize()
            if rep >= 2:
                res[s].append((time.perf_counter() - t0, eng.last_timing["flow_s"], eng.last_timing["hift_s"], int(wavs[0].numel())))
    for s in speeds:
        med = lambda i: round(1e3 * statistics.median(r[i] for r in res[s]), 2)
        say(part="vocode", B=B, tokens=N, speed=s, samples_per_utterance=res[s][0][3], total_ms=med(0), flow_ms=med(1), vocoder_ms=med(2),
            runs_total_ms=[round(1e3 * r[0], 2) for r in res[s]])

if "launch" in what and has_speed:
    mel = torch.randn(B, 2 * N, 80, device=dev) * 3 - 5
    for s in (0.8, 1.25):
        ts = []
        for i in range(35):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, _ = ops.mel_time_scale(mel, [s] * B, in_lens=[2 * N] * B)
            e1.record()
            e1.synchronize()
            if i >= 5:
                ts.append(e0.elapsed_time(e1))
        mb = (out.numel() + 2 * out.numel()) * 4 / 1e6  # one float4 written, two read (neighbouring threads share lines: an upper bound on HBM traffic)
        say(part="launch", speed=s, frames_in=2 * N, frames_out=out.shape[1], median_us=round(1e3 * statistics.median(ts), 1), min_us=round(1e3 * min(ts), 1), MB_touched=round(mb, 2))
