"""What the finishing visit costs, one process on one box: the finish of a dialogue of eight chunks of 10 s each (two voices alternating,
every second turn coming in 0.2 s early, balance=True), with loudness=-16, true_peak=-1, sample_rate=48000, encoding="s16" -- the "-16 LUFS at -1 dBTP"
delivery --, three forms ALTERNATING inside every repetition on the same pieces:
  mono    _TTS._mix_dialogue: upload, the balance meter, cbx_wave_mix_f32, then the chain: the meter, the limiter, the format, the one copy to the host
  stereo  _TTS._mix_dialogue with pan= (the voices at -0.3 / +0.3): upload, the balance meter, cbx_wave_pan_mix_f32, then the chain over two planes:
          cbx_wave_loudness_ch_f32, cbx_wave_limit_ch_f32, the format over two rows, the one copy to the host
  long    _Finish._finish(the eight pieces as one 80 s waveform on the host, converted=False, loud=-16, peak=-1): generate_long's finish -- upload, the chain
          (the waveform is concatenated once, outside the clock)
The script runs on older checkouts too, so that two commits can be compared in one visit: where the stereo finish is a method of its own
(_mix_dialogue_stereo) that one is called, and where there is no pan= at all the stereo form is left out.  _finish has had this signature throughout.
The pieces are synthetic waveforms (seeded noise bursts; the finish does not depend on who spoke them), so no synthesis runs and the model is the small synthetic
one (two T3 layers): only its device and its delivery options are used.  Times are a host clock around each call; each call ends in the device-to-host copy, which
synchronises.  Every form is warmed up once (tables, allocator, code objects).  Writes one JSON line -- median, min and max per form over the repetitions, the
ratio of the stereo and mono medians, the sizes -- to the log (default profiles/stereo_measure.log) and prints it.

    python scripts/stereo_measure.py [repetitions, default 20] [log path]
"""
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from chatterbox_amd import api, ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
log = sys.argv[2] if len(sys.argv) > 2 else "profiles/stereo_measure.log"
assert torch.cuda.is_available(), "this measurement needs the MI355X"
dev = torch.device("cuda:0")

CHUNKS, N = 8, 240000   # eight chunks of 10 s at 24 kHz
m = api.ChatterboxTTS.from_synthetic(dev, t3_layers=2)
m.watermarker = None
rng = np.random.default_rng(5)
pieces = []
for k in range(CHUNKS):   # words of 0.3 s at changing levels with short silences between them, the second voice 6 dB quieter
    amp = np.repeat(rng.choice([0.0, 0.05, 0.15, 0.3], size=N // 7200 + 1), 7200)[:N] * (1.0 if k % 2 == 0 else 0.5)
    pieces.append(torch.from_numpy((rng.standard_normal(N) * amp).astype(np.float32)))
recs = [dict(edges=[(0, N)], offsets=[0], n=[N], total=N) for _ in range(CHUNKS)]
after = [(-4800 if k % 2 == 0 else 7200) for k in range(CHUNKS - 1)] + [0]
row_voice, keys = [k % 2 for k in range(CHUNKS)], ["host", "guest"]
opts = api._Options(m, loudness=-16, true_peak=-1, sample_rate=48000, encoding="s16")
forms = {"mono": lambda: m._mix_dialogue(pieces, recs, after, row_voice, keys, api.DIALOGUE_BALANCE, 240, opts)[0]}
pan = [ops.pan_gains((-0.3, 0.3)[v]) for v in row_voice] if hasattr(ops, "pan_gains") else None
if pan is None:
    pass
elif hasattr(m, "_mix_dialogue_stereo"):
    forms["stereo"] = lambda: m._mix_dialogue_stereo(pieces, recs, after, row_voice, keys, api.DIALOGUE_BALANCE, 240, opts, pan)[0]
elif "pan" in inspect.signature(m._mix_dialogue).parameters:
    forms["stereo"] = lambda: m._mix_dialogue(pieces, recs, after, row_voice, keys, api.DIALOGUE_BALANCE, 240, opts, pan=pan)[0]
whole = torch.cat(pieces)
forms["long"] = lambda: m._finish(whole, opts.fmt, converted=False, loud=-16.0, peak=-1.0)
out = {k: fn() for k, fn in forms.items()}   # (the warm-up)
ms = {k: [] for k in forms}
for _ in range(reps):
    for name, fn in forms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms[name].append((time.perf_counter() - t0) * 1e3)
summary = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
med = {k: statistics.median(v) for k, v in ms.items()}
line = json.dumps(dict(script=f"{CHUNKS} chunks of {N} samples, two voices, balance, loudness=-16, true_peak=-1, 48000 Hz s16", shape={k: list(w.shape) for k, w in out.items()},
                       dtype=str(out["mono"].dtype), repetitions=reps, ms_finishing_visit={k: summary(v) for k, v in ms.items()},
                       stereo_over_mono=round(med["stereo"] / med["mono"], 3) if "stereo" in med else None, gpu=torch.cuda.get_device_name(0)))
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
with open(log, "w") as f:
    f.write(line + "\n")
