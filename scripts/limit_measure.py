"""The cost of the true-peak limiter in the delivery chain, one process on one box: 8 rows of 10 s (240 000 samples each, noise bursts whose level changes every
50 ms) through the two forms of the step that _deliver runs behind the vocoder, ALTERNATING inside every repetition:
  loudness        ops.wave_normalize(rows, -16): the meter with the sample-peak cap and ops.wave_gain in place -- the parent commit's path, five launches
  loudness+peak   ops.wave_loudness(rows, -16, ceiling=None) and ops.wave_limit(rows, -1, gain=...): the meter with the full gain, then the limiter with that
                  gain as its pre-gain into a new buffer -- six launches
  peak            ops.wave_limit(rows, -1) alone -- two launches
Every repetition starts from a fresh copy of the rows (outside the timed span).  Times are device events around the calls and the host's time to enqueue them.
Writes one JSON line -- median, min and max per form over the repetitions, and what the limiter did -- to the log (default profiles/limit_measure.log) and prints it.

    python scripts/limit_measure.py [repetitions, default 30] [log path]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from chatterbox_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
log = sys.argv[2] if len(sys.argv) > 2 else "profiles/limit_measure.log"
R, n = 8, 240000
g = torch.Generator(device="cpu").manual_seed(1)
level = torch.tensor([0.003, 0.05, 0.3, 0.9])[torch.randint(0, 4, (R, n // 1200), generator=g)].repeat_interleave(1200, dim=1)
src = (torch.randn(R, n, generator=g) * level * 0.25).to(dev)
work = torch.empty_like(src)
rows = [work[b] for b in range(R)]


def loudness():
    return ops.wave_normalize(rows, [-16.0] * R)


def loudness_peak():
    stats, gain = ops.wave_loudness(rows, [-16.0] * R, None)
    return ops.wave_limit(rows, [-1.0] * R, gain=gain)[1]


def peak():
    return ops.wave_limit(rows, [-1.0] * R)[1]


forms = {"loudness": loudness, "loudness+peak": loudness_peak, "peak": peak}
for fn in forms.values():  # (tables, allocator, code objects)
    work.copy_(src)
    fn()
torch.cuda.synchronize()
us = {k: [] for k in forms}
host_us = {k: [] for k in forms}
for _ in range(reps):
    for name, fn in forms.items():
        work.copy_(src)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        last = fn()
        host_us[name].append((time.perf_counter() - t0) * 1e6)
        e1.record()
        torch.cuda.synchronize()
        us[name].append(e0.elapsed_time(e1) * 1e3)
        if name == "loudness+peak":
            lim = last.cpu()
summary = lambda v: dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
line = json.dumps(dict(shape=f"{R} x {n}", repetitions=reps, us_between_events={k: summary(v) for k, v in us.items()}, host_us_to_enqueue={k: summary(v) for k, v in host_us.items()},
                       limiter=dict(true_peak_before=[round(float(v), 3) for v in lim[:, 0]], min_gain=[round(float(v), 3) for v in lim[:, 1]],
                                    share_gained_down=round(float(lim[:, 2].sum()) / (R * n), 4), share_over_ceiling=round(float(lim[:, 3].sum()) / (R * n), 4)),
                       gpu=torch.cuda.get_device_name(0)))
print(line, flush=True)
with open(log, "w") as f:
    f.write(line + "\n")
