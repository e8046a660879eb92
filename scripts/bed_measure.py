"""What a music bed costs, one process on one box: the two-voice eight-turn script of scripts/dialogue_measure.py on the synthetic full-size
ChatterboxTTS (30 T3 layers; the token budget cut to --tokens per chunk with end-of-speech banned), delivered with loudness=-16, true_peak=-1, encoding="s16",
three forms ALTERNATING inside every repetition, same seed:
  plain       generate_dialogue without a bed -- the parent commit's call
  device      generate_dialogue(bed=...): the bed laid and ducked inside the finishing visit (two meter readings, the level launch, cbx_wave_duck_f32)
  host        what a producer did before: generate_dialogue without a bed and without a finish (24 kHz fp32 back to the host), the bed laid by the NumPy float32
              restatement of the definition (tests/bed_common.py; the gain taken from the device form, so no host meter is counted), then a SECOND visit to the
              device for loudness, true_peak and the s16 store over the sum
Times are a host clock around each call (each ends in a copy to the host).  The device and host forms are compared sample for sample (the s16 results may differ
by the restatement's roundings: the count of differing samples and the largest difference are reported, nothing is asserted).  Writes one JSON line -- median, min
and max per form over the repetitions, the differences of the medians, the sizes -- to the log (default profiles/bed_measure.log) and prints it.

    python scripts/bed_measure.py [repetitions, default 5] [log path] [--tokens 150]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bed_common  # noqa: E402  (the NumPy statement of the definition)
from chatterbox_amd import api, ops, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
tokens = int(sys.argv[sys.argv.index("--tokens") + 1]) if "--tokens" in sys.argv else 150
if "--tokens" in sys.argv:
    args.remove(str(tokens))
reps = int(args[0]) if args else 5
log = args[1] if len(args) > 1 else "profiles/bed_measure.log"
assert torch.cuda.is_available(), "this measurement needs the MI355X"
dev = torch.device("cuda:0")

SENTENCES = ["Welcome back to the show, it is good to have you.", "Thank you, I have been looking forward to this.", "Let us begin with the question everyone asks.",
             "Go ahead, I think I know which one you mean.", "How did the project start, and who was there?", "It started in a kitchen, with three of us and a laptop.",
             "And when did you know that it would work?", "Honestly, not until the day we shipped the thing."]


class _Tok:
    """a stand-in tokenizer (the synthetic model has none): one id per character"""

    def text_to_tokens(self, text, language_id=None):
        return torch.tensor([[3 + (ord(c) % 600) for c in text]], dtype=torch.int32)


m = api.ChatterboxTTS.from_synthetic(dev)
m.tokenizer, m.watermarker = _Tok(), None
syn, pip = m.engine.synthesize, m.engine.synthesize_pipelined
m.engine.synthesize = lambda *a, **kw: syn(*a, **{**kw, "max_new_tokens": tokens, "ban_eos": True})
m.engine.synthesize_pipelined = lambda jobs, **kw: pip(jobs, **{**kw, "max_new_tokens": tokens, "ban_eos": True})
voices = dict(host=m.conds, guest=api.Conditionals(api.T3Cond(**synth.t3_cond(seed=7)), synth.s3gen_ref(seed=7)))
turns = [dict(voice=("host", "guest")[k % 2], text=s, gap=(0.3, -0.2)[k % 2]) for k, s in enumerate(SENTENCES)]
source = bed_common.bed(10 * 24000, 1)   # ten seconds of "music": it loops under the conversation
BED = dict(audio=(source, 24000), lead=1.0, tail=1.5)
plan = ops.check_bed(BED)
fin = dict(loudness=-16, true_peak=-1, encoding="s16")
say = lambda **kw: m.generate_dialogue(turns, voices, seed=5, max_chars=60, balance=True, **kw)
gain = [1.0]


def on_host():
    speech = say()[0].numpy()
    summed = bed_common.oracle(speech, source, plan, gain[0], np.float32)["out"]
    return m._finish(torch.from_numpy(summed), ops.check_format(None, "s16"), converted=False, loud=-16.0, peak=-1.0)


forms = {"plain": lambda: say(**fin), "device": lambda: say(bed=BED, **fin), "host": on_host}
out = {}
for k in ("plain", "device", "host"):  # (tables, allocator, code objects, the voice-prefix caches; the device form leaves the gain the host form uses)
    out[k] = forms[k]()
    if k == "device":
        gain[0], last_bed = m.last_bed["gain"], dict(m.last_bed)
diff = (out["device"][0].int() - out["host"][0].int()).abs()
ms = {k: [] for k in forms}
for _ in range(reps):
    for name, fn in forms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms[name].append((time.perf_counter() - t0) * 1e3)
summary = lambda v: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
med = {k: statistics.median(v) for k, v in ms.items()}
line = json.dumps(dict(script=f"{len(SENTENCES)} turns, {tokens} speech tokens each, two voices", samples={k: int(w.shape[1]) for k, w in out.items()}, repetitions=reps,
                       ms_per_call={k: summary(v) for k, v in ms.items()}, ms_device_minus_plain=round(med["device"] - med["plain"], 2),
                       ms_host_minus_plain=round(med["host"] - med["plain"], 2), ms_host_minus_device=round(med["host"] - med["device"], 2), last_bed=last_bed,
                       s16_samples_differing_device_against_host=int((diff > 0).sum()), s16_largest_difference=int(diff.max()), gpu=torch.cuda.get_device_name(0)))
print(line, flush=True)
with open(log, "w") as f:
    f.write(line + "\n")
