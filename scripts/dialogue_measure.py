"""What a conversation costs, one process on one box: an eight-turn script on the synthetic full-size ChatterboxTTS (30 T3 layers; the
token budget cut to --tokens per chunk with end-of-speech banned, so every form synthesises the same amount of audio), three forms ALTERNATING inside every
repetition, same seed:
  long        generate_long(the eight sentences as one text, one voice) -- the parent commit's code path
  dialogue-1  generate_dialogue(one turn per sentence, ONE voice, turn_pause = pause): bit for bit the same waveform -- the expectation to confirm or refute is that
              it costs what `long` costs plus the finishing visit
  dialogue-2  generate_dialogue(the same turns, TWO voices alternating, every second turn coming in 0.2 s early, balance=True)
and, inside the two dialogue forms, the finishing visit on its own (upload of the pieces, the meter of balance=, the mix, the one copy to the host): a host clock
around _TTS._mix_dialogue, which ends in the device-to-host copy.  Times are a host clock around each call (each ends in a copy to the host).  Writes one JSON line --
median, min and max per form over the repetitions, the differences of the medians, the sizes -- to the log (default profiles/dialogue_measure.log) and prints it.

    python scripts/dialogue_measure.py [repetitions, default 5] [log path] [--tokens 150]
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from chatterbox_amd import api, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
tokens = int(sys.argv[sys.argv.index("--tokens") + 1]) if "--tokens" in sys.argv else 150
if "--tokens" in sys.argv:
    args.remove(str(tokens))
reps = int(args[0]) if args else 5
log = args[1] if len(args) > 1 else "profiles/dialogue_measure.log"
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
other = api.Conditionals(api.T3Cond(**synth.t3_cond(seed=7)), synth.s3gen_ref(seed=7))
voices = dict(host=m.conds, guest=other)
visit = []
mix = m._mix_dialogue


def timed_mix(*a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mix(*a, **kw)
    visit.append((time.perf_counter() - t0) * 1e3)
    return out


m._mix_dialogue = timed_mix
forms = {
    "long": lambda: m.generate_long(" ".join(SENTENCES), seed=5, max_chars=60),
    "dialogue-1": lambda: m.generate_dialogue([(None, s) for s in SENTENCES], seed=5, max_chars=60, turn_pause=0.15),
    "dialogue-2": lambda: m.generate_dialogue([dict(voice=("host", "guest")[k % 2], text=s, gap=(0.3, -0.2)[k % 2]) for k, s in enumerate(SENTENCES)], voices, seed=5,
                                              max_chars=60, balance=True),
}
out = {k: fn() for k, fn in forms.items()}  # (tables, allocator, code objects, the voice-prefix caches)
assert torch.equal(out["long"], out["dialogue-1"]), "a one-voice dialogue is generate_long bit for bit"
ms = {k: [] for k in forms}
visits = {"dialogue-1": [], "dialogue-2": []}
for _ in range(reps):
    for name, fn in forms.items():
        torch.cuda.synchronize()
        visit.clear()
        t0 = time.perf_counter()
        fn()
        ms[name].append((time.perf_counter() - t0) * 1e3)
        if name in visits:
            visits[name].append(visit[0])
summary = lambda v: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
med = {k: statistics.median(v) for k, v in ms.items()}
line = json.dumps(dict(script=f"{len(SENTENCES)} turns, {tokens} speech tokens each", samples={k: int(w.shape[1]) for k, w in out.items()}, repetitions=reps,
                       ms_per_call={k: summary(v) for k, v in ms.items()}, ms_finishing_visit={k: summary(v) for k, v in visits.items()},
                       ms_dialogue1_minus_long=round(med["dialogue-1"] - med["long"], 2), ms_dialogue2_minus_long=round(med["dialogue-2"] - med["long"], 2),
                       balance=m.last_balance, gpu=torch.cuda.get_device_name(0)))
print(line, flush=True)
with open(log, "w") as f:
    f.write(line + "\n")
