"""One variant per process (variant a uses nothing newer than generate(), so it also runs from a checkout of an older commit): a = 8 sequential generate(), b = one generate_batch of 8, c = engine.synthesize on the same batch (the floor).
configs[2] shape: Multilingual, synthetic 30-layer weights, 64 text tokens, 250 sampled tokens (10 s) per utterance, 3 voices."""
import json, sys, time
import torch
sys.path.insert(0, ".")
from chatterbox_amd import api, synth

variant, reps = sys.argv[1], 3
dev = torch.device("cuda:0")
m = api.ChatterboxMultilingualTTS.from_synthetic(dev, t3_layers=30)


class Tok:
    def text_to_tokens(self, text, language_id=None):
        return synth.text_tokens(62, seed=len(text)).int().unsqueeze(0)   # + SOT / EOT = 64 text tokens


m.tokenizer = Tok()
gen = m.engine.t3.generate
m.engine.t3.generate = lambda conds, tt, **kw: gen(conds, tt, **dict(kw, max_new_tokens=250, ban_eos=True))
voices = [api.Conditionals(api.T3Cond(**synth.t3_cond(seed=s)), synth.s3gen_ref(seed=s)) for s in (11, 12, 13)]
conds = [voices[k % 3] for k in range(8)]
texts = ["x" * (10 + k) + "." for k in range(8)]
tts = [torch.cat([torch.tensor([255]), synth.text_tokens(62, seed=len(t)), torch.tensor([0])]) for t in texts]


def run():
    if variant == "a":
        out = []
        for k in range(8):
            m.conds = conds[k]
            out.append(m.generate(texts[k], "en"))
        return out
    if variant == "b":
        return m.generate_batch(texts, "en", conds=conds)
    wavs, _ = m.engine.synthesize(tts, [api._t3_dict(c.t3, 0.5) for c in conds], [c.gen for c in conds], max_new_tokens=1000, drop_last_token=True)
    torch.cuda.synchronize()
    return wavs


run()
ts = []
for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
fin = None
if variant == "c":  # the per-utterance _finish cost the public call adds (D2H + float + unsqueeze; no watermarker loaded)
    t0 = time.perf_counter()
    fin_out = [m._finish(w) for w in out]
    fin = time.perf_counter() - t0
audio_s = sum(w.shape[-1] for w in out) / 24000.0
print(json.dumps(dict(variant=variant, seconds=[round(t, 4) for t in ts], best_s=round(min(ts), 4), audio_s=round(audio_s, 2),
                      x_realtime=round(audio_s / min(ts), 1), finish_all_s=None if fin is None else round(fin, 5), gpu=torch.cuda.get_device_name(0))), flush=True)
