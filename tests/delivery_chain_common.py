"""What the engines do with the delivery options (seeds, speed, pitch, join, format, loudness, pauses), as data: record() runs
  * ChatterboxEngine.vocode over stand-in flow / vocoder stages on the CPU (the setup of test_wave_squeeze_host.py's
    test_vocode_squeezes_on_the_stream_of_the_waveforms: three rows of 12, 5 and 9 tokens, a 6-token prompt) for every combination of speed, pitch, loudness,
    pauses, join, format and sync -- the ordered ops calls behind the vocoder with their arguments, the structure of what is returned, last_loudness / last_pauses;
  * ChatterboxEngine.synthesize and TurboEngine.synthesize over a stand-in T3 with vocode spied -- the exact keywords that reach vocode (and T3) per option;
  * engine._checked_job over a table of jobs -- its output, or the exception's type and the argument it names.
The ops that would launch (mel_time_scale, wave_pitch, wave_normalize, wave_squeeze, wave_join, wave_format) and cut_pauses are recorders that return results of the
right structure: nothing is launched.  A tensor is written as its length (a 1-D row) or its shape; scalars, dicts and lists stay as they are.
tests/golden/delivery_chain.json is the list as the code gave it before the option path was folded into one record and one chain; test_delivery_chain_host.py
compares the two.  Rewrite the fixture (python tests/delivery_chain_common.py) only for a change that is MEANT to alter what the engines do."""
import contextlib
import itertools
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "delivery_chain.json")
CPU = torch.device("cpu")
N_TOKENS, N_PROMPT = (12, 5, 9), 6
ON = dict(speed=[1.25, None, 0.5], pitch=[2, None, -3], loudness=[-16, None, -23], pauses=dict(keep=[2, 0, 3], db=30), join=dict(gaps=[5, 0, 7], trim_db=40),
          format=dict(sample_rate=8000, encoding="mulaw"))
OFF = dict(seeds=[None], speed=[None, 1.0, [None, 1.0, None]], pitch=[None, 0, [None, 0, None]], join=[None], format=[None, dict(sample_rate=24000, encoding="f32")],
           loudness=[None, [None] * 3], pauses=[None, [None, 0, None], dict(keep=0)])
BAD = dict(seeds=[[1, 2], [1, 2, -3]], speed=[3.0, "fast"], pitch=[13, [1, 2]], join=[dict(gaps=[1]), [1, 2, 3]], format=[dict(sample_rate=11025), "wav"],
           loudness=[-3, [None, -16]], pauses=[dict(keep=[1, 2, 2]), 5])


def enc(v):
    if torch.is_tensor(v):
        return int(v.numel()) if v.dim() == 1 else dict(shape=list(v.shape))
    if isinstance(v, dict):
        return {k: enc(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [enc(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"delivery_chain: no JSON form for a {type(v).__name__}")


def shape_of(res):
    """The structure of what vocode / synthesize returns as audio: a list or a dict with its keys, tensors as their lengths"""
    return enc(res)


def raised(fn):
    """fn()'s exception as dict(error=its type, names=the argument its message begins with)"""
    try:
        fn()
    except (TypeError, ValueError) as e:
        return dict(error=type(e).__name__, names=re.match(r"[a-z_]*", str(e)).group(0))
    raise AssertionError("nothing was raised")


@contextlib.contextmanager
def recording_ops(calls):
    from chatterbox_amd import ops

    def mel_time_scale(mel, rates, in_lens=None):
        calls.append(["mel_time_scale", enc(mel), rates, in_lens])
        out = [ops.scaled_len(n, r) for n, r in zip(in_lens, rates)]
        return torch.ones(mel.shape[0], max(out), 80), torch.tensor(out, dtype=torch.int32)

    def wave_pitch(rows, steps, out_lens):
        calls.append(["wave_pitch", enc(rows), steps, out_lens])
        return [torch.zeros(n) for n in out_lens]

    def wave_normalize(rows, loud):
        calls.append(["wave_normalize", enc(rows), loud])
        return "loudness stats"

    def wave_squeeze(rows, keep, db, fade):
        calls.append(["wave_squeeze", enc(rows), keep, db, fade])
        return dict(rows=[r.clone() for r in rows], stats=torch.tensor([[int(r.numel()) - 480 * k, 1, k, int(r.numel())] for r, k in zip(rows, keep)], dtype=torch.int32), edges=None)

    def wave_join(rows, **kw):
        calls.append(["wave_join", enc(rows), enc(kw)])
        n = [int(r.numel()) for r in rows]
        piece = dict(out=kw["out"] if kw.get("out") is not None else torch.zeros(sum(n) + sum(kw["gaps"])), rec=torch.zeros(3 * len(n) + 1, dtype=torch.int32), n=n)
        return dict(piece, pauses=torch.zeros(len(n), 4, dtype=torch.int32)) if kw.get("squeeze") is not None else piece

    def wave_format(rows, fmt):
        calls.append(["wave_format", enc(rows), fmt])
        return [r[: ops.formatted_len(int(r.numel()), fmt["sample_rate"])] for r in rows]

    real_cut = ops.cut_pauses

    def cut_pauses(rows, stats, fmt=None):
        calls.append(["cut_pauses", enc(rows), stats.tolist(), fmt])
        return real_cut(rows, stats, fmt)

    stand_ins = dict(mel_time_scale=mel_time_scale, wave_pitch=wave_pitch, wave_normalize=wave_normalize, wave_squeeze=wave_squeeze, wave_join=wave_join, wave_format=wave_format,
                     cut_pauses=cut_pauses)
    real = {k: getattr(ops, k) for k in stand_ins}
    real_sync, torch.cuda.synchronize = torch.cuda.synchronize, lambda *a, **k: None
    for k, v in stand_ins.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        torch.cuda.synchronize = real_sync
        for k, v in real.items():
            setattr(ops, k, v)


def _engine(cls):
    eng = cls.__new__(cls)
    eng.dev, eng.last_timing, eng.last_pauses, eng.last_loudness = CPU, {}, None, None
    eng.flow = type("Flow", (), {"precision": 1, "co_resident": lambda self, on: None,
                                 "inference": lambda self, tok, lens, ref, **kw: torch.ones(tok.shape[0], 2 * tok.shape[1], 80)})()
    eng.hift = type("Hift", (), {"precision": 1, "inference": staticmethod(lambda mel, lens=None, **kw: (torch.zeros(mel.shape[0], 480 * mel.shape[1]), None))})()
    return eng


def record_vocode(out):
    from chatterbox_amd import engine, synth
    eng = _engine(engine.ChatterboxEngine)
    ref = synth.s3gen_ref(n_prompt_tokens=N_PROMPT)
    st = [synth.speech_tokens(n, seed=k) for k, n in enumerate(N_TOKENS)]
    names = ("speed", "pitch", "loudness", "pauses", "join", "format")
    for flags in itertools.product((False, True), repeat=len(names) + 1):
        on, sync = [n for n, f in zip(names, flags) if f], flags[-1]
        if "loudness" in on and "join" in on:
            continue
        calls = []
        eng.last_loudness = eng.last_pauses = None
        with recording_ops(calls):
            res, mel = eng.vocode(st, ref, sync=sync, **{n: ON[n] for n in on})
        out.append(dict(what="vocode", on=on, sync=sync, calls=calls, result=shape_of(res), last_loudness=enc(eng.last_loudness), last_pauses=enc(eng.last_pauses)))
    with recording_ops([]):
        out.append(dict(what="vocode", on=["loudness", "join"], **raised(lambda: eng.vocode(st, ref, loudness=ON["loudness"], join=ON["join"]))))


class _T3:
    """T3 that returns fixed tokens and keeps the keywords it was called with"""
    MAX_BATCH, last_guard = 4, "the report"

    def __init__(self, toks):
        self.toks, self.kw = toks, None

    def generate(self, conds, text_tokens, **kw):
        self.kw = kw
        return self.toks

    def check_guard(self, guard):
        return dict(guard)

    def check_align_heads(self, heads):
        return heads

    def align(self, text_tokens, toks, align_heads=None):
        return [torch.tensor([[i, i + 1] for i in range(int(t.numel()))]) for t in text_tokens]


def record_synthesize(out):
    from chatterbox_amd import engine
    from chatterbox_amd.t3 import START_SPEECH, STOP_SPEECH
    text = [torch.arange(n) for n in (4, 2, 3)]
    body = [torch.arange(10, 10 + n) for n in N_TOKENS]
    llama = [torch.cat([torch.tensor([START_SPEECH]), b, torch.tensor([STOP_SPEECH])]) for b in body[:2]] + [torch.cat([torch.tensor([START_SPEECH]), body[2]])]
    for cls, toks, more in ((engine.ChatterboxEngine, llama, dict(words=dict(heads=None), guard=dict(tail=2.0))), (engine.TurboEngine, body, {})):
        eng = _engine(cls)
        eng.t3 = _T3(toks)
        seen = {}

        def vocode(speech_tokens, gen_ref, **kw):
            seen.update(tokens=enc(speech_tokens), keys=" ".join(sorted(kw)), on=enc({k: v for k, v in kw.items() if v is not None and k not in ("n_cfm_timesteps", "drop_last_token")}))
            n = [960 * int(t.numel()) for t in speech_tokens]
            if kw.get("join") is None:
                return [torch.zeros(k) for k in n], None
            piece = dict(out=torch.zeros(sum(n)), rec=torch.zeros(3 * len(n) + 1, dtype=torch.int32), n=n)
            if kw.get("format") is not None:
                piece.update(formatted=torch.zeros(sum(n) // 3, dtype=torch.uint8), format=kw["format"])
            return (dict(piece, pauses=torch.zeros(len(n), 4, dtype=torch.int32)) if kw.get("pauses") is not None else piece), None
        eng.vocode = vocode
        on = dict(ON, seeds=[1, 2, 3], **more)
        cases = [("nothing", {})] + [(f"{k} alone", {k: v}) for k, v in on.items()]
        cases += [("all but join and pauses", {k: v for k, v in on.items() if k not in ("join", "pauses")}),   # (loudness excludes a join, words exclude pauses)
                  ("all but loudness and words", {k: v for k, v in on.items() if k not in ("loudness", "words")})]
        cases += [(f"{k} off ({i})", {k: v}) for k, vals in dict(OFF, **{k: [None] for k in more}).items() for i, v in enumerate(vals)]
        for name, kw in cases:
            seen.clear()
            with recording_ops([]):
                res = eng.synthesize(text, None, None, **kw)
            out.append(dict(what=f"{cls.__name__}.synthesize", case=name, vocode=dict(seen), t3=enc({k: eng.t3.kw[k] for k in ("seeds", "guard") if k in eng.t3.kw}),
                            n_results=len(res), result=shape_of(res[0]), last_guard=eng.last_guard if more else None))
        for k, vals in BAD.items():
            for i, v in enumerate(vals):
                out.append(dict(what=f"{cls.__name__}.synthesize", case=f"{k} invalid ({i})", **raised(lambda: eng.synthesize(text, None, None, **{k: v}))))
        out.append(dict(what=f"{cls.__name__}.synthesize", case="loudness with join", **raised(lambda: eng.synthesize(text, None, None, loudness=-16, join=ON["join"]))))
        out.append(dict(what=f"{cls.__name__}.synthesize", case="speed x pitch", **raised(lambda: eng.synthesize(text, None, None, speed=2.0, pitch=-12))))


def record_checked_job(out):
    from chatterbox_amd import engine
    base = dict(text_tokens=[torch.zeros(n, dtype=torch.long) for n in (4, 2, 3)], t3_conds=None, gen_ref=None, temperature=0.7)
    on = dict(ON, seeds=[1, 2, 3], guard=dict(tail=2.0))
    table = [("nothing", {})] + [(f"{k} on", {k: v}) for k, v in on.items()] + [("everything but loudness", {k: v for k, v in on.items() if k != "loudness"}),
                                                                              ("everything but the join", {k: v for k, v in on.items() if k != "join"})]
    table += [(f"{k} off ({i})", {k: v}) for k, vals in dict(OFF, words=[None], guard=[None]).items() for i, v in enumerate(vals)]
    table += [("one seed for all", dict(seeds=7)), ("one speed for all", dict(speed=0.8, pitch=1)), ("a generator", dict(generator="a generator"))]
    for name, opts in table:
        out.append(dict(what="_checked_job", case=name, job=enc(engine._checked_job(dict(base, **opts)))))
    bad = [(f"{k} invalid ({i})", {k: v}) for k, vals in BAD.items() for i, v in enumerate(vals)]
    bad += [("loudness with join", dict(loudness=-16, join=ON["join"])), ("speed x pitch", dict(speed=2.0, pitch=-12)), ("words", dict(words=dict(heads=None))),
            ("seeds with a generator", dict(seeds=[1, 2, 3], generator="a generator"))]
    for name, opts in bad:
        out.append(dict(what="_checked_job", case=name, **raised(lambda: engine._checked_job(dict(base, **opts)))))


def _walk(v, fn):
    """v with fn applied top-down: where fn returns something, that replaces the sub-value whole"""
    r = fn(v)
    if r is not None:
        return r
    return {k: _walk(x, fn) for k, x in v.items()} if isinstance(v, dict) else [_walk(x, fn) for x in v] if isinstance(v, list) else v


def pack(entries):
    """The entries with every list / dict inside them that occurs four times or more written once: -> [dict(definitions={"$k": value}), *entries with "$k" in its
    place] (an entry itself is never replaced)"""
    key = lambda v: json.dumps(v, separators=(",", ":")) if isinstance(v, (list, dict)) else None
    inside = lambda fn: [{k: _walk(x, fn) for k, x in e.items()} for e in entries]
    count = {}
    inside(lambda v: count.__setitem__(key(v), count.get(key(v), 0) + 1))
    names = {k: f"${i}" for i, k in enumerate(k for k, n in count.items() if k is not None and n >= 4 and len(k) >= 16)}
    packed, used = inside(lambda v: names.get(key(v))), set()
    _walk(packed, lambda v: used.add(v) if isinstance(v, str) else None)   # (a repeated value inside a larger repeated value is not needed)
    return [dict(definitions={name: json.loads(k) for k, name in names.items() if name in used})] + packed


def unpack(packed):
    defs = packed[0]["definitions"]
    return [_walk(e, lambda v: defs.get(v) if isinstance(v, str) else None) for e in packed[1:]]


def write(entries, path):
    """the packed entries, one per line"""
    entries = json.loads(json.dumps(entries))
    assert unpack(pack(entries)) == entries
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in pack(entries)) + "\n]\n")
    print(f"{len(entries)} entries -> {path} ({os.path.getsize(path)} bytes)")


def record():
    out = []
    record_vocode(out)
    record_synthesize(out)
    record_checked_job(out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    write(record(), FIXTURE)
