"""Latency of Turbo / Nano streaming against the one-shot call, and the chunked token step through cbx_gpt2_loop_run against the Python replay loop
(README).  One process = one measurement kind; scripts/turbo_stream_measure.sh interleaves the processes.

    python scripts/turbo_stream_measure.py latency --model turbo|nano [--reps 5]
        seeded synthetic full-depth model (Turbo: 24 layers, D = 1024; Nano: 12 layers, D = 768), batch 1, a 10 s utterance (250 tokens, EOS banned so
        every run has the same length).  Reps alternate inside the process: one-shot ChatterboxTurboTTS._generate (the body of generate(), which has no
        length argument), then TurboEngine.synthesize_stream with overlap on and off (the engine of generate_stream).  Per rep: wall time of the one-shot
        call, time to the first yielded piece and wall time of the whole stream.
    python scripts/turbo_stream_measure.py loop --impl c|py [--steps 200]
        Turbo T3 alone, batch 1: ms per token step of `steps` steps enqueued through cbx_gpt2_loop_run (poll_every = 0) resp. replayed from Python (the
        one-shot generate()'s loop: one torch graph replay per token), HIP events around the enqueue on the launch stream, best of 3.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SAMP = dict(temperature=0.8, top_k=1000, top_p=0.95, repetition_penalty=1.2)


def latency(model, reps):
    from chatterbox_amd import synth
    from chatterbox_amd.api import ChatterboxTurboTTS
    m = ChatterboxTurboTTS.from_synthetic("cuda", nano=model == "nano")
    m.watermarker = None
    eng, ids = m.engine, synth.turbo_text_tokens(64)
    kw = dict(max_gen_len=249, ban_eos=True, ban_from=6561, **SAMP)
    res = dict(oneshot=[], first_ov=[], total_ov=[], first_serial=[], total_serial=[])

    def stream(overlap):
        torch.cuda.synchronize()
        t0, first = time.perf_counter(), None
        n = 0
        for r in eng.synthesize_stream([ids], m.conds.t3.as_dict(), m.conds.gen, overlap=overlap, **kw):
            if first is None and r["wavs"][0].numel():
                first = time.perf_counter() - t0
            n += r["wavs"][0].numel()
        torch.cuda.synchronize()
        return first, time.perf_counter() - t0, n

    for rep in range(reps + 1):  # rep 0: warm-up (graph captures, kernel loads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav = m._generate(ids, **kw)
        t1 = time.perf_counter() - t0
        f_ov, t_ov, n_ov = stream(True)
        f_se, t_se, n_se = stream(False)
        assert n_ov == n_se == wav.shape[1], (n_ov, n_se, wav.shape)
        if rep:
            for k, v in (("oneshot", t1), ("first_ov", f_ov), ("total_ov", t_ov), ("first_serial", f_se), ("total_serial", t_se)):
                res[k].append(v * 1e3)
        print(f"rep {rep}: one-shot {t1 * 1e3:.1f} ms | overlap first {f_ov * 1e3:.1f} total {t_ov * 1e3:.1f} | serial first {f_se * 1e3:.1f} "
              f"total {t_se * 1e3:.1f} ms | {wav.shape[1]} samples", flush=True)
    out = dict(kind="latency", model=model, reps=reps, samples=int(wav.shape[1]), **{f"p50_{k}_ms": round(statistics.median(v), 2) for k, v in res.items()},
               raw_ms={k: [round(x, 2) for x in v] for k, v in res.items()})
    out["ratio_total_ov_to_oneshot"] = round(out["p50_total_ov_ms"] / out["p50_oneshot_ms"], 3)
    out["ratio_total_serial_to_oneshot"] = round(out["p50_total_serial_ms"] / out["p50_oneshot_ms"], 3)
    return out


@torch.inference_mode()
def loop(impl, steps):
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import T3TurboEngine
    eng = T3TurboEngine(synth.t3_turbo_state_dict(24, 1024, 0), "cuda")
    cond, ids = synth.t3_cond(prompt_len=375), synth.turbo_text_tokens(64)
    best = None
    for rep in range(4):  # rep 0: warm-up
        h = eng.generate(cond, [ids], max_gen_len=steps, ban_eos=True, ban_from=6561, async_mode=True, run_steps=1, **SAMP)
        st = h["st"]
        if impl == "py" and st["graph"] is None:
            eng._capture(st)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if impl == "c":
            eng._run_c_loop(st, steps, 0)
        else:
            for _ in range(steps):
                st["graph"].replay()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        assert int(st["n_generated"][0]) == steps + 1
        if rep:
            best = ms if best is None else min(best, ms)
        print(f"rep {rep}: {impl} {ms:.4f} ms / token", flush=True)
    return dict(kind="loop", impl=impl, steps=steps, ms_per_token=round(best, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=("latency", "loop"))
    ap.add_argument("--model", default="turbo", choices=("turbo", "nano"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--impl", default="c", choices=("c", "py"))
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    torch.manual_seed(0)
    out = latency(a.model, a.reps) if a.kind == "latency" else loop(a.impl, a.steps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
