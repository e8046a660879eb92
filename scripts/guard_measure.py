"""The alignment guard's cost on the B = 8 token step (16 rows, synthetic 30-layer weights, 64 text tokens) at contexts 224 and 1200, one process on one box,
the variants ALTERNATING inside every repetition.

    python scripts/guard_measure.py [variants, default off,off_py,on] [repetitions, default 5] [steps per window, default 64]
        off      the unguarded step as generate() replays it: the stage-level C step (cbx_t3_decode_step), captured.  Uses nothing newer than measure_decode's
                 ingredients, so it also runs from a checkout of the parent commit (`... off`).
        off_py   the same launches sequenced by Python (c_step off), captured by torch: what a guarded request's step is built on.
        on       off_py plus the guard -- one cbx_guard_text_mass_f32 launch per layer the heads name (the default ALIGN_HEADS: layers 9, 12, 13, one head
                 each: 3 launches of 8 workgroups, the one-workgroup-per-(row, head) form) and one cbx_guard_update_f32 launch ahead of the sampler -- with
                 rules that never fire (tail = repeat = inf, token_run = 0; hold_eos on, so the ban column is written every step).
A window = `steps` replays of the captured step between two events, from a state reset to the context (which grows by one per step inside the window); EOS and
every id beyond the speech codebook are banned, so no row ever finishes.  Prints one JSON line per context."""
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from chatterbox_amd import synth  # noqa: E402
from chatterbox_amd.t3 import T3Engine  # noqa: E402

dev = torch.device("cuda:0")
variants = (sys.argv[1] if len(sys.argv) > 1 else "off,off_py,on").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 64
B, TEXT = 8, 64
INF = float("inf")

with torch.cuda.device(dev), torch.inference_mode():
    eng = T3Engine(synth.t3_state_dict(30, 0), dev)
    for ctx in (224, 1200):
        max_ctx = (ctx + steps + 2 + 63) // 64 * 64
        st = eng._get_state(B, max_ctx, steps + 2, 7)
        eng._prepare_tune()
        gen = torch.Generator(device=dev).manual_seed(20240229)
        for k in ("kc", "vc"):
            st[k].normal_(0.0, 0.5, generator=gen)
        st["uniforms"].uniform_(generator=gen)
        samp = torch.tensor([0.5, 0.8, 0.05, 1.0, 1.2, 0.0, 6562.0, 6561.0]).repeat(B, 1)
        ids = torch.tensor([(911 * b + 17) % 6561 for b in range(B)] * 2, dtype=torch.int64)

        def reset():
            for k in ("seen", "step", "done", "n_generated", "out_tokens"):
                st[k].zero_()
            st["samp_dev"].copy_(samp)
            st["next_ids"].copy_(ids)
            st["next_pos_ids"].fill_(1)
            st["positions"].fill_(ctx)
            st["ctx_lens"].fill_(ctx + 1)
            st["step"].fill_(1)
            if st.get("guard") is not None:
                for k in ("state", "sums", "trace"):
                    st["guard"][k].zero_()

        graphs, launches = {}, {}
        for v in variants:
            eng.c_step = v == "off"
            st["guard_on"] = None
            if v == "on":
                g = eng.check_guard(dict(tail=INF, repeat=INF, token_run=0))
                st["guard_on"] = eng._begin_guard(st, g, [TEXT] * B, samp.clone())
                launches[v] = sum(len(r) for r in st["guard_on"]["by_layer"].values()) + 1
            st.pop("cstep", None)
            reset()
            eng._decode_step(st)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                eng._decode_step(st)
            graphs[v] = (gr, st["guard_on"])
        ms = {v: [] for v in variants}
        for r in range(reps + 1):   # (repetition 0 warms every variant up)
            for v in variants:
                gr, st["guard_on"] = graphs[v]
                reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    gr.replay()
                e1.record()
                torch.cuda.synchronize()
                assert int(st["step"].min()) == steps + 1 and int(st["done"].sum()) == 0, "every row took every step"
                if r:
                    ms[v].append(round(e0.elapsed_time(e1) / steps, 5))
        med = {v: round(statistics.median(t), 5) for v, t in ms.items()}
        out = dict(ctx=ctx, B=B, steps=steps, ms_per_step=ms, median_ms=med, spread_ms={v: round(max(t) - min(t), 5) for v, t in ms.items()}, guard_launches=launches,
                   gpu=torch.cuda.get_device_name(0))
        if "on" in med and "off_py" in med:
            out["guard_us_per_step"] = round(1e3 * (med["on"] - med["off_py"]), 2)
        if "on" in med and "off" in med:
            out["on_over_off"] = round(med["on"] / med["off"], 4)
        print(json.dumps(out), flush=True)
        graphs.clear()
        eng.release_state(7)
