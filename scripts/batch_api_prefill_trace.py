"""What a B = 8 T3 batch costs AHEAD of its first prefill GEMM (launches, and the time from call entry to that GEMM's start), from a kernel trace:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o trace -- python scripts/batch_api_prefill_trace.py run
    python scripts/batch_api_prefill_trace.py report OUT LABEL

`run` uses engine-level calls only, so the same file serves a checkout that predates cbx_prefill_embed / cbx_kv_prefix_paste_f32.  Two scenarios, each warmed
(prefixes cached where the tree can cache them), then 6 measured calls: `mixed` = 8 utterances of ragged text over 3 voices (a list of cond dicts), `single` = the
same texts over one voice (one dict).  Every measured call is preceded by a device synchronisation and ONE marker launch (cbx_reduce_max_f32; the T3 path never launches it): the device is idle, so the marker starts within a launch latency of call entry, and the start of
the first q | k | v GEMM of the prefill (the first GEMM after the marker that is 3072 columns = 48 column tiles wide) minus the marker's start is the time the host
needed to get there."""
import csv
import glob
import os
import sys


def run():
    import torch
    sys.path.insert(0, ".")
    from chatterbox_amd import ops, synth
    from chatterbox_amd.t3 import T3Engine
    dev = torch.device("cuda:0")
    eng = T3Engine(synth.t3_state_dict(30, 0), dev)
    voices = [synth.t3_cond(seed=s) for s in (11, 12, 13)]
    tt = [synth.text_tokens(n, seed=k + 1) for k, n in enumerate((64, 40, 64, 12, 55, 64, 30, 64))]
    u = synth.rand((8, 2), seed=3)
    samp = dict(temperature=0.8, cfg_weight=0.5, repetition_penalty=1.2, min_p=0.05, top_p=1.0)
    out = torch.zeros(1, device=dev)
    x = torch.ones(1, 64, device=dev)
    for conds in ([voices[k % 3] for k in range(8)], voices[0]):
        for i in range(9):  # 3 warm-up calls (unmarked), 6 measured
            torch.cuda.synchronize()
            if i >= 3:
                ops.reduce_max(x, out)
            eng.generate(conds, tt, max_new_tokens=2, uniforms=u, ban_eos=True, **samp)
    torch.cuda.synchronize()


def report(out_dir, label):
    path = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    gx = lambda r: int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
    wx = lambda r: int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1)
    marks = [i for i, r in enumerate(rows) if "reduce_max" in r["Kernel_Name"]]
    assert len(marks) == 12, f"{len(marks)} marker launches in {path}"
    res = {"mixed": [], "single": []}
    for j, i in enumerate(marks):  # the first six markers belong to the mixed-voice scenario
        for n, r in enumerate(rows[i + 1:]):
            if "gemm" in r["Kernel_Name"].lower() and gx(r) // max(1, wx(r)) == 48:
                res["mixed" if j < 6 else "single"].append((n, (int(r["Start_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e3,
                                                            sorted({k["Kernel_Name"].split("(")[0][-48:] for k in rows[i + 1:i + 1 + n]})))
                break
    for scen in ("mixed", "single"):
        v = res[scen]
        us = sorted(t for _, t, _ in v)
        print(f"{label} {scen}: launches ahead of the first prefill GEMM {[n for n, _, _ in v]}, call entry -> that GEMM's start (us) "
              f"{[round(t) for _, t, _ in v]}, median {us[len(us) // 2]:.0f}")
        print(f"{label} {scen}: kernels ahead of it: {v[-1][2]}")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else report(sys.argv[2], sys.argv[3])
