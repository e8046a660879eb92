"""Long-form join on the device against B separate copies: what a sub-batch of B chunks costs between the vocoder's last kernel and its audio on
the host.  A: B pinned device-to-host copies of the B waveforms (what synthesize_pipelined does for a job without `join`).  B: cbx_wave_edges_f32 + cbx_wave_join_f32
behind the waveforms, then ONE pinned copy of the piece and one of its records (a job with `join`).  Both end in the event wait the schedule does anyway; the two
forms alternate in one process, medians over --iters rounds after a warm-up.  Host trimming / joining of form A's waveforms is NOT included in A (it would add to it).

    python scripts/long_form_join_measure.py [--rows 8] [--seconds 10] [--iters 200]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    from chatterbox_amd import ops
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    n = int(a.seconds * 24000) // 480 * 480
    g = torch.Generator().manual_seed(0)
    big = (torch.rand(a.rows, n, generator=g) * 2 - 1) * 0.1
    big[:, : 480 * 20] *= 1e-3   # 0.4 s of hum in front of and behind the speech: something to trim
    big[:, -480 * 20:] *= 1e-3
    big = big.to(dev)
    rows = [big[r] for r in range(a.rows)]
    gaps = [3600] * a.rows
    pinned = lambda w: torch.empty(w.shape, dtype=w.dtype, pin_memory=True).copy_(w, non_blocking=True)

    def copies():
        host = [pinned(w) for w in rows]
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        return host

    def joined():
        p = ops.wave_join(rows, gaps, trim_db=40.0, pad_frames=2, fade=240, first=True, last=True)
        host = (pinned(p["out"]), pinned(p["rec"]))
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        return ops.piece_on_host(host[0], host[1], p["n"])

    for _ in range(20):
        copies()
        piece = joined()
    print(f"rows {a.rows} x {n} samples ({a.seconds} s each); kept {piece['edges'][0]}, piece of {piece['total']} samples")
    t = {"B pinned copies": [], "edges + join + 1 copy + record": []}
    for _ in range(a.iters):
        for name, fn in (("B pinned copies", copies), ("edges + join + 1 copy + record", joined)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e6)
    for name, v in t.items():
        q = statistics.quantiles(v, n=10)
        print(f"{name:32s}: median {statistics.median(v):8.1f} us   p10 {q[0]:8.1f}   p90 {q[-1]:8.1f}   ({len(v)} rounds, host clock from first enqueue to the event wait)")
    # the two launches alone, device events
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ks = []
    for _ in range(a.iters):
        e0.record()
        ops.wave_join(rows, gaps, trim_db=40.0, pad_frames=2, fade=240, first=True, last=True)
        e1.record()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1) * 1e3)
    print(f"{'the launches of ops.wave_join':32s}: median {statistics.median(ks):8.1f} us between device events (3 kernels, one small H2D-free call chain; reads {a.rows * n * 4 * 2 / 1e6:.1f} MB, writes {piece['total'] * 4 / 1e6:.1f} MB)")


if __name__ == "__main__":
    main()
