"""Reads a rocprofv3 kernel trace of bench.py (argv[1] = *_kernel_trace.csv) and prints, per CFM solve (the kernels only the CFM estimator launches --
plane GEMMs, plane attention, narrow LayerNorm, plane split, Euler update -- cut into solves at gaps of 5 ms without any of them): the solve's wall span,
the union and the sum of its kernels' durations, the queues they ran on, and the time two of those queues had a CFM kernel running at once (two chains:
profiles/r09_cfm_two_chains_*).  argv[2] (optional): how many of the last solves to print (default 4: the timed steps of --steps 4)."""
import csv
import json
import re
import sys
from collections import defaultdict

CFM = re.compile(r"gemm_pl|flash_attn_pl|layernorm_narrow|split_planes|cfm_euler")
key = lambda r, *names: next((r[n] for n in names if n in r), None)
ev = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        name = key(r, "Kernel_Name", "Name")
        if CFM.search(name):
            ev.append((int(key(r, "Start_Timestamp", "BeginNs")), int(key(r, "End_Timestamp", "EndNs")), key(r, "Queue_Id", "Queue_ID", "queue_id"),
                       key(r, "Stream_Id", "Stream_ID"), name))
ev.sort()
segs, cur, last_end = [], [], None
for x in ev:
    if cur and x[0] - last_end >= 5e6:
        segs.append(cur)
        cur = []
    cur.append(x)
    last_end = x[1] if len(cur) == 1 else max(last_end, x[1])
if cur:
    segs.append(cur)


def union(iv):
    tot, ce = 0, None
    for s, e in sorted(iv):
        if ce is None or s > ce:
            tot, ce = tot + e - s, e
        elif e > ce:
            tot, ce = tot + e - ce, e
    return tot


def both_busy(a, b):
    pts = sorted([(s, 1, 0) for s, e in a] + [(e, -1, 0) for s, e in a] + [(s, 1, 1) for s, e in b] + [(e, -1, 1) for s, e in b])
    c, tot, prev = [0, 0], 0, None
    for t, d, w in pts:
        if prev is not None and c[0] > 0 and c[1] > 0:
            tot += t - prev
        c[w] += d
        prev = t
    return tot


print(f"# {len(ev)} CFM kernel records in {len(segs)} solves", flush=True)
for seg in segs[-int(sys.argv[2]) if len(sys.argv) > 2 else -4:]:
    by = defaultdict(list)
    for s, e, q, st, n in seg:
        by[(q, st)].append((s, e))
    qs = sorted(by, key=lambda k: -len(by[k]))
    line = dict(kernels=len(seg), span_ms=round((max(e for _, e, *_ in seg) - seg[0][0]) / 1e6, 2), busy_union_ms=round(union([(s, e) for s, e, *_ in seg]) / 1e6, 2),
                kernel_sum_ms=round(sum(e - s for s, e, *_ in seg) / 1e6, 2), queues={f"queue {q} stream {st}": len(by[(q, st)]) for q, st in qs})
    if len(qs) >= 2:
        line["two_chains_busy_at_once_ms"] = round(both_busy(by[qs[0]], by[qs[1]]) / 1e6, 2)
    print(json.dumps(line), flush=True)
