"""Shared by tests/test_wave_join_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_wave_join_kernels_gpu.py and tests/test_long_form_gpu.py: the NumPy
restatement of the long-form trim + join (include/cbx.h cbx_wave_edges_f32 / cbx_wave_join_f32) -- edges in fp64, layout in Python ints, join
in float32 --, the input builder and the check of one ops.wave_join call against the restatement.  Not a test module.

Inputs are built from three kinds of 480-sample frame: uniform noise of amplitude >= 0.05 ("S", speech), uniform noise of amplitude 1e-4 ("H", hum) and exact zeros
("Z").  The builder asserts, on the fp64 restatement, that no frame's mean square lies within a factor 1 +- 1e-6 of the threshold -- a condition on the INPUTS, not a
tolerance: under it the kernel's fp64 sums (another order of additions) must give the same integers, and everything downstream is exact."""
import math

import numpy as np
import torch

FRAME = 480
MARGIN = 1e-6


def ramp(fade):
    """(2 i + 1) / (2 fade) in fp64, rounded to float32"""
    return ((2.0 * np.arange(fade, dtype=np.float64) + 1.0) / (2.0 * fade)).astype(np.float32)


def frame_ms(row):
    row = np.asarray(row, dtype=np.float64)
    return np.array([np.mean(row[f: f + FRAME] ** 2) for f in range(0, len(row), FRAME)], dtype=np.float64)


def edges(row, trim_db, pad, check_margin=False):
    """(start, stop) of one row; trim_db None: (0, n)"""
    n = len(row)
    if trim_db is None:
        return 0, n
    if n == 0:
        return 0, 0
    m = frame_ms(row)
    thr = m.max() * 10.0 ** (-float(trim_db) / 10.0)
    if check_margin:
        pos = m[m > 0]
        assert not np.any((pos > thr * (1 - MARGIN)) & (pos < thr * (1 + MARGIN))), "a frame of the test input lies on the trim threshold"
    live = np.nonzero((m > thr) & (m > 0))[0]
    if len(live) == 0:
        return 0, 0
    return FRAME * max(0, int(live[0]) - pad), min(n, FRAME * (int(live[-1]) + 1 + pad))


def layout(ns, edge_table, gaps, last):
    """-> (offsets, total) in Python ints"""
    offs, off, R = [], 0, len(ns)
    for r, (a, b) in enumerate(edge_table):
        offs.append(off)
        L = b - a
        off += L + (gaps[r] if L > 0 and not (last and r == R - 1) else 0)
    return offs, off


def join(rows, edge_table, gaps, fade, first, last):
    """rows: float32 arrays -> (out float32 (total,), offsets, total)"""
    ns = [len(r) for r in rows]
    offs, total = layout(ns, edge_table, gaps, last)
    out = np.zeros(total, dtype=np.float32)
    rp = ramp(fade) if fade else None
    R = len(rows)
    for r, (a, b) in enumerate(edge_table):
        L = b - a
        seg = np.asarray(rows[r][a:b], dtype=np.float32).copy()
        F = min(fade, L // 2)
        if F and not (first and r == 0 and a == 0):
            seg[:F] = seg[:F] * rp[:F]
        if F and not (last and r == R - 1 and b == ns[r]):
            seg[L - F:] = seg[L - F:] * rp[:F][::-1]
        out[offs[r]: offs[r] + L] = seg
    return out, offs, total


def make_row(n, pattern, rng):
    """n samples whose frame f is of kind pattern[f % len(pattern)]: S speech (amplitude 0.05 .. 0.3), H hum (1e-4), Z zeros"""
    row = np.zeros(n, dtype=np.float32)
    for k, f in enumerate(range(0, n, FRAME)):
        kind = pattern[k % len(pattern)]
        amp = {"S": float(rng.choice([0.05, 0.11, 0.3])), "H": 1e-4, "Z": 0.0}[kind]
        m = min(FRAME, n - f)
        row[f: f + m] = (rng.uniform(-1.0, 1.0, m) * amp).astype(np.float32)
    return row


# (length, frame pattern) per row.  A: a trimmed row with a partial last frame, an empty row, a row of zeros, a row shorter than a frame, a one-frame row.
# B: 70 000 samples (several workgroups per row), a row whose live part is ONE frame (fade > L / 2), a row that needs no trim, a hum-only frame, zeros shorter than a frame.
SETS = {
    "A": [(2879, "ZHSSHH"), (0, "S"), (7680, "Z"), (137, "S"), (480, "S")],
    "B": [(70000, "ZZHH" + "S" * 4 + "H" + "SS" + "Z" + "S" * 128 + "HHZZZZ"),
          (7680, "HHHHHHHSHHHHHHHH"), (2879, "S"), (480, "H"), (137, "Z")],
    "one_long": [(70000, "ZH" + "S" * 20 + "H" + "S" * 120 + "HZZ")],
    "one_partial": [(2879, "HSSSSZ")],
    "one_empty": [(0, "S")],
}
GAPS = [3600, 0, 17, 1, 960]
# (pad, fade, trim_db, first, last, row stride a multiple of 4): both pads, the three fades, trimming on / off, the four first / last combinations, both access forms
CONFIGS = [(0, 0, 40.0, False, False, True), (2, 240, 40.0, True, True, False), (0, 1000, 40.0, True, False, True), (2, 1000, 40.0, False, True, False),
           (2, 240, None, True, True, True), (0, 1000, None, False, False, False)]
CASES = [(name, cfg) for name in SETS for cfg in CONFIGS]
CASE_IDS = [f"{name}-pad{c[0]}-fade{c[1]}-trim{c[2]}-first{int(c[3])}-last{int(c[4])}-{'vec' if c[5] else 'scalar'}" for name, c in CASES]


def build(name, aligned, dev, seed=0):
    """-> (rows as NumPy arrays, rows as views of ONE padded (R, L) tensor on dev whose padding holds NaN)"""
    rng = np.random.RandomState(seed)
    rows = [make_row(n, pat, rng) for n, pat in SETS[name]]
    L = max(4, -(-max(len(r) for r in rows) // 4) * 4) + (4 if aligned else 3)
    big = torch.full((len(rows), L), float("nan"))
    for r, row in enumerate(rows):
        big[r, : len(row)] = torch.from_numpy(row)
    big = big.to(dev)
    return rows, [big[r, : len(row)] for r, row in enumerate(rows)]


def check_launch(ops, dev, name, cfg, sync=lambda: None, extra=7):
    """One ops.wave_join call (edges + join, or join alone) on the rows of SETS[name] against the restatement: the edge table and the layout record equal as
    integers, out[:total] equal BITWISE, out[total:] (pre-filled with NaN) untouched.  Returns (edge table, total)."""
    pad, fade, trim_db, first, last, aligned = cfg
    rows, views = build(name, aligned, dev)
    R = len(rows)
    gaps = GAPS[:R]
    want_edges = [edges(r, trim_db, pad, check_margin=True) for r in rows]
    want, offs, total = join(rows, want_edges, gaps, fade, first, last)
    cap = sum(len(r) for r in rows) + sum(gaps)
    out = torch.full((cap + extra,), float("nan"), device=dev)
    piece = ops.wave_join(views, gaps, trim_db=trim_db, pad_frames=pad, fade=fade, first=first, last=last, out=out)
    sync()
    assert piece["out"].data_ptr() == out.data_ptr() and piece["n"] == [len(r) for r in rows]
    got_edges = [tuple(e) for e in piece["edges"].cpu().tolist()]
    print(f"{name}: edges {got_edges} offsets {piece['layout'].cpu().tolist()}")
    assert got_edges == want_edges, (got_edges, want_edges)
    assert piece["layout"].cpu().tolist() == offs + [total], (piece["layout"].cpu().tolist(), offs, total)
    host = out.cpu().numpy()
    bad = np.nonzero(host[:total].view(np.int32) != want.view(np.int32))[0]
    assert len(bad) == 0, f"{len(bad)} of {total} samples differ bitwise, first at {bad[:5]}: {host[bad[:5]]} vs {want[bad[:5]]}"
    assert np.isnan(host[total:]).all(), "samples at or beyond `total` must not be written"
    return want_edges, total


def what_the_sets_cover():
    """Host arithmetic on the restatement: the inputs are what the shapes were chosen for."""
    rng = np.random.RandomState(0)
    a = [make_row(n, p, rng) for n, p in SETS["A"]]
    assert edges(a[0], 40.0, 0) == (960, 1920) and edges(a[0], 40.0, 2) == (0, 2879) and edges(a[1], 40.0, 2) == (0, 0) and edges(a[2], 40.0, 2) == (0, 0)
    assert edges(a[3], 40.0, 0) == (0, 137) and edges(a[4], 40.0, 2) == (0, 480)
    rng = np.random.RandomState(0)
    b = [make_row(n, p, rng) for n, p in SETS["B"]]
    e0 = edges(b[0], 40.0, 0)
    assert e0[0] == 4 * FRAME and 0 < e0[1] < 70000 and e0[1] % FRAME == 0
    assert edges(b[1], 40.0, 0) == (7 * FRAME, 8 * FRAME), "one live frame: L = 480, so fade 1000 is cut to 240"
    assert edges(b[2], 40.0, 0) == (0, 2879) and edges(b[3], 40.0, 0) == (0, 480) and edges(b[4], 40.0, 0) == (0, 0)
    assert math.ceil(70000 / 4096) > 1, "several join workgroups per row"
