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


# Row lengths on either side of the two block lengths of the shared block pass (wave_common.h): the 480-sample frame here, the 512-sample block of the voice
# trim (wave_ingest_common.check_trim_seams runs the same rows).  One call per triple; its first row is the one on the 16-byte grid (seam_rows), so it is not the empty one.
SEAMS = [(479, 0, 1), (480, 481, 511), (512, 513, 1025)]


def seam_rows(signals, dev):
    """The rows of one call as views of ONE NaN-filled buffer: row r begins r floats behind a 16-byte boundary, so row 0 takes the block pass's 16-byte loads
    and rows 1 and 2 its scalar loads, in the same launch."""
    offs, pos = [], 0
    for r, x in enumerate(signals):
        pos = -(-pos // 4) * 4 + r
        offs.append(pos)
        pos += len(x) + 1
    big = torch.full((pos + 4,), float("nan"))
    for o, x in zip(offs, signals):
        big[o: o + len(x)] = torch.from_numpy(x)
    big = big.to(dev)
    assert big.data_ptr() % 16 == 0 and [o % 4 for o in offs] == [0, 1, 2] and big.numel() < 4000
    return [big[o: o + len(x)] for o, x in zip(offs, signals)]


def check_seams(ops, dev, lengths, sync=lambda: None):
    """cbx_wave_edges_f32 on three rows of the lengths of one SEAMS entry: frames of hum, speech and zeros, so that the last, partial frame of a row decides its
    stop; the table equals the restatement's exactly, at both pads."""
    rng = np.random.RandomState(sum(lengths))
    rows = [make_row(n, "HSZ" if n > 2 * FRAME else "HS" if n % 2 else "SH", rng) for n in lengths]
    views = seam_rows(rows, dev)
    for pad in (0, 2):
        want = [edges(r, 40.0, pad, check_margin=True) for r in rows]
        got = ops.wave_edges(views, 40.0, pad_frames=pad)
        sync()
        print(f"seams {lengths} pad {pad}: edges {got.cpu().tolist()}")
        assert got.dtype == torch.int32 and [tuple(e) for e in got.cpu().tolist()] == want, (lengths, pad, got.cpu().tolist(), want)
    return want


# The entries that take rows as (row_off, row_len, R) and check them with the one helper of wave_common.h, which is handed the entry's name.
ROW_ENTRIES = ("cbx_wave_edges_f32", "cbx_wave_join_f32", "cbx_wave_squeeze_f32", "cbx_wave_pitch_f32", "cbx_wave_format_f32", "cbx_wave_loudness_f32",
               "cbx_wave_loudness_push_f32", "cbx_wave_gain_f32", "cbx_wave_limit_f32", "cbx_wave_trim_edges_f32")
ROW_REFUSALS = ("R0", "R65", "length", "offset")


def check_row_refusal(lib, ops, entry, case):
    """One bad row descriptor -- R = 0, R = 65, a negative length, a negative offset -- around otherwise good arguments of `entry`, all in host memory: -22, the
    shared message under the ENTRY's name (the whole text: no other check fired first), and not a byte of any output written."""
    import ctypes
    who = entry[len("cbx_"):].replace("_f32", "")
    N = 65
    f32 = lambda v, n=4096: np.full(n, v, np.float32)
    wav, out, gain, ramp, tail = f32(0.25, 2048), f32(7.0), f32(7.0, N), f32(1.0, 8), f32(7.0, 2 * N * 2400)
    ints, stats, ws, rec = np.full(1024, 7, np.int32), np.full(1024, 7.0), np.full(4096, 7.0), np.full(N * 64, 7.0)
    zeros, lens8, steps, nans = np.zeros(N, np.int32), np.full(N, 8, np.int32), np.ones(N), np.full(N, np.nan)
    long0, out_off = np.zeros(N, np.int64), 16 * np.arange(N, dtype=np.int64)
    off, n, R = np.array([0, 960] + [0] * (N - 2), np.int64), np.array([960, 960] + [0] * (N - 2), np.int32), 2
    if case == "R0":
        R, text = 0, f"{who}: R = 0 outside [1, 64]"
    elif case == "R65":
        R, text = 65, f"{who}: R = 65 outside [1, 64]"
    elif case == "length":
        n[1], text = -1, f"{who}: row 1 has length -1 at offset 960"
    else:
        off[1], text = -4, f"{who}: row 1 has length 960 at offset -4"
    p = lambda a: a.ctypes.data
    pf, tp, lf = ops.pitch_filter(), ops.true_peak_filter(), ops.loudness_filter()
    win, coef = ops.limit_window(ops.LIMIT_LOOK), np.ascontiguousarray(lf["coef"])
    rows = (p(wav), p(off), p(n))
    args = {
        "cbx_wave_edges_f32": (*rows, R, 1e-4, 2, p(ints), p(ws), ws.size, None),
        "cbx_wave_join_f32": (*rows, p(zeros), R, p(ints), p(ramp), 8, 1, 1, p(out), out.size, p(ints) + 2048, None),
        "cbx_wave_squeeze_f32": (*rows, p(zeros), R, 1e-4, p(ramp), 8, p(out), out.size, None, p(ints), p(ws), 8 * ws.size, None),
        "cbx_wave_pitch_f32": (*rows, p(steps), p(lens8), R, p(pf["tab"]), pf["Z"], pf["L"], p(out), p(out_off), out.size, None),
        "cbx_wave_format_f32": (*rows, R, 24000, 0, None, 1, 1, None, None, None, None, None, p(out), p(long0), out.size, None),
        "cbx_wave_loudness_f32": (*rows, R, p(coef), lf["hop"], p(nans), 1.0, p(stats), p(gain), p(ws), ws.size, None),
        "cbx_wave_loudness_push_f32": (*rows, p(long0), R, p(coef), lf["hop"], p(nans), 1.0, p(rec), 56, p(tail), p(tail) + 4 * N * 2400, p(stats), p(gain), p(ws),
                                       ws.size, None),
        "cbx_wave_gain_f32": (*rows, R, p(gain), None),
        "cbx_wave_limit_f32": (*rows, R, None, p(nans), p(tp["tab"]), tp["U"], tp["T"], p(win), ops.LIMIT_LOOK, p(out), p(long0), out.size, p(stats), p(ws), ws.size, None),
        "cbx_wave_trim_edges_f32": (*rows, R, 0.01, p(ints), p(ws), ws.size, None),
    }[entry]
    rc = getattr(lib, entry)(*args)
    assert rc == -22 and lib.cbx_last_error().decode() == text, (entry, case, rc, lib.cbx_last_error())
    assert all(bool((a == 7).all()) for a in (out, gain, tail, ints, stats, ws, rec)) and bool((wav == 0.25).all()), f"{entry}, {case}: a refusal writes nothing"


def what_the_sets_cover():
    """Host arithmetic on the restatement: the inputs are what the shapes were chosen for."""
    assert {n // FRAME for t in SEAMS for n in t} == {0, 1, 2} and {n % FRAME for t in SEAMS for n in t} >= {0, 1, 479} and {n % 512 for t in SEAMS for n in t} >= {0, 1, 511}
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
