"""Shared by tests/test_wave_squeeze_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_wave_squeeze_kernels_gpu.py and tests/test_pauses_api_gpu.py: the
NumPy restatement of the pause control (include/cbx.h cbx_wave_squeeze_f32) -- frame energies in fp64 (wave_join_common.frame_ms, by import),
runs and cuts in Python ints, the seam in float32 with an exact fmaf --, the case table and the check of one ops.wave_squeeze call against the restatement.  Not a
test module.

Inputs are built from 480-sample frames of seven kinds: S uniform noise of amplitude >= 0.05 (speech), H uniform noise of amplitude 1e-4 (hum: silent at 40 dB),
Z exact zeros, N hum with one NaN sample (a NaN frame: not silent), and for the frame that lies ON the threshold three kinds of exact powers of two: P +-1.0
(m = 1), Q +-0.5 (m = 0.25 exactly), q +-0.5 with one sample +-0.75 (just above).  As in wave_join_common, the builder asserts on the restatement that no other
frame's mean square lies within a factor 1 +- 1e-6 of the threshold -- a condition on the INPUTS, not a tolerance: under it the kernel's fp64 sums (another order
of additions) give the same decisions, and everything downstream is exact."""
import math

import numpy as np
import torch

import wave_join_common as W

FRAME = W.FRAME
from chatterbox_amd.ops import WAVE_SQUEEZE_TILE as TILE  # frames per step of the plan kernel's scans: the long rows put their pauses around its multiples


def exact_db():
    """A db whose ratio 10^(-db / 10), evaluated as ops.wave_squeeze evaluates it, is exactly 0.25"""
    d = 10.0 * math.log10(4.0)
    cands = [d]
    lo = hi = d
    for _ in range(64):
        lo, hi = math.nextafter(lo, 0.0), math.nextafter(hi, 100.0)
        cands += [lo, hi]
    for c in cands:
        if 10.0 ** (-float(c) / 10.0) == 0.25:
            return c
    raise AssertionError("no db near 6.02 gives the ratio 0.25 exactly")


EXACT_DB = exact_db()


def fmaf(a, b, c):
    """float32 fma(a, b, c) with ONE rounding, for finite float32 arrays: the product is exact in fp64, TwoSum gives the error of the fp64 addition, the sum is
    forced to round-to-odd and then rounded to float32 (53 >= 24 + 2 bits: no double rounding)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def plan(row, K, ratio, check_margin=False):
    """-> the cuts [(a + h, b - t)] of one row, in frames"""
    n = len(row)
    if n == 0 or K == 0:
        return []
    m = W.frame_ms(row)
    ok = ~np.isnan(m)
    peak = max(0.0, float(m[ok].max())) if ok.any() else 0.0
    thr = peak * ratio
    if check_margin:
        pos = m[ok & (m > 0) & (m != thr)]
        assert not np.any((pos > thr * (1 - W.MARGIN)) & (pos < thr * (1 + W.MARGIN))), "a frame of the test input lies near the pause threshold"
    silent = ok & ((m <= thr) | (m == 0))
    live = np.nonzero(~silent)[0]
    if len(live) == 0:
        return []
    f0, f1 = int(live[0]), int(live[-1])
    cuts, f = [], f0 + 1
    while f < f1:
        if not silent[f]:
            f += 1
            continue
        a = f
        while silent[f]:  # (f1 is not silent: the run ends at or before it)
            f += 1
        b = f
        if b - a > K:
            cuts.append((a + K - K // 2, b - K // 2))
    return cuts


def squeeze(row, K, ratio, fade, edge=None, check_margin=False):
    """One row -> (y float32 (n,): the shortened row and its zero tail, stats [n', pauses cut, frames removed, n], the mapped edge entry or None)"""
    row = np.asarray(row, dtype=np.float32)
    n = len(row)
    cuts = plan(row, K, ratio, check_margin)
    kept = np.ones(n, dtype=bool)
    for a, b in cuts:
        kept[FRAME * a: FRAME * b] = False
    cum = np.concatenate([[0], np.cumsum(kept)])  # map(p), p in [0, n]
    n_new = int(cum[n])
    y = np.zeros(n, dtype=np.float32)
    y[:n_new] = row[kept]
    if fade:
        rp = W.ramp(fade)
        for a, b in cuts:
            c0, c1, q = FRAME * a, FRAME * b, int(cum[FRAME * a])
            x0, x1 = row[c0 - fade: c0], row[c1 - fade: c1]
            y[q - fade: q] = fmaf(rp, x1 - x0, x0)
    frames = sum(b - a for a, b in cuts)
    assert n_new == n - FRAME * frames
    mapped = None
    if edge is not None:
        s = min(max(int(edge[0]), 0), n)
        e = min(max(int(edge[1]), s), n)
        mapped = (int(cum[s]), int(cum[e]))
    return y, [n_new, len(cuts), frames, n], mapped


def make_row(n, pattern, rng):
    """n samples whose frame f is of kind pattern[f % len(pattern)]"""
    row = np.zeros(n, dtype=np.float32)
    for k, f in enumerate(range(0, n, FRAME)):
        kind = pattern[k % len(pattern)]
        m = min(FRAME, n - f)
        if kind in "PQq":
            seg = np.where(np.arange(m) % 2 == 0, 1.0, -1.0) * (1.0 if kind == "P" else 0.5)
            if kind == "q":
                seg[m // 2] *= 1.5
        else:
            amp = {"S": float(rng.choice([0.05, 0.11, 0.3])), "H": 1e-4, "N": 1e-4, "Z": 0.0}[kind]
            seg = rng.uniform(-1.0, 1.0, m) * amp
            if kind == "N":
                seg[m // 3] = float("nan")
        row[f: f + m] = seg.astype(np.float32)
    return row


def long_pattern(variant, frames):
    """`frames` frames of speech with a pause at every multiple b of TILE: variant 0 ends AT b ([b - 5, b)), 1 starts AT b ([b, b + 6)), 2 straddles it
    ([b - 3, b + 4)).  Besides: variant 0 alternates live and silent frames over [2 T - 6, 2 T + 6) instead; variant 1 has one pause over two tile edges,
    [3 T - 10, 5 T + 7); variant 2 a pause that is a whole tile, [6 T, 7 T)."""
    p = ["S"] * frames
    for b in range(TILE, frames - 8, TILE):
        lo, hi = [(b - 5, b), (b, b + 6), (b - 3, b + 4)][variant]
        for f in range(lo, hi):
            p[f] = "HZ"[f % 2]
    if variant == 0:
        for f in range(2 * TILE - 6, 2 * TILE + 6):
            p[f] = "SH"[f % 2]
    if variant == 1:
        for f in range(3 * TILE - 10, 5 * TILE + 7):
            p[f] = "H"
    if variant == 2:
        for f in range(6 * TILE - 1, 7 * TILE + 1):
            p[f] = "S" if f in (6 * TILE - 1, 7 * TILE) else "Z"
    return "".join(p)


LONG_FRAMES = 2100
# rows: (length, frame pattern, keep, edge entry or None = {0, n}).  An edge entry may name "c0" / "c1" / "in" (the first cut's bounds, a position inside it).
SETS = {
    # exactly K: unchanged | K + 1: one frame goes | K odd (h = 3, t = 2) | K = 2 | leading and trailing silence of 10 frames stays
    "pauses": [(8 * FRAME, "SSHHHHSS", 4, None), (9 * FRAME, "SSHHHHHSS", 4, None), (11 * FRAME, "S" + "Z" * 9 + "S", 5, None),
               (8 * FRAME + 137, "S" + "H" * 6 + "SS", 2, None), (30 * FRAME, "H" * 10 + "SS" + "H" * 7 + "S" + "Z" * 10, 3, None)],
    # two pauses one live frame apart | all zeros | no silent frame | keep = 0 beside rows with cuts | a NaN sample splits the pause (K = 2: 3 + 3 frames)
    "mixed": [(17 * FRAME, "S" + "H" * 6 + "S" + "Z" * 8 + "S", 2, None), (7680, "Z", 2, None), (2879, "S", 2, None), (11 * FRAME, "S" + "H" * 9 + "S", 0, None),
              (9 * FRAME, "SHHHNHHHS", 2, None)],
    # the lengths 0, 137, 480, 2879 (a partial last frame behind a cut), 7680
    "lengths": [(0, "S", 2, None), (137, "S", 2, None), (480, "H", 2, None), (2879, "SHHHHS", 2, None), (7680, "SS" + "H" * 12 + "SS", 3, None)],
    # m_f == peak * ratio exactly (db = EXACT_DB: ratio 0.25): Q is silent, q is not
    "threshold": [(14 * FRAME, "P" + "Q" * 6 + "q" + "Q" * 5 + "P", 2, None)],
    # the edge table: positions at 0 and n, at c0 and c1, inside a removed frame and beyond n, below 0 and inside; a trimmed table; keep = 0
    "edges": [(12 * FRAME, "SS" + "H" * 8 + "SS", 2, (0, 12 * FRAME)), (12 * FRAME, "SS" + "H" * 8 + "SS", 2, ("c0", "c1")),
              (12 * FRAME, "SS" + "H" * 8 + "SS", 2, ("in", 13 * FRAME)), (12 * FRAME + 7, "SS" + "H" * 8 + "SSS", 3, (-5, "in")),
              (12 * FRAME, "HH" + "SS" + "H" * 6 + "SH", 2, (2 * FRAME - 3, 11 * FRAME + 1)), (12 * FRAME, "SS" + "H" * 8 + "SS", 0, (480, 5000))],
    "one": [(20 * FRAME + 1, "SS" + "Z" * 15 + "SSS", 7, None)],
    "one_empty": [(0, "S", 2, None)],
    "sixty_four": [((3 + r % 9) * FRAME + (r * 37) % FRAME, "S" + "HZ"[r % 2] * (r % 7) + "SS", 2 + r % 3 if r % 5 else 0, None) for r in range(64)],
    "long": [(LONG_FRAMES * FRAME + 137, long_pattern(0, LONG_FRAMES + 1), 2, None), (LONG_FRAMES * FRAME, long_pattern(1, LONG_FRAMES), 3, None),
             (LONG_FRAMES * FRAME + FRAME - 1, long_pattern(2, LONG_FRAMES + 1), 4, ("in", LONG_FRAMES * FRAME))],
}
# (set, fade, db)
CASES = [("pauses", 240, 40.0), ("pauses", 0, 40.0), ("pauses", 480, 40.0), ("mixed", 240, 40.0), ("mixed", 480, 40.0), ("lengths", 240, 40.0), ("lengths", 0, 40.0),
         ("threshold", 240, EXACT_DB), ("edges", 240, 40.0), ("edges", 0, 40.0), ("one", 480, 40.0), ("one_empty", 240, 40.0), ("sixty_four", 240, 40.0),
         ("long", 240, 40.0)]
CASE_IDS = [f"{name}-fade{fade}-db{db:.3g}" for name, fade, db in CASES]
_BUILT = {}


def ratio_of(db):
    return 10.0 ** (-float(db) / 10.0)


def rows_of(name, db=40.0):
    """-> [(row float32, keep, edge entry in ints or None)], built once per (set, db) and not changed afterwards"""
    if (name, db) not in _BUILT:
        rng = np.random.RandomState(len(name))
        out = []
        for n, pat, keep, edge in SETS[name]:
            row = make_row(n, pat, rng)
            if edge is not None:
                cuts = plan(row, keep if keep else 2, ratio_of(db))
                names = {"c0": FRAME * cuts[0][0], "c1": FRAME * cuts[0][1], "in": FRAME * cuts[0][0] + 700} if cuts else {}
                edge = tuple(names[e] if isinstance(e, str) else e for e in edge)
            row.setflags(write=False)
            out.append((row, keep, edge))
        _BUILT[(name, db)] = out
    return _BUILT[(name, db)]


def place(rows, dev, pad=5):
    """The rows as views of ONE 1-D tensor on dev filled with NaN: row r begins r % 4 floats past a 16-byte boundary.  -> (views, buffer, offsets)"""
    offs, pos = [], 8
    for r, row in enumerate(rows):
        pos = -(-pos // 4) * 4 + r % 4
        offs.append(pos)
        pos += len(row) + pad
    big = torch.full((pos + 8,), float("nan"))
    for off, row in zip(offs, rows):
        big[off: off + len(row)] = torch.from_numpy(np.array(row))
    big = big.to(dev)
    return [big[off: off + len(row)] for off, row in zip(offs, rows)], big, offs


def check_launch(ops, dev, name, fade, db, sync=lambda: None):
    """One ops.wave_squeeze call on the rows of SETS[name] against the restatement: samples BITWISE, stats and mapped edges as integers, y[n', n) zeros, nothing
    outside the rows written (the output buffer is pre-filled with NaN), the input unchanged.  Returns (got stats, host copy of the output buffer)."""
    assert ops.WAVE_SQUEEZE_TILE == TILE
    built = rows_of(name, db)
    rows, keeps = [b[0] for b in built], [b[1] for b in built]
    R, ratio = len(rows), ratio_of(db)
    want = [squeeze(row, keep, ratio, fade, edge if edge is not None else (0, len(row)), check_margin=True) for row, keep, edge in built]
    views, big, offs = place(rows, dev)
    before = big.clone()
    table = torch.tensor([list(edge) if edge is not None else [0, len(row)] for row, _, edge in built], dtype=torch.int32).to(dev)
    out = torch.full((big.numel(),), float("nan"), device=dev)
    got = ops.wave_squeeze(views, keeps, db=db, fade=fade, edges=table, out=out)
    sync()
    assert got["edges"] is table and got["n"] == [len(r) for r in rows] and [v.numel() for v in got["rows"]] == got["n"]
    assert all(v.data_ptr() - out.data_ptr() == 4 * o for v, o in zip(got["rows"], offs) if v.numel()), "row r of the result lies where row r of the input lies in its buffer"
    stats, mapped = got["stats"].cpu().tolist(), [tuple(e) for e in table.cpu().tolist()]
    print(f"{name}: stats {stats[:8]} edges {mapped[:8]}")
    assert stats == [w[1] for w in want], (stats, [w[1] for w in want])
    assert mapped == [w[2] for w in want], (mapped, [w[2] for w in want])
    host = out.cpu().numpy()
    touched = np.zeros(host.shape, dtype=bool)
    for r, (off, row) in enumerate(zip(offs, rows)):
        y, st, _ = want[r]
        g = host[off: off + len(row)]
        bad = np.nonzero(g.view(np.int32) != y.view(np.int32))[0]
        assert len(bad) == 0, f"row {r}: {len(bad)} of {len(row)} samples differ bitwise, first at {bad[:5]}: {g[bad[:5]]} vs {y[bad[:5]]}"
        assert not g[st[0]:].any(), "the tail [n', n) is zeros"
        touched[off: off + len(row)] = True
    assert np.isnan(host[~touched]).all(), "nothing outside the rows is written"
    assert torch.equal(big.view(torch.int32), before.view(torch.int32)), "the input is not written"
    return stats, host


def check_composition(ops, dev, name, trim_db, first, last, fade=240, db=40.0, join_fade=240, pad=2, sync=lambda: None):
    """ops.wave_join(squeeze=) -- edges on the ORIGINAL rows, squeeze (which maps the table), join over the shortened rows with the host-side lengths -- against the
    NumPy composition: the existing restatement of the join (wave_join_common.join) over the zero-tailed rows and the mapped table.  Bitwise; two calls agree."""
    built = rows_of(name, db)
    rows, keeps = [b[0] for b in built], [b[1] for b in built]
    R, ratio = len(rows), ratio_of(db)
    gaps = [(37 * (r + 1)) % 500 for r in range(R)]
    table = [W.edges(row, trim_db, pad, check_margin=True) for row in rows]
    sq = [squeeze(row, keep, ratio, fade, e, check_margin=True) for row, keep, e in zip(rows, keeps, table)]
    want, offs, total = W.join([s[0] for s in sq], [s[2] for s in sq], gaps, join_fade, first, last)
    views, big, _ = place(rows, dev)
    cap = sum(len(r) for r in rows) + sum(gaps)
    got = []
    for _ in range(2):
        out = torch.full((cap + 7,), float("nan"), device=dev)
        piece = ops.wave_join(views, gaps, trim_db=trim_db, pad_frames=pad, fade=join_fade, first=first, last=last, out=out, squeeze=dict(keep=keeps, db=db, fade=fade))
        sync()
        got.append((piece["edges"].cpu().tolist(), piece["layout"].cpu().tolist(), piece["pauses"].cpu().tolist(), out.cpu().numpy()))
    edges_g, layout_g, stats_g, host = got[0]
    assert [tuple(e) for e in edges_g] == [s[2] for s in sq], (edges_g, [s[2] for s in sq])
    assert layout_g == offs + [total] and stats_g == [s[1] for s in sq]
    bad = np.nonzero(host[:total].view(np.int32) != want.view(np.int32))[0]
    assert len(bad) == 0, f"{len(bad)} of {total} samples differ bitwise, first at {bad[:5]}"
    assert np.isnan(host[total:]).all(), "samples at or beyond `total` must not be written"
    assert got[1][:3] == got[0][:3] and (got[1][3].view(np.int32) == host.view(np.int32)).all(), "two launches give identical results"
    return total, sum(s[1][2] for s in sq)


def what_the_sets_cover():
    """Host arithmetic on the restatement alone: each case is what it claims."""
    st = lambda name, db=40.0, fade=240: [squeeze(row, keep, ratio_of(db), fade, edge)[1:] for row, keep, edge in rows_of(name, db)]
    frames = lambda name, db=40.0: [s[0][2] for s in st(name, db)]
    cuts = lambda name, db=40.0: [s[0][1] for s in st(name, db)]
    assert frames("pauses") == [0, 1, 4, 4, 4] and cuts("pauses") == [0, 1, 1, 1, 1], "exactly K stays, K + 1 loses one, K = 5 of 9, K = 2 of 6, K = 3 of 7 (10 + 10 at the ends stay)"
    assert plan(rows_of("pauses")[2][0], 5, 1e-4) == [(1 + 3, 10 - 2)], "K odd: h = 3, t = 2"
    assert frames("mixed") == [4 + 6, 0, 0, 0, 2] and cuts("mixed") == [2, 0, 0, 0, 2], "two pauses; zeros; no silence; keep 0; the NaN frame splits 7 into 3 + 3"
    unsplit = np.array(rows_of("mixed")[4][0])
    unsplit[np.isnan(unsplit)] = 0.0
    assert squeeze(unsplit, 2, 1e-4, 0)[1][1:3] == [1, 5], "without the NaN it is one pause of 7"
    assert frames("lengths") == [0, 0, 0, 2, 9] and [len(r[0]) for r in rows_of("lengths")] == [0, 137, 480, 2879, 7680]
    assert ratio_of(EXACT_DB) == 0.25
    m = W.frame_ms(rows_of("threshold", EXACT_DB)[0][0])
    assert m[0] == 1.0 and (m[1:7] == 0.25).all() and 0.25 < m[7] < 0.26 and (m[8:13] == 0.25).all(), "Q frames lie ON the threshold, q just above"
    assert frames("threshold", EXACT_DB) == [4 + 3] and cuts("threshold", EXACT_DB) == [2], "m_f == peak * ratio is silent"
    e = st("edges")
    c0, c1 = 3 * FRAME, 9 * FRAME  # pause [2, 10), K = 2: frames [3, 9) go
    assert [s[0][2] for s in e] == [6, 6, 6, 5, 4, 0]
    assert e[0][1] == (0, 6 * FRAME) and e[1][1] == (c0, c0) and e[2][1] == (c0, 6 * FRAME), "0 and n; c0 and c1 map to one point; inside a cut -> c0, beyond n -> n'"
    assert rows_of("edges")[2][2] == (c0 + 700, 13 * FRAME) and e[3][1][0] == 0 and e[5][1] == (480, 5000)
    assert e[4][1] == (2 * FRAME - 3, 11 * FRAME + 1 - 4 * FRAME), "a trimmed table keeps its offsets into kept frames"
    assert frames("one") == [8] and frames("one_empty") == [0]
    f64 = frames("sixty_four")
    assert len(f64) == 64 and sum(1 for f in f64 if f) >= 10 and all(f == 0 for r, f in enumerate(f64) if r % 5 == 0)
    lg = rows_of("long")
    assert all(len(r[0]) >= LONG_FRAMES * FRAME for r in lg) and LONG_FRAMES > 8 * TILE
    n_edges = len(range(TILE, LONG_FRAMES - 8, TILE))
    p0, p1, p2 = (plan(r[0], r[1], 1e-4) for r in lg)
    assert len(p0) == n_edges - 1 and all(b - a == 3 and (b + 1) % TILE == 0 for a, b in p0), "variant 0: every pause ends AT a tile edge; none among the alternating frames"
    assert (3 * TILE - 10 + 2, 5 * TILE + 7 - 1) in p1 and len(p1) == n_edges - 2 and all(a % TILE == 2 for a, b in p1 if b - a == 3), "variant 1: pauses start AT a tile edge; one spans two"
    assert (6 * TILE + 2, 7 * TILE - 2) in p2 and all(a < (a // TILE + 1) * TILE <= b + 2 for a, b in p2), "variant 2: every pause straddles a tile edge; one is a whole tile"
    assert len(p2) == n_edges - 1
