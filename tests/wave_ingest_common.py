"""Shared by tests/test_wave_ingest_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_wave_ingest_kernels_gpu.py and tests/test_audio_in_api_gpu.py: the
oracle of the audio inputs (include/cbx.h cbx_wave_ingest, cbx_wave_trim_edges_f32) -- the NumPy decode and mixdown (frontend.decode_pcm, which
host mode itself uses: it is pinned here against the committed G.711 encode tables of tests/golden/g711_tables.npz and, in the host test, against load_wav),
scipy.signal.resample_poly in fp64 of the fp32 decoded-and-mixed signal, a direct fp64 restatement of the formula that also gives the bound's S_m, the input builder
and the checks of a launch against them.  Not a test module.

The bound, per element: |y - y64[m]| <= (T + 2) 2^-24 S_m + 2^-24 |y64[m]|, S_m = sum_j |h_j| |x_j| -- wave_format_common.py derives it (a T-term fp32 fma chain
over coefficients rounded to fp32); it is derived, not measured."""
import ctypes
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENCODINGS = ("u8", "s16", "s24", "s32", "f32", "mulaw", "alaw")
SAMPLE_BYTES = dict(u8=1, s16=2, s24=3, s32=4, f32=4, mulaw=1, alaw=1)
ALIGN = dict(u8=1, s16=2, s24=1, s32=4, f32=4, mulaw=1, alaw=1)     # what a row's first byte must be a multiple of
CHANNELS = (1, 2, 3, 8)
# (rate_in, rate_out): U = 1; D = 1; a small table; an LDS-staged table at U = 80; the largest T U in common use and the largest table (both read from global
# memory); no table at all (decode only)
PAIRS = ((48000, 16000), (8000, 24000), (24000, 16000), (44100, 24000), (44100, 16000), (11025, 16000), (16000, 16000))
IN_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)
# frames per row.  A: R = 5, every short length; B: R = 1, several workgroups per row at every pair (>= 4 x 256 outputs); b: its stand-in on the emulator
SETS = {"A": [1931, 0, 7, 479, 480], "B": [3101], "b": [1]}
EPS = 2.0 ** -24
_G711 = {}


def g711_tables():
    if not _G711:
        with np.load(os.path.join(HERE, "golden", "g711_tables.npz")) as z:
            _G711.update(mulaw=z["mulaw"], alaw=z["alaw"])
    return _G711


def decode(raw, enc, channels):
    """the decode and mixdown oracle: bytes -> mono float32"""
    from chatterbox_amd import frontend
    return frontend.decode_pcm(bytes(raw), enc, channels)


def check_g711_expansion_is_pinned():
    """table[decode(c) + 32768] == c for all 256 codes of both laws; the one exception is mu-law 0x7F (negative zero), which decodes to 0, whose code is 0xFF.
    The ranges are the Recommendation's: A-law +-32256, mu-law +-32124."""
    from chatterbox_amd import frontend
    codes = np.arange(256, dtype=np.uint8)
    for law, top in (("mulaw", 32124), ("alaw", 32256)):
        pcm = frontend.g711_expand(codes, law)
        assert pcm.shape == (256,) and int(pcm.max()) == top and int(pcm.min()) == -top, (law, pcm.min(), pcm.max())
        back = g711_tables()[law][pcm + 32768]
        odd = np.flatnonzero(back != codes).tolist()
        assert odd == ([0x7F] if law == "mulaw" else []), (law, odd)
    assert int(frontend.g711_expand([0x7F], "mulaw")[0]) == 0 and int(g711_tables()["mulaw"][32768]) == 0xFF


def ratio(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def out_len(n, rate_in, rate_out):
    U, D = ratio(rate_in, rate_out)
    return -(-n * U // D)


def taps(rate_in, rate_out):
    U, D = ratio(rate_in, rate_out)
    return 1 if U == D else -(-(20 * max(U, D) + 1) // U)


def scipy_design(rate_in, rate_out):
    """(U, D, hl, h): the filter resample_poly builds itself for rate_in -> rate_out"""
    from scipy.signal import firwin
    U, D = ratio(rate_in, rate_out)
    hl = 10 * max(U, D)
    return U, D, hl, U * firwin(2 * hl + 1, 1.0 / max(U, D), window=("kaiser", 5.0))


def restate(x, rate_in, rate_out, h=None):
    """The definition in fp64 -> (y, S), S_m = sum_j |h_j| |x_j|.  Equal rates: y = x, S = |x|."""
    x = np.asarray(x, np.float64)
    if rate_in == rate_out:
        return x.copy(), np.abs(x)
    U, D, hl, hs = scipy_design(rate_in, rate_out)
    h = hs if h is None else np.asarray(h, np.float64)
    n, T = len(x), -(-(2 * hl + 1) // U)
    M = -(-n * U // D)
    c = np.arange(M, dtype=np.int64) * D + hl
    p, kh = c % U, c // U
    y, S = np.zeros(M), np.zeros(M)
    for j in range(T):
        i, k = p + j * U, kh - j
        coef = np.where(i <= 2 * hl, h[np.minimum(i, 2 * hl)], 0.0)
        xv = np.where((k >= 0) & (k < n), x[np.clip(k, 0, max(n - 1, 0))] if n else 0.0, 0.0)
        y += coef * xv
        S += np.abs(coef) * np.abs(xv)
    return y, S


def oracle(x, rate_in, rate_out):
    """(y64, S): scipy.signal.resample_poly(x in fp64, U, D) of the fp32 mono signal x, and the bound's S_m"""
    from scipy.signal import resample_poly
    x = np.asarray(x, np.float64)
    y, S = restate(x, rate_in, rate_out)
    if rate_in == rate_out or len(x) == 0:
        return y, S
    U, D = ratio(rate_in, rate_out)
    y64 = resample_poly(x, U, D)
    assert y64.shape == y.shape, (y64.shape, y.shape)
    return y64, S


def check_bound(y, x, rate_in, rate_out, what=""):
    """the fp32 result y against the oracle of the fp32 mono input x, per element -> worst |err| / bound"""
    y64, S = oracle(x, rate_in, rate_out)
    y = np.asarray(y, np.float64)
    assert y.shape == y64.shape, f"{what}: {y.shape[0]} outputs, ceil(n U / D) = {y64.shape[0]}"
    if not len(y):
        return 0.0
    bound = (taps(rate_in, rate_out) + 2) * EPS * S + EPS * np.abs(y64)
    err = np.abs(y - y64)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: element {worst}: |y - y64| = {err[worst]:.3e} > {bound[worst]:.3e} (y {y[worst]!r}, y64 {y64[worst]!r})"
    return float(np.max(err / np.maximum(bound, 1e-300)))


# ----------------------------------------------------------------------------- inputs
def raw_row(enc, channels, frames, seed):
    """the bytes of one row: random samples, led by both extremes of the encoding (s16 -32768 / 32767, s32's, s24's, u8 0 / 255) and, for G.711, by all 256 codes"""
    rng = np.random.default_rng(seed)
    count = frames * channels
    if enc == "f32":
        return rng.uniform(-0.99, 0.99, count).astype("<f4").tobytes()
    if enc in ("u8", "mulaw", "alaw"):
        v = rng.integers(0, 256, count, dtype=np.uint8)
        lead = np.arange(256, dtype=np.uint8) if enc != "u8" else np.array([0, 255, 128, 127], np.uint8)
        v[: min(count, len(lead))] = lead[:count]
        return v.tobytes()
    if enc == "s16":
        v = rng.integers(-32768, 32768, count).astype("<i2")
        v[: min(count, 4)] = np.array([-32768, 32767, 0, -1], "<i2")[:count]
        return v.tobytes()
    if enc == "s32":
        v = rng.integers(-2 ** 31, 2 ** 31, count).astype("<i4")
        v[: min(count, 4)] = np.array([-2 ** 31, 2 ** 31 - 1, 0, -1], "<i4")[:count]
        return v.tobytes()
    assert enc == "s24"
    v = rng.integers(-2 ** 23, 2 ** 23, count).astype(np.int64)
    v[: min(count, 4)] = np.array([-2 ** 23, 2 ** 23 - 1, 0, -1])[:count]
    u = (v & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], 1).astype(np.uint8).tobytes()


ALIGNMENTS = ("aligned", 0, 5, 10, 15)   # with rows 0 .. 4 the shifts 0, 5, 10, 15 put a row at every multiple of the encoding's alignment mod 16


def build(name, enc, channels, dev, alignment, pad_byte):
    """-> (host rows [bytes], device views): the rows of SETS[name] as uint8 views of ONE allocation filled with `pad_byte` (0xFF: an f32 row's padding then reads
    as NaN whatever its alignment).  alignment "aligned": every row begins on a 16-byte boundary; an int s: row r begins (s + r) ALIGN[enc] mod 16 bytes behind one."""
    fb = channels * SAMPLE_BYTES[enc]
    rows = [raw_row(enc, channels, n, 100 + r) for r, n in enumerate(SETS[name])]
    offs, pos = [], 32
    for r, b in enumerate(rows):
        mis = 0 if alignment == "aligned" else ((alignment + r) * ALIGN[enc]) % 16
        pos = (pos + 15) // 16 * 16 + mis
        offs.append(pos)
        pos += len(b) + 16
    host = np.full(pos + 48, pad_byte, np.uint8)
    for o, b in zip(offs, rows):
        host[o: o + len(b)] = np.frombuffer(b, np.uint8)
    big = torch.from_numpy(host).to(dev)
    assert big.data_ptr() % 16 == 0
    views = [big[o: o + len(b)] for o, b in zip(offs, rows)]
    assert all(len(b) == n * fb for b, n in zip(rows, SETS[name]))
    return rows, views


def check_ingest(ops, dev, name, enc, rate_in, rate_out, alignments=ALIGNMENTS, channels=CHANNELS, sync=lambda: None):
    """One encoding at one pair of rates, every channel count: lengths, the decode-only pair bit for bit, the bound against the fp64 oracle of the decoded-and-mixed
    signal, and identical bits at every alignment of the rows and with different padding bytes around them (0xFF: NaN padding for f32)."""
    worst = 0.0
    for C in channels:
        first = None
        for al in alignments:
            for pad in (0xFF, 0x5A):
                rows, views = build(name, enc, C, dev, al, pad)
                outs = ops.wave_ingest(views, enc, C, rate_in, rate_out)
                sync()
                assert len(outs) == len(rows) and len({o.untyped_storage().data_ptr() for o in outs}) == 1, "R views of one packed buffer"
                got = [o.cpu().numpy() for o in outs]
                if first is None:
                    first = got
                    for r, raw in enumerate(rows):
                        x, y = decode(raw, enc, C), got[r]
                        assert x.dtype == np.float32 and x.shape == (SETS[name][r],)
                        assert y.dtype == np.float32 and y.shape == (out_len(len(x), rate_in, rate_out),), (name, enc, C, r, y.shape)
                        if rate_in == rate_out:
                            assert np.array_equal(y.view(np.uint32), x.view(np.uint32)), f"{enc} x {C}, row {r}: decode and mixdown are exact"
                        else:
                            worst = max(worst, check_bound(y, x, rate_in, rate_out, f"{name} {enc} x {C} {rate_in} -> {rate_out} row {r}"))
                else:
                    for r in range(len(rows)):
                        assert np.array_equal(got[r].view(np.uint32), first[r].view(np.uint32)), f"{enc} x {C} row {r}: alignment {al}, padding {pad:#x} changed the bits"
    return worst


def raw_args(base, offs, frames, enc, channels, tab, U, D, T, out, out_offs, stream, out_cap=None):
    """the argument list of cbx_wave_ingest and the ctypes arrays it points into (keep them alive)"""
    R = len(frames)
    keep = [(ctypes.c_long * R)(*offs), (ctypes.c_long * R)(*frames), (ctypes.c_long * R)(*out_offs)]
    a = ctypes.addressof
    return [base, a(keep[0]), a(keep[1]), R, enc, channels, tab, U, D, T, out.data_ptr(), a(keep[2]), out.numel() if out_cap is None else out_cap, stream], keep


def check_sentinels(ops, dev, enc, channels, rate_in, rate_out, sync=lambda: None):
    """an oversized, prefilled output is untouched outside the rows' spans, and the spans hold the wrapper's result"""
    rows, views = build("A", enc, channels, dev, 5, 0xFF)
    f = ops.resample_filter(rate_in, rate_out)
    cnt = [out_len(n, rate_in, rate_out) for n in SETS["A"]]
    offs, pos = [], 5
    for c in cnt:
        offs.append(pos)
        pos += c + 3
    out = torch.full((pos + 9,), 7.0, device=dev)
    base = views[0].untyped_storage().data_ptr()
    tab = ops._resample_table(rate_in, rate_out, dev)
    args, keep = raw_args(base, [v.data_ptr() - base if v.numel() else 0 for v in views], SETS["A"], ENCODINGS.index(enc), channels, tab.data_ptr() if f["hl"] else None,
                          f["U"], f["D"], f["T"], out, offs, ops._stream())
    assert ops.lib.cbx_wave_ingest(*args) == 0, ops.lib.cbx_last_error()
    ref = ops.wave_ingest(views, enc, channels, rate_in, rate_out)
    sync()
    o, mask = out.cpu(), torch.ones(out.numel(), dtype=torch.bool)
    for r, (a, c) in enumerate(zip(offs, cnt)):
        assert torch.equal(o[a: a + c], ref[r].cpu()), (enc, r)
        mask[a: a + c] = False
    assert bool((o[mask] == 7.0).all()), "the output buffer is untouched outside the rows"


def check_refusals(lib, ops, dev, stream, sync=lambda: None, run_good=True):
    """every refused descriptor returns -22 with the entry's name and writes nothing; then the good one runs and writes its rows only.  run_good=False: the refusals
    alone (the product library on host buffers: a refusal never gets as far as a launch)"""
    ri, ro = 24000, 16000
    f = ops.resample_filter(ri, ro)
    tab = torch.from_numpy(f["tab"]).to(dev)
    raw = torch.from_numpy(np.frombuffer(raw_row("s16", 2, 2 * 960, 3), np.uint8).copy()).to(dev)   # two rows of 960 stereo s16 frames, 3840 bytes each
    out = torch.full((1500,), 7.0, device=dev)
    good, keep = raw_args(raw.data_ptr(), [0, 3840], [960, 960], 1, 2, tab.data_ptr(), f["U"], f["D"], f["T"], out, [3, 700], stream)
    a = ctypes.addressof
    L = ctypes.c_long * 2
    neg_n, neg_off, odd_off, neg_out, over = L(960, -1), L(0, -4), L(0, 3841), L(-1, 700), L(3, 861)
    bad = [(0, None), (1, None), (2, None), (10, None), (11, None), (6, None), (3, 0), (3, -1), (3, 65), (2, a(neg_n)), (1, a(neg_off)), (1, a(odd_off)), (11, a(neg_out)),
           (11, a(over)), (4, 7), (4, -1), (5, 0), (5, 9), (7, 4), (7, 0), (8, 6), (8, 0), (9, f["T"] + 1), (9, f["T"] - 1), (12, 1279), (12, 0)]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.cbx_wave_ingest(*args) == -22 and b"wave_ingest" in lib.cbx_last_error(), (i, v)
    # a span over the cap (1 -> 100: D = 100, 255 D + T > 2048) and a table over the cap (U = 2000: 2000 x 21 floats), each with the T that belongs to it
    for U, D in ((1, 100), (2000, 1999)):
        args = list(good)
        args[7], args[8], args[9] = U, D, -(-(20 * max(U, D) + 1) // U)
        assert lib.cbx_wave_ingest(*args) == -22 and b"wave_ingest" in lib.cbx_last_error() and b"cap" in lib.cbx_last_error(), (U, D, lib.cbx_last_error())
    sync()
    assert bool((out == 7.0).all()), "a refused call launches nothing"
    if not run_good:
        return keep
    args = list(good)
    args[12] = 1340          # exactly out_off[1] + 640
    assert lib.cbx_wave_ingest(*args) == 0
    sync()
    ref = ops.wave_ingest([raw[:3840], raw[3840:]], "s16", 2, ri, ro)
    sync()
    o = out.cpu()
    assert torch.equal(o[3:643], ref[0].cpu()) and torch.equal(o[700:1340], ref[1].cpu())
    assert bool((o[:3] == 7.0).all()) and bool((o[643:700] == 7.0).all()) and bool((o[1340:] == 7.0).all()), "nothing is written outside the rows"
    return keep, (neg_n, neg_off, odd_off, neg_out, over)


def what_the_sets_cover():
    for ri, ro in PAIRS:
        assert out_len(SETS["B"][0], ri, ro) >= 4 * 256, (ri, ro)
    assert sorted(SETS["A"]) == [0, 7, 479, 480, 1931] and SETS["b"] == [1]
    for enc in ENCODINGS:
        assert {((s + r) * ALIGN[enc]) % 16 for s in ALIGNMENTS[1:] for r in range(5)} == set(range(0, 16, ALIGN[enc])), "every misalignment the encoding allows"
    assert [ratio(*p) for p in PAIRS[:2]] == [(1, 3), (3, 1)] and ratio(44100, 16000) == (160, 441) and ratio(11025, 16000) == (640, 441) and ratio(16000, 16000) == (1, 1)


# ----------------------------------------------------------------------------- trim
TRIM_DB = 20.0
TRIM_CASES = ("bursts", "silent", "loud", "short")
from wave_join_common import SEAMS as TRIM_SEAMS  # noqa: E402  (the lengths on either side of both block lengths of the shared block pass)


def trim_case(kind):
    """bursts: 0.4 s of near-silence (-80 dB), speech-like bursts of 30 .. 90 ms with pauses, near-silence again; silent: all zeros; loud: noise throughout; short:
    shorter than one frame"""
    rng = np.random.default_rng(11)
    if kind == "silent":
        return np.zeros(9000, np.float32)
    if kind == "loud":
        return rng.uniform(-0.5, 0.5, 9001).astype(np.float32)
    if kind == "short":
        return rng.uniform(-0.5, 0.5, 1500).astype(np.float32)
    assert kind == "bursts"
    n = 30000
    env = np.full(n, 1e-4)
    pos = 6400
    while pos < n - 8000:
        k = int(rng.integers(480, 1440))
        env[pos: pos + k] = rng.uniform(0.2, 0.9)
        pos += k + int(rng.integers(200, 1200))
    return (env * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def trim_margin_db(y, top_db=TRIM_DB):
    """how far every frame's level (frontend.trim_silence's own dB values) is from the threshold: the smallest distance"""
    y = np.asarray(y, np.float32)
    yp = np.pad(y, (1024, 1024))
    nf = 1 + (len(yp) - 2048) // 512
    idx = np.arange(2048)[None, :] + 512 * np.arange(nf)[:, None]
    rms = np.sqrt(np.mean(yp[idx].astype(np.float64) ** 2, axis=1))
    db = 20.0 * np.log10(np.maximum(rms, 1e-10)) - 20.0 * np.log10(max(rms.max(), 1e-10))
    return float(np.abs(db + top_db).min())


def check_trim_rule(kind):
    """the device rule restated in NumPy (frontend.trim_edges_rule) keeps what frontend.trim_silence keeps, on an input every frame of which is at least 0.01 dB from
    the threshold -> (y, (start, stop))"""
    from chatterbox_amd import frontend
    y = trim_case(kind)
    assert trim_margin_db(y) >= 0.01, kind
    start, stop = frontend.trim_edges_rule(y, TRIM_DB)
    kept = frontend.trim_silence(y, TRIM_DB)
    assert len(kept) == stop - start and np.array_equal(kept, y[start:stop]), (kind, start, stop, len(kept))
    if kind == "bursts":
        assert 0 < start and stop < len(y), "the silent head and tail go"
    else:
        assert (start, stop) == (0, len(y)), "silence throughout, noise throughout and less than a frame are kept whole (librosa's rule)"
    return y, (start, stop)


def check_trim_seams(ops, dev, lengths, sync=lambda: None):
    """cbx_wave_trim_edges_f32 on three rows of the lengths of one wave_join_common.SEAMS entry -- either side of the 480-sample frame of the join and of the
    512-sample block here --, rows 1 and 2 off the 16-byte grid: blocks of loud and of faint noise (74 dB apart, every frame at least 0.01 dB from the
    threshold), the edges are the host rule's exactly."""
    import wave_join_common as J
    from chatterbox_amd import frontend
    rng = np.random.default_rng(sum(lengths))
    rows = []
    for r, n in enumerate(lengths):
        amp = np.where((np.arange(n) // 512 + r) % 2 == 0, 0.5, 1e-4)
        rows.append((amp * rng.uniform(-1.0, 1.0, n)).astype(np.float32))
        assert n == 0 or trim_margin_db(rows[-1]) >= 0.01, (lengths, r)
    want = [list(frontend.trim_edges_rule(y, TRIM_DB)) for y in rows]
    got = ops.wave_trim_edges(J.seam_rows(rows, dev), TRIM_DB)
    sync()
    print(f"trim seams {lengths}: edges {got.cpu().tolist()}")
    assert got.dtype == torch.int32 and got.cpu().tolist() == want, (lengths, got.cpu().tolist(), want)
    return want


def check_trim(ops, dev, sync=lambda: None):
    """the four cases as rows of ONE launch, at two alignments: the device's edges are the host rule's exactly"""
    cases = [check_trim_rule(k) for k in TRIM_CASES]
    for shift in (0, 1):
        ld = max(len(y) for y, _ in cases) + 8
        big = torch.full((len(cases), ld), float("nan"), device=dev)
        views = []
        for r, (y, _) in enumerate(cases):
            sh = (r + shift) % 4 if shift else 0
            big[r, sh: sh + len(y)] = torch.from_numpy(y).to(dev)
            views.append(big[r, sh: sh + len(y)])
        edges = ops.wave_trim_edges(views, TRIM_DB)
        sync()
        assert edges.dtype == torch.int32 and edges.shape == (len(cases), 2)
        assert edges.cpu().tolist() == [list(e) for _, e in cases], (shift, edges.cpu().tolist())
