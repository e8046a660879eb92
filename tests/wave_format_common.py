"""Shared by tests/test_wave_format_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_wave_format_kernels_gpu.py and tests/test_wave_format_api_gpu.py:
the oracle of the output formats (include/cbx.h cbx_wave_format_f32) -- scipy.signal.resample_poly in fp64, a direct fp64 restatement of the
formula that also gives the bound's S_m = sum_j |h_j| |x_j|, the NumPy quantisation and the G.711 tables of tests/golden/g711_tables.npz --, the input builder and
the checks of a launch against them.  Not a test module.

The bound of check (a), per element: |y - y64[m]| <= (T + 2) 2^-24 S_m + 2^-24 |y64[m]|.  A T-term fp32 fma chain over coefficients rounded to fp32 errs by at most
2^-24 |h_j x_j| per coefficient and 2^-24 |partial sum| <= 2^-24 S_m per fma, (T + 1) 2^-24 S_m to first order; one more unit covers the second-order terms, and the
last term is the rounding of the comparison's own fp32 value.  Derived, not measured; an off-by-one tap or phase misses it by orders of magnitude."""
import ctypes
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RESAMPLED = (8000, 16000, 22050, 32000, 44100, 48000)
RATES = RESAMPLED + (24000,)
ENCODINGS = ("f32", "s16", "mulaw", "alaw")
NP_DTYPES = dict(f32=np.float32, s16=np.int16, mulaw=np.uint8, alaw=np.uint8)
EPS = 2.0 ** -24
_G711 = {}


def g711_tables():
    """{"mulaw", "alaw"}: 65536-entry uint8 tables, entry s + 32768 is the code of the int16 sample s"""
    if not _G711:
        with np.load(os.path.join(HERE, "golden", "g711_tables.npz")) as z:
            _G711.update(mulaw=z["mulaw"], alaw=z["alaw"])
    return _G711


def ratio(rate):
    import math
    g = math.gcd(rate, 24000)
    return rate // g, 24000 // g


def out_len(n, rate):
    U, D = ratio(rate)
    return -(-n * U // D)


def scipy_design(rate):
    """(U, D, hl, h): the filter resample_poly builds itself for 24000 -> rate"""
    from scipy.signal import firwin
    U, D = ratio(rate)
    hl = 10 * max(U, D)
    return U, D, hl, U * firwin(2 * hl + 1, 1.0 / max(U, D), window=("kaiser", 5.0))


def restate(x, rate, h=None):
    """The definition, in fp64: y[m] = sum_j h[p + j U] x[k_hi - j] with c = m D + hl, p = c mod U, k_hi = c div U, m < ceil(n U / D); -> (y, S), S_m = sum_j |h_j| |x_j|.
    24000: y = x, S = |x|."""
    x = np.asarray(x, np.float64)
    if rate == 24000:
        return x.copy(), np.abs(x)
    U, D, hl, hs = scipy_design(rate)
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


def oracle(x, rate):
    """(y64, S): scipy.signal.resample_poly(x in fp64, U, D) and the bound's S_m"""
    from scipy.signal import resample_poly
    x = np.asarray(x, np.float64)
    y, S = restate(x, rate)
    if rate == 24000 or len(x) == 0:
        return y, S
    U, D = ratio(rate)
    y64 = resample_poly(x, U, D)
    assert y64.shape == y.shape, (y64.shape, y.shape)
    return y64, S


def taps(rate):
    U, D = ratio(rate)
    return 1 if U == D else -(-(20 * max(U, D) + 1) // U)


def check_bound(y, x, rate, what=""):
    """check (a): the fp32 result against the oracle, per element"""
    y64, S = oracle(x, rate)
    y = np.asarray(y, np.float64)
    assert y.shape == y64.shape, f"{what}: {y.shape[0]} outputs, ceil(n U / D) = {y64.shape[0]}"
    if not len(y):
        return 0.0
    bound = (taps(rate) + 2) * EPS * S + EPS * np.abs(y64)
    err = np.abs(y - y64)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: element {worst}: |y - y64| = {err[worst]:.3e} > {bound[worst]:.3e} (y {y[worst]!r}, y64 {y64[worst]!r})"
    return float(np.max(err / np.maximum(bound, 1e-300)))


def quantise(y32, encoding):
    """The store of an encoding, in NumPy, from the fp32 values: s16 = clamp(rint(y * 32768), -32768, 32767) (ties to even, NaN -> 0); mulaw / alaw = the table's
    code of that s16"""
    y32 = np.asarray(y32, np.float32)
    if encoding == "f32":
        return y32
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(y32 * np.float32(32768.0))
    s = np.clip(np.where(np.isnan(v), np.float32(0.0), v), -32768.0, 32767.0).astype(np.int16)
    return s if encoding == "s16" else g711_tables()[encoding][s.astype(np.int32) + 32768]


# ----------------------------------------------------------------------------- inputs
def signal(kind, n, seed):
    """uniform in +-0.99; a full-scale square wave of period 38 (the filter overshoots it: s16 must clip); zeros"""
    if kind == "uniform":
        return np.random.default_rng(seed).uniform(-0.99, 0.99, n).astype(np.float32)
    if kind == "square":
        return np.where((np.arange(n) // 19) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if kind == "mixed":  # uniform, then the square wave
        return np.concatenate([signal("uniform", n // 2, seed), signal("square", n - n // 2, seed)])
    assert kind == "zeros"
    return np.zeros(n, np.float32)


# name -> [(length, kind)]; A: R = 5, every short length and every input kind; B: R = 1, several workgroups per row; b: its stand-in on the emulator
SETS = {"A": [(1931, "uniform"), (0, "zeros"), (7, "uniform"), (479, "square"), (480, "zeros")], "B": [(70000, "mixed")], "b": [(1, "uniform")], "C": [(4097, "mixed")]}


def build(name, dev, aligned):
    """-> (host rows [np.float32], device views): the rows of SETS[name] as views of ONE padded (R, ld) tensor whose padding holds NaN.  aligned: every row begins
    on a 16-byte boundary of the allocation (torch allocations are at least that aligned); else row r begins r mod 3 + 1 floats behind one, so the set holds every
    4-byte misalignment."""
    spec = SETS[name]
    R, nmax = len(spec), max(n for n, _ in spec)
    ld = (nmax + 8 + 3) // 4 * 4
    host = np.full((R, ld), np.nan, np.float32)
    rows, shifts = [], []
    for r, (n, kind) in enumerate(spec):
        sh = 0 if aligned else r % 3 + 1
        x = signal(kind, n, 100 + r)
        host[r, sh: sh + n] = x
        rows.append(x)
        shifts.append(sh)
    big = torch.from_numpy(host).to(dev)
    views = [big[r, sh: sh + n] for r, (sh, (n, _)) in enumerate(zip(shifts, spec))]
    assert big.data_ptr() % 16 == 0
    if not aligned:
        assert {(v.data_ptr() // 4) % 4 for v in views if v.numel()} >= ({1, 2, 3} if R >= 3 else {1})
    return rows, views


def check_one_shot(ops, dev, name, rate, aligned, sync=lambda: None):
    """checks (a), (b: lengths) and (c) of one set at one rate: the f32 launch against the oracle, every encoded launch against the NumPy quantisation of the f32
    launch's values"""
    rows, views = build(name, dev, aligned)
    got = {}
    for enc in ENCODINGS:
        outs = ops.wave_format(views, dict(sample_rate=rate, encoding=enc))
        sync()
        assert len(outs) == len(rows) and len({o.untyped_storage().data_ptr() for o in outs}) == 1, "R views of one packed buffer"
        got[enc] = [o.cpu().numpy() for o in outs]
    worst = 0.0
    for r, x in enumerate(rows):
        y = got["f32"][r]
        assert y.dtype == np.float32 and y.shape == (out_len(len(x), rate),), (name, rate, r, y.shape)
        worst = max(worst, check_bound(y, x, rate, f"{name} {rate} row {r}"))
        for enc in ENCODINGS[1:]:
            q = got[enc][r]
            assert q.dtype == NP_DTYPES[enc] and q.shape == y.shape and np.array_equal(q, quantise(y, enc)), (name, rate, r, enc)
        if rate == 24000:
            assert np.array_equal(y, x), "24000 -> 24000 is the identity"
    return worst, got


def what_the_sets_cover():
    """the shapes are what their comments claim: the square wave's overshoot clips at every resampled rate, and several workgroups serve a row of set B"""
    for rate in RESAMPLED:
        y, _ = restate(signal("square", 479, 0), rate)
        assert y.max() > 1.0 and y.min() < -1.0, rate
        assert out_len(70000, rate) > 4 * 256
    assert sorted(n for n, _ in SETS["A"]) == [0, 7, 479, 480, 1931]


# ----------------------------------------------------------------------------- identity-rate s16: ties and clip cases, constructed
def tie_cases():
    """fp32 inputs whose y * 32768 is a tie (k + 0.5: to even), sits at or beyond either clip edge, or is not a number"""
    k = np.array([0, 1, 2, 3, -1, -2, -3, 32766, -32768, 100, -101], np.float64)
    ties = (k + 0.5) / 32768.0
    edge = np.array([32767.0, 32767.4, 32767.5, 32768.0, 40000.0, -32768.0, -32768.5, -32769.0, -50000.0, 0.49999, -0.5]) / 32768.0
    x = np.concatenate([ties, edge, [np.nan, np.inf, -np.inf, 0.0, -0.0]]).astype(np.float32)
    expect = np.array([0, 2, 2, 4, 0, -2, -2, 32766, -32768, 100, -100, 32767, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768, 0, 0, 0, 32767, -32768, 0, 0],
                      np.int16)
    return x, expect


# ----------------------------------------------------------------------------- splits (check d)
# per split: the pieces of rows 0, 1 and 2 round by round (None: the row went final in an earlier round).  Row 2 is empty throughout; in split 0 row 1 goes final
# two rounds before the others; split 2 feeds pieces shorter than the history (H = 20 .. 60).
SPLITS = [
    ([1, 0, 7, 480, 3, 1440, 1], [300, 59, 0, 1000, 2, None, None], [0] * 7),
    ([960, 960, 11], [5, 5, 2000], [0, 0, 0]),
    ([1] * 45, [13] * 45, [0] * 45),
]


def check_split(ops, dev, k, rate, encoding, sync=lambda: None):
    """the concatenated pushes of WaveFormatStream == the one-shot ops.wave_format of the whole rows, torch.equal"""
    split = SPLITS[k]
    rounds = len(split[0])
    total = [sum(p for p in row if p) for row in split]
    last = [max(i for i, p in enumerate(row) if p is not None) for row in split]
    data = [signal("uniform" if r == 0 else "mixed", n, 7 + r) for r, n in enumerate(total)]
    fmt = dict(sample_rate=rate, encoding=encoding)
    big = torch.full((3, max(total) + 4), float("nan"), device=dev)
    for r in range(3):
        big[r, 1: 1 + total[r]] = torch.from_numpy(data[r]).to(dev)
    whole = ops.wave_format([big[r, 1: 1 + total[r]] for r in range(3)], fmt)
    st = ops.WaveFormatStream(3, fmt, dev)
    pos, got = [0, 0, 0], [[], [], []]
    for i in range(rounds):
        rows = []
        for r in range(3):
            p = split[r][i]
            rows.append(None if p is None else big[r, 1 + pos[r]: 1 + pos[r] + p])
            pos[r] += p or 0
        outs = st.push(rows, [i >= last[r] for r in range(3)])
        for r in range(3):
            got[r].append(outs[r].clone())
    sync()
    for r in range(3):
        cat = torch.cat(got[r])
        assert cat.dtype == whole[r].dtype and cat.shape == whole[r].shape == (out_len(total[r], rate),), (k, rate, r, cat.shape, whole[r].shape)
        assert torch.equal(cat, whole[r]), f"split {k}, rate {rate}, row {r}: first difference at {int((cat != whole[r]).nonzero()[0])}"
    return got


def check_large_positions(ops, dev, rate, sync=lambda: None):
    """positions past 2^31 and 2^32: the definition depends on (n0, m0) through c = m D + hl alone, so a continued launch at (n0 + K D, m0 + K U) must give, bit for
    bit, the outputs and the next history of the same launch at (n0, m0) -- K = 2^33 + 5 puts n0 and m0 past 2^33 at every rate (and below the entry's 2^48); a 32-bit index anywhere breaks it"""
    f, K = ops.wave_filter(rate), 2 ** 33 + 5
    x = torch.full((1504,), float("nan"), device=dev)
    x[1:1501] = torch.from_numpy(signal("uniform", 1500, 17)).to(dev)
    st = ops.WaveFormatStream(1, dict(sample_rate=rate, encoding="f32"), dev)
    st.push([x[1:701]], [False])
    n0, m0, hist = st.n0[0], st.m0[0], st.hist[st.cur]
    got = []
    for shift in (0, K):
        nxt = torch.full_like(hist, 7.0)
        a, b = n0 + shift * f["D"], m0 + shift * f["U"]
        assert shift == 0 or (2 ** 33 < a < 2 ** 48 and 2 ** 33 < b < 2 ** 48)
        packed, spans = ops._wave_format_launch([x[701:1501]], rate, 0, [a], [b], [True], hist, nxt)
        sync()
        got.append((packed[spans[0][0]: spans[0][0] + spans[0][1]].clone(), nxt))
    assert got[0][0].numel() == out_len(1500, rate) - m0 > 0
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and bool((got[0][1] != 7.0).any())


# ----------------------------------------------------------------------------- the raw entry (checks b and e)
def raw_args(base, offs, lens, rate, enc, tab, U, T, out, out_offs, stream, cont=None, hist=(None, None)):
    """the argument list of cbx_wave_format_f32 and the ctypes arrays it points into (keep them alive)"""
    R = len(lens)
    keep = [(ctypes.c_long * R)(*offs), (ctypes.c_int * R)(*lens), (ctypes.c_long * R)(*out_offs)]
    c = [None, None, None]
    if cont is not None:
        keep += [(ctypes.c_long * R)(*cont[0]), (ctypes.c_long * R)(*cont[1]), (ctypes.c_int * R)(*cont[2])]
        c = [ctypes.addressof(a) for a in keep[3:]]
    a = ctypes.addressof
    return [base, a(keep[0]), a(keep[1]), R, rate, enc, tab, U, T, *c, hist[0], hist[1], out.data_ptr(), a(keep[2]), out.numel(), stream], keep


def check_refusals(lib, ops, dev, stream, sync=lambda: None, run_good=True):
    """check (e): every refused descriptor returns -22 with the entry's name and writes nothing; then the good one runs, and writes its rows only (check b).
    run_good=False: the refusals alone (the product library on host buffers: a launch on them would fault, a refusal never gets that far)"""
    rate = 16000
    f = ops.wave_filter(rate)
    tab = torch.from_numpy(f["tab"]).to(dev)
    wav = torch.from_numpy(signal("uniform", 2 * 960, 3)).to(dev)
    out = torch.full((1500,), 7.0, device=dev)
    hist = [torch.zeros(2, f["H"], device=dev) for _ in range(2)]
    good, keep = raw_args(wav.data_ptr(), [0, 960], [960, 960], rate, 0, tab.data_ptr(), f["U"], f["T"], out, [3, 700], stream)
    a = ctypes.addressof
    neg_len, neg_off, neg_out, over = (ctypes.c_int * 2)(960, -1), (ctypes.c_long * 2)(0, -4), (ctypes.c_long * 2)(-1, 700), (ctypes.c_long * 2)(3, 861)
    zeros, ones, negl, fin = (ctypes.c_long * 2)(0, 0), (ctypes.c_long * 2)(0, 5), (ctypes.c_long * 2)(0, -5), (ctypes.c_int * 2)(1, 1)
    bad = [(0, None), (1, None), (2, None), (14, None), (15, None), (6, None), (3, 0), (3, -1), (3, 65), (2, a(neg_len)), (1, a(neg_off)), (15, a(neg_out)),
           (15, a(over)), (4, 24001), (4, 11025), (4, 0), (5, 4), (5, -1), (7, 3), (8, f["T"] + 1), (8, f["T"] - 1), (16, 1279), (16, 0)]
    cont_bad = [dict(n0=a(zeros), m0=None, fin=a(fin)), dict(n0=a(zeros), m0=a(zeros), fin=None), dict(n0=a(negl), m0=a(zeros), fin=a(fin)),
                dict(n0=a(zeros), m0=a(negl), fin=a(fin)), dict(n0=a(ones), m0=a(zeros), fin=a(fin)),                       # (continued without a history)
                dict(n0=a(ones), m0=a(zeros), fin=a(fin), hi=hist[0].data_ptr(), ho=hist[0].data_ptr())]                # (hist_out == hist_in)
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.cbx_wave_format_f32(*args) == -22 and b"wave_format" in lib.cbx_last_error(), (i, v)
    for c in cont_bad:
        args = list(good)
        args[9], args[10], args[11], args[12], args[13] = c["n0"], c["m0"], c["fin"], c.get("hi"), c.get("ho")
        assert lib.cbx_wave_format_f32(*args) == -22 and b"wave_format" in lib.cbx_last_error(), c
    sync()
    assert bool((out == 7.0).all()) and all(bool((h == 0).all()) for h in hist), "a refused call launches nothing"
    if not run_good:
        return keep
    args = list(good)
    args[16] = 1340          # exactly out_off[1] + 640
    assert lib.cbx_wave_format_f32(*args) == 0
    sync()
    ref = ops.wave_format([wav[:960], wav[960:]], dict(sample_rate=rate, encoding="f32"))
    sync()
    o = out.cpu()
    assert torch.equal(o[3:643], ref[0].cpu()) and torch.equal(o[700:1340], ref[1].cpu())
    assert bool((o[:3] == 7.0).all()) and bool((o[643:700] == 7.0).all()) and bool((o[1340:] == 7.0).all()), "nothing is written outside the rows"
    return keep, (neg_len, neg_off, neg_out, over, zeros, ones, negl, fin)


def check_sentinels(ops, dev, rate, encoding, sync=lambda: None):
    """check (b) through the wrapper's own launch path for an encoded store: an oversized, prefilled output is untouched outside the rows' spans"""
    from chatterbox_amd import _lib
    rows, views = build("A", dev, aligned=False)
    enc = ENCODINGS.index(encoding)
    f = ops.wave_filter(rate)
    tab = ops._wave_table(rate, dev)
    cnt = [out_len(len(x), rate) for x in rows]
    offs, pos = [], 5
    for c in cnt:
        offs.append(pos)
        pos += c + 3
    fill = {"f32": 7.0, "s16": 0x7777, "mulaw": 0x77, "alaw": 0x77}[encoding]
    out = torch.full((pos + 9,), fill, dtype={"f32": torch.float32, "s16": torch.int16}.get(encoding, torch.uint8), device=dev)
    base = views[0].untyped_storage().data_ptr()
    args, keep = raw_args(base, [(v.data_ptr() - base) // 4 if v.numel() else 0 for v in views], [len(x) for x in rows], rate, enc,
                          tab.data_ptr() if f["hl"] else None, f["U"], f["T"], out, offs, ops._stream())
    assert ops.lib.cbx_wave_format_f32(*args) == 0, ops.lib.cbx_last_error()
    ref = ops.wave_format(views, dict(sample_rate=rate, encoding=encoding))
    sync()
    o, mask = out.cpu(), torch.ones(out.numel(), dtype=torch.bool)
    for r, (a, c) in enumerate(zip(offs, cnt)):
        assert torch.equal(o[a: a + c], ref[r].cpu()), (rate, encoding, r)
        mask[a: a + c] = False
    assert bool((o[mask] == fill).all()), "the output buffer is untouched outside the rows"
