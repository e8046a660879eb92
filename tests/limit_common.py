"""Shared by tests/test_limit_host.py (SIMT emulator, CPU tensors), tests/test_limit_kernels_gpu.py and tests/test_limit_api_gpu.py: the oracle of the true-peak
limiter (include/cbx.h cbx_wave_limit_f32) -- steps 1 - 7 in NumPy fp64 over scipy.signal.firwin's taps as the fp32 table holds them, written
independently of ops --, its float32 restatement, the signal builders, the cases and the check of a launch against the oracle.  Not a test module.

Tolerances.  The float32 restatement (oracle(dtype=np.float32): the same tap order, a rounded multiply and a rounded add per tap, fp32 accumulation) deviates from
the fp64 oracle over every committed case (measure(): all of cases(), H = 3, 120 and 480) by at most
    |dg| = 1.032e-6 and |dout| / max|u| = 8.46e-7 -- measured by measure() on the CPU; REF_G / REF_OUT are these rounded up, and test_limit_host.py asserts that
    measure() stays within them --,
and the kernel is allowed FACTOR = 4 times that: an fma differs from a multiply-add by at most one rounding per tap, and the kernel's order is the restatement's.
TOL_G = 4.16e-6, TOL_OUT = 3.4e-6 (relative to max|u| of the row).  The true peak in the stats is an fp32 sum of 21 taps: within TOL_OUT of the oracle's, relative.
The ceiling of the output: the oracle's own meter reads the kernel's output; it may exceed C only by what the ORACLE's output exceeds it on the same case (gain
modulation between the samples makes TP(u g) slightly larger than max(g m)), plus TOL_OUT max|u|; asserted only where the oracle alone stays within C (1 + 1e-5)
(the case asserts that precondition itself; cases with H < 120 are checked against the oracle only)."""
import numpy as np
import torch

import loudness_common as L

FS = 24000
U, HL, T = 4, 40, 21
LOOK = 120
FACTOR = 4.0
REF_G, REF_OUT = 1.04e-6, 8.5e-7          # the float32 restatement against the fp64 oracle (measure())
TOL_G, TOL_OUT = FACTOR * REF_G, FACTOR * REF_OUT
CEIL_PRE = 1e-5                          # the oracle alone stays within C (1 + CEIL_PRE) wherever the ceiling of the kernel's output is asserted
DB09 = 20.0 * np.log10(0.9)              # the ceiling 0.9 in dBTP


def linear(db):
    return None if db is None else 10.0 ** (float(db) / 20.0)


def taps(U=U):
    """h = U firwin(2 hl + 1, 1 / U, kaiser 5.0), hl = 10 U, as the fp32 phase table holds it, (U, T) float64: row p = h[p + j U], zero past 2 hl (T = 21 for every U)"""
    from scipy.signal import firwin
    h = U * firwin(20 * U + 1, 1.0 / U, window=("kaiser", 5.0))
    pad = np.zeros(U * T)
    pad[: 20 * U + 1] = h
    return pad.reshape(T, U).T.astype(np.float32).astype(np.float64)


def window(H):
    k = np.arange(-H, H + 1, dtype=np.float64)
    w = 0.5 * (1.0 + np.cos(np.pi * k / (H + 1)))
    return (w / w.sum()).astype(np.float32).astype(np.float64)


def _peaks(u, dtype, U=U):
    """m[i] = max(|u[i]|, |y[U i .. U i + U - 1]|) (NaN where one is), y by the taps in ascending order from 0"""
    n, tab = len(u), taps(U).astype(dtype)
    pad = np.zeros(n + T + 10, dtype)
    pad[T: T + n] = u                      # u[i] at pad[i + T]
    m = np.abs(u)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(U):
            acc = np.zeros(n, dtype)
            for j in range(T):
                acc = acc + tab[p, j] * pad[T + 10 - j: T + 10 - j + n]
            m = np.maximum(m, np.abs(acc))  # (np.maximum propagates a NaN)
    return m


def oracle(x, db, gamma=1.0, H=LOOK, dtype=np.float64, U=U):
    """Steps 1 - 7 on one row -> dict(u (float32), m, c, g, out, stats = [true peak, min g, samples with g < 1, samples with m > C]).  dtype = np.float32: the
    restatement in the kernel's precision."""
    from numpy.lib.stride_tricks import sliding_window_view
    u32 = np.asarray(x, np.float32) * np.float32(gamma)
    u, n = u32.astype(dtype), len(u32)
    C = dtype(np.float32(linear(db))) if db is not None and dtype is np.float32 else (np.nan if db is None else linear(db))
    if n == 0:
        z = np.zeros(0, dtype)
        return dict(u=u32, m=z, c=z, g=z, out=z, stats=[0.0, 1.0, 0, 0], C=C)
    m = _peaks(u, dtype, U)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = np.isfinite(m) & (m > C)
        c = np.where(over, dtype(C) / np.where(over, m, 1), dtype(1))
    ext = np.ones(n + 4 * H, dtype)
    ext[2 * H: 2 * H + n] = c
    d = dtype(1) - sliding_window_view(ext, 2 * H + 1).min(axis=1)   # 1 - a[i], i = -H .. n + H - 1
    w = window(H).astype(dtype)
    s = np.zeros(n, dtype)
    for k in range(2 * H + 1):
        s = s + w[k] * d[k: k + n]
    g = np.minimum(dtype(1) - s, c)
    out = u * g
    with np.errstate(invalid="ignore"):
        n_over = int((m > C).sum())
    return dict(u=u32, m=m, c=c, g=g, out=out, stats=[float(m.max()), float(g.min()), int((g < 1).sum()), n_over], C=C)


def true_peak(x):
    """the fp64 oracle's meter over one row"""
    x = np.asarray(x, np.float64)
    return float(_peaks(x, np.float64).max()) if len(x) else 0.0


# ----------------------------------------------------------------------------- the signals
def bursts(n, seed):
    """loudness_common.bursts with the amplitude 0.9 added: every 1200 samples another amplitude"""
    rng = np.random.default_rng(seed)
    amp = np.repeat(rng.choice(L.AMPS + (0.9,), size=n // 1200 + 1), 1200)[:n]
    return (rng.standard_normal(n) * amp).astype(np.float32)


def spikes(n, at, level=2.0):
    """a quiet 997 Hz sine with single samples of `level` at the indices `at`"""
    x = L.sine(n, amp=0.05)
    for k, i in enumerate(at):
        x[i] = level if k % 2 == 0 else -level
    return x


def inter_sample(n=1276):
    """6 kHz at 45 degrees, amplitude 1: every sample is +-0.7071, the true peak is 1.0"""
    return np.sin(2.0 * np.pi * 6000.0 * np.arange(n) / FS + np.pi / 4.0).astype(np.float32)


GROUPS = ((0, 1, 3333), (11, 0, 2051), (240, 1276, 0), (241, 1023, 1024), (1025, 0, 11))   # every length, an empty row first, in the middle and last
N = 2051


def cases():
    """name -> dict(signals, db (per row; None: not limited), gamma (per row, or None: no gain vector), H).  Every case is R <= 3 rows of at most 3333 samples."""
    out = {}
    for g, lens in enumerate(GROUPS):
        out[f"lengths{g}"] = dict(signals=[bursts(n, 20 + n) for n in lens], db=[-1.0, -1.0, -1.0], gamma=[3.0, 3.0, 3.0], H=LOOK)
    out["peak_ends"] = dict(signals=[spikes(N, [0]), spikes(N, [N - 1]), spikes(N, [50, N - 51])], db=[DB09] * 3, gamma=None, H=LOOK)
    out["peak_tile_edge"] = dict(signals=[spikes(N, [1023]), spikes(N, [1024]), spikes(N, [1023, 1024])], db=[DB09] * 3, gamma=None, H=LOOK)
    out["peak_pairs"] = dict(signals=[spikes(N, [600, 600 + 2 * LOOK]), spikes(N, [600, 601 + 2 * LOOK]), spikes(N, [900, 900 + 2 * LOOK + 1, 1500])], db=[DB09] * 3,
                             gamma=None, H=LOOK)
    out["inter_sample"] = dict(signals=[inter_sample()], db=[DB09], gamma=None, H=LOOK)
    out["under"] = dict(signals=[L.sine(1276, amp=0.5), bursts(1025, 3) * np.float32(0.05)], db=[DB09, -1.0], gamma=[1.3, 1.0], H=LOOK)
    out["mixed"] = dict(signals=[bursts(N, 5), bursts(1276, 6), bursts(1025, 7)], db=[-1.0, None, -6.0], gamma=[3.0, 0.7, 3.0], H=LOOK)
    out["bursts_m1"] = dict(signals=[bursts(3333, 8)], db=[-1.0], gamma=[3.0], H=LOOK)
    out["bursts_m6"] = dict(signals=[bursts(3333, 8)], db=[-6.0], gamma=[3.0], H=LOOK)
    out["look3"] = dict(signals=[bursts(N, 9)], db=[-1.0], gamma=[3.0], H=3)
    out["look480"] = dict(signals=[bursts(N, 9)], db=[-1.0], gamma=[3.0], H=480)
    return out


def measure():
    """(max |dg|, max |dout| / max|u|) of the float32 restatement against the fp64 oracle over every row of cases()"""
    dg = dout = 0.0
    for name, c in cases().items():
        for r, x in enumerate(c["signals"]):
            if len(x) == 0:
                continue
            gam = 1.0 if c["gamma"] is None else c["gamma"][r]
            a, b = oracle(x, c["db"][r], gam, c["H"]), oracle(x, c["db"][r], gam, c["H"], np.float32)
            dg = max(dg, float(np.abs(a["g"] - b["g"]).max()))
            dout = max(dout, float(np.abs(a["out"] - b["out"]).max() / np.abs(a["u"]).max()))
    return dg, dout


# ----------------------------------------------------------------------------- a launch against the oracle
def check_row(name, r, x, db, gam, H, got, st, far=None):
    """the output `got` and the stats row `st` (None: the output alone) of a launch over x against the fp64 oracle; far (a bool mask): compare only there (a row with a NaN).  Returns the
    oracle's dict."""
    ref = oracle(x, db, gam, H)
    n = len(x)
    if n == 0:
        assert list(st) == [0.0, 1.0, 0.0, 0.0], f"{name} row {r}: an empty row has the stats {{0, 1, 0, 0}}, got {st}"
        return ref
    if st is None:  # (the caller has no stats of this row: a sub-batch of an API call)
        st = [ref["stats"][0], ref["stats"][1], float(int((ref["g"] < 1.0 - TOL_G).sum())), float(ref["stats"][3])]
    scale = max(float(np.nanmax(np.abs(ref["u"]))), 1e-30)   # (a silent row: every difference is 0)
    sel = np.ones(n, bool) if far is None else far
    err = float(np.abs(got.astype(np.float64) - ref["out"])[sel].max()) / scale
    print(f"{name} row {r}: n {n} H {H} C {ref['C']!r} max|u| {scale:.4g} |dout|/max|u| {err:.3g} (allowed {TOL_OUT:.3g}) stats {list(st)} oracle {ref['stats']}")
    assert err <= TOL_OUT, f"{name} row {r}: out deviates from the oracle by {err:.3g} max|u|, allowed {TOL_OUT:.3g}"
    if far is not None:
        assert np.isnan(st[0]), f"{name} row {r}: the true peak of a row with a NaN is NaN, got {st[0]}"
        return ref
    tp, gmin, n_g, n_m = ref["stats"]
    assert abs(st[0] - tp) <= TOL_OUT * scale, f"{name} row {r}: true peak {st[0]!r}, oracle {tp!r}"
    assert abs(st[1] - gmin) <= TOL_G, f"{name} row {r}: min g {st[1]!r}, oracle {gmin!r}"
    if db is None or not np.any(np.abs(ref["m"] - ref["C"]) <= TOL_OUT * scale):
        assert st[3] == n_m, f"{name} row {r}: {st[3]} samples over the ceiling, oracle {n_m}"
    else:
        print(f"{name} row {r}: an m lies within the tolerance of C: the count of samples over the ceiling is not compared")
    # g < 1 is decided for the samples whose oracle g is further than the tolerance from 1; a sample with 1 - TOL_G <= g < 1 in fp64 (the outermost taps of the
    # window over a barely limited neighbour) may round to 1 in fp32: those may count either way, and the test says how many there were
    sure, maybe = int((ref["g"] < 1.0 - TOL_G).sum()), int(((ref["g"] >= 1.0 - TOL_G) & (ref["g"] < 1.0)).sum())
    if maybe:
        print(f"{name} row {r}: {maybe} samples have 1 - {TOL_G:.2g} <= g < 1 in the oracle: the count of g < 1 is compared as {sure} <= count <= {sure + maybe}")
    assert sure <= st[2] <= sure + maybe, f"{name} row {r}: {st[2]} samples with g < 1, oracle {n_g} ({maybe} of them within the tolerance of 1)"
    if db is None or n_m == 0:
        assert np.array_equal(got, ref["u"], equal_nan=True), f"{name} row {r}: a row that is not limited, or lies under its ceiling, is bit for bit x * float32(gamma)"
        assert st[1] == 1.0 and st[2] == 0 and st[3] == 0
    if db is not None and H >= LOOK:
        C, tp_ref = linear(db), true_peak(ref["out"])
        assert tp_ref <= C * (1.0 + CEIL_PRE), f"{name} row {r}: the oracle's own output reads {tp_ref / C - 1:.3g} over C: the case does not separate the ceiling"
        tp_got = true_peak(got)
        print(f"{name} row {r}: true peak of the output {tp_got!r} (oracle's output {tp_ref!r}, C {C!r})")
        assert tp_got <= max(C, tp_ref) + TOL_OUT * scale, f"{name} row {r}: the output reads {tp_got!r} dBTP-linear over the ceiling {C!r}"
    return ref


def run_case(ops, name, case, mis, device="cpu", sync=lambda: None, use_gain=True):
    """One wave_limit over the case's rows as views of one NaN-padded buffer at misalignment `mis`, into rows of another NaN-padded buffer at misalignment
    mis + 1: against the oracle, the padding of `out` still NaN, `wav` unchanged.  Returns (outputs, stats) as host arrays."""
    sig = case["signals"]
    buf, rows, spans = L.padded_rows(sig, mis, device)
    obuf, orows, ospans = L.padded_rows([np.zeros(len(s), np.float32) for s in sig], mis + 1, device)
    before = buf.cpu().numpy().copy()
    gain = None if case["gamma"] is None or not use_gain else torch.tensor(case["gamma"], dtype=torch.float32).to(device)
    out, stats = ops.wave_limit(rows, list(case["db"]), gain=gain, look=case["H"], out=orows)
    sync()
    st, after = stats.cpu().numpy(), obuf.cpu().numpy()
    assert st.shape == (len(sig), 4) and st.dtype == np.float64
    assert np.array_equal(buf.cpu().numpy(), before, equal_nan=True), f"{name}: wav is only read"
    keep = np.ones(len(after), bool)
    got = []
    for r, ((a, b), x) in enumerate(zip(ospans, sig)):
        keep[a:b] = False
        got.append(after[a:b].copy())
        check_row(name, r, x, case["db"][r], 1.0 if case["gamma"] is None else case["gamma"][r], case["H"], got[-1], st[r])
    assert np.isnan(after[keep]).all(), f"{name}: nothing outside the rows of out is written"
    return got, st


def check_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    """Every -22 case of the entry, each with the entry's name in cbx_last_error and nothing written; then (run_good) the good descriptor runs: rc 0 and the
    oracle's output"""
    import ctypes
    x0 = bursts(1276, 3)
    x = torch.from_numpy(x0).to(device)
    out = torch.full((1276,), 7.0, dtype=torch.float32, device=device)
    stats = torch.full((1, 4), 7.0, dtype=torch.float64, device=device)
    ws = torch.zeros(8, dtype=torch.float64, device=device)
    f = ops.true_peak_filter()
    tab, win = torch.from_numpy(f["tab"]).to(device), torch.from_numpy(ops.limit_window(LOOK)).to(device)
    A = ctypes.addressof
    dbl = lambda v: (ctypes.c_double * 1)(v)
    cl, off, ln = dbl(0.5), (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(1276)
    neg_off, neg_len, far_off, zero, neg, inf, tiny = (ctypes.c_long * 1)(-1), (ctypes.c_int * 1)(-1), (ctypes.c_long * 1)(1), dbl(0.0), dbl(-0.5), dbl(float("inf")), dbl(1e-60)
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), R=1, gain=None, ceil=A(cl), tab=tab.data_ptr(), U=f["U"], T=f["T"], win=win.data_ptr(), H=LOOK,
                out=out.data_ptr(), ooff=A(off), ocap=1276, stats=stats.data_ptr(), ws=ws.data_ptr(), cap=ws.numel())
    call = lambda d: lib.cbx_wave_limit_f32(d["wav"], d["off"], d["len"], d["R"], d["gain"], d["ceil"], d["tab"], d["U"], d["T"], d["win"], d["H"], d["out"], d["ooff"],
                                            d["ocap"], d["stats"], d["ws"], d["cap"], stream)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "ceil", "tab", "win", "stats", "ws", "ooff")]
    bad += [dict(good, R=0), dict(good, R=65), dict(good, len=A(neg_len)), dict(good, off=A(neg_off)), dict(good, ooff=A(neg_off)), dict(good, U=0), dict(good, U=9),
            dict(good, T=0), dict(good, U=8, T=129), dict(good, H=0), dict(good, H=481), dict(good, ceil=A(zero)), dict(good, ceil=A(neg)), dict(good, ceil=A(inf)),
            dict(good, ceil=A(tiny)), dict(good, ocap=1275), dict(good, ooff=A(far_off)), dict(good, out=x.data_ptr()), dict(good, out=x.data_ptr() + 4 * 1275, ocap=1 << 20),
            dict(good, cap=7)]
    for d in bad:
        assert call(d) == -22 and b"wave_limit" in lib.cbx_last_error(), d
    sync()
    assert float(stats.min()) == 7.0 and float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(ws.abs().max()) == 0.0 and np.array_equal(x.cpu().numpy(), x0), \
        "a refusal writes nothing"
    if run_good:
        assert call(good) == 0
        sync()
        check_row("good", 0, x0, 20.0 * np.log10(0.5), 1.0, LOOK, out.cpu().numpy(), stats.cpu().numpy()[0])
        assert call(dict(good, out=None, ooff=None, ocap=0)) == 0, "measure only: out and out_off NULL"


# ----------------------------------------------------------------------------- the properties beyond "equals the oracle", shared by the host and the GPU tests
def _launch(ops, signals, db, gamma, H, mis, device, sync, **kw):
    buf, rows, _ = L.padded_rows(signals, mis, device)
    gain = None if gamma is None else torch.tensor(gamma, dtype=torch.float32).to(device)
    out, stats = ops.wave_limit(rows, list(db), gain=gain, look=H, **kw)
    sync()
    return [o.cpu().numpy() for o in out], stats.cpu().numpy()


def check_inter_sample(ops, device="cpu", sync=lambda: None):
    """the case a sample-peak implementation fails: every |x| is 0.7071 < C = 0.9, yet the row is limited"""
    case = cases()["inter_sample"]
    x = case["signals"][0]
    assert abs(float(np.abs(x).max()) - np.sqrt(0.5)) < 1e-6, "the sample peak is 0.7071"
    got, st = run_case(ops, "inter_sample", case, 2, device, sync)
    assert st[0, 0] >= 1.0 and st[0, 1] < 1.0 and st[0, 2] > 0 and st[0, 3] > 0, st
    assert not np.array_equal(got[0], x), "the row is not returned unchanged"


def check_gain_null(ops, device="cpu", sync=lambda: None):
    sig = [bursts(N, 5) * np.float32(3.0), bursts(1025, 7)]
    a, sa = _launch(ops, sig, [-1.0, None], None, LOOK, 1, device, sync)
    b, sb = _launch(ops, sig, [-1.0, None], [1.0, 1.0], LOOK, 1, device, sync)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(sa, sb), "gain = NULL is a gain of ones, bit for bit"


def check_measure_only(ops, device="cpu", sync=lambda: None):
    sig = [bursts(N, 5) * np.float32(3.0), bursts(1276, 6), np.zeros(0, np.float32)]
    _, st = _launch(ops, sig, [-1.0, -6.0, -1.0], None, LOOK, 3, device, sync)
    buf, rows, _ = L.padded_rows(sig, 3, device)
    before = buf.cpu().numpy().copy()
    tp = ops.wave_true_peak(rows)
    sync()
    tp = tp.cpu().numpy()
    assert np.array_equal(buf.cpu().numpy(), before, equal_nan=True), "the meter writes nothing into the waveforms"
    assert np.array_equal(tp[:, 0], st[:, 0]) and np.array_equal(tp[:, 1:], [[1.0, 0.0, 0.0]] * 3), (tp, st)
    for r, x in enumerate(sig):
        assert abs(tp[r, 0] - true_peak(x)) <= TOL_OUT * max(1e-30, float(np.abs(x).max(initial=0.0)))


def check_nan_row(ops, device="cpu", sync=lambda: None):
    """one NaN sample: the true peak reads NaN, the call returns, and samples further than the filter's reach plus 2 H from it equal the oracle's"""
    x = bursts(N, 5) * np.float32(3.0)
    x[700] = np.nan
    got, st = _launch(ops, [x, bursts(1025, 7)], [-1.0, -1.0], None, LOOK, 0, device, sync)
    far = np.abs(np.arange(N) - 700) > 2 * LOOK + T
    check_row("nan_row", 0, x, -1.0, 1.0, LOOK, got[0], st[0], far=far)
    check_row("nan_row", 1, bursts(1025, 7), -1.0, 1.0, LOOK, got[1], st[1])
    assert np.isnan(got[0][700])


def check_determinism(ops, device="cpu", sync=lambda: None):
    """the same rows at two misalignments, and as R = 1 calls against one R = 3 call: out and stats bit for bit equal"""
    sig, db, gam = [bursts(3333, 8), bursts(N, 5), bursts(1025, 7)], [-1.0, -6.0, DB09], [3.0, 3.0, 2.0]
    a, sa = _launch(ops, sig, db, gam, LOOK, 0, device, sync)
    b, sb = _launch(ops, sig, db, gam, LOOK, 3, device, sync)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(sa, sb), "the result does not depend on the rows' alignment"
    for r in range(3):
        c, sc = _launch(ops, [sig[r]], [db[r]], [gam[r]], LOOK, 1, device, sync)
        assert np.array_equal(c[0], a[r]) and np.array_equal(sc[0], sa[r]), "a row alone is the row in the batch"


def check_many_rows(ops, device="cpu", sync=lambda: None):
    """R = 64, the most rows a call takes, two tiles each: every row against the oracle"""
    sig = [bursts(1100 + r, 100 + r) for r in range(64)]
    db = [None if r % 5 == 4 else -1.0 - (r % 3) for r in range(64)]
    gam = [1.0 + (r % 4) for r in range(64)]
    got, st = _launch(ops, sig, db, gam, LOOK, 2, device, sync)
    for r in range(64):
        check_row("many_rows", r, sig[r], db[r], gam[r], LOOK, got[r], st[r])


def check_other_table(lib, ops, device="cpu", stream=None, sync=lambda: None):
    """the entry with a table that is not the product's (U = 2, T = 21: the kernel's general tap loop) against the oracle for that U"""
    import ctypes
    x0 = bursts(1276, 3) * np.float32(3.0)
    ref = oracle(x0, -1.0, 1.0, LOOK, U=2)
    x = torch.from_numpy(x0).to(device)
    out = torch.full((1276,), float("nan"), dtype=torch.float32, device=device)
    stats, ws = torch.zeros(1, 4, dtype=torch.float64, device=device), torch.zeros(8, dtype=torch.float64, device=device)
    tab = torch.from_numpy(np.ascontiguousarray(taps(2).astype(np.float32))).to(device)
    win = torch.from_numpy(ops.limit_window(LOOK)).to(device)
    off, ln, cl = (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(1276), (ctypes.c_double * 1)(linear(-1.0))
    A = ctypes.addressof
    assert lib.cbx_wave_limit_f32(x.data_ptr(), A(off), A(ln), 1, None, A(cl), tab.data_ptr(), 2, T, win.data_ptr(), LOOK, out.data_ptr(), A(off), 1276, stats.data_ptr(),
                                  ws.data_ptr(), ws.numel(), stream) == 0
    sync()
    scale = float(np.abs(x0).max())
    err, st = float(np.abs(out.cpu().numpy().astype(np.float64) - ref["out"]).max()) / scale, stats.cpu().numpy()[0]
    print(f"U = 2: |dout|/max|u| {err:.3g} (allowed {TOL_OUT:.3g}) stats {list(st)} oracle {ref['stats']}")
    assert err <= TOL_OUT and abs(st[0] - ref["stats"][0]) <= TOL_OUT * scale and abs(st[1] - ref["stats"][1]) <= TOL_G and st[3] > 0
