"""Shared by tests/test_loudness_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_loudness_kernels_gpu.py and tests/test_loudness_api_gpu.py: the
oracle of the loudness launches (include/cbx.h cbx_wave_loudness_f32 / cbx_wave_gain_f32) -- a NumPy / SciPy fp64 restatement with
scipy.signal.lfilter --, the signal builders and the check of a launch against the oracle.  Not a test module.

Tolerances (the issue's): |dL| <= 1e-6 LU -- fp64 sums of <= 1e6 terms leave ~4e-10 LU, the 4096-sample warm-up 4e-14 of the signal; an fp32 state, at ~5e-3 LU,
misses it --, peak and blocks exact, gain within 1e-6 relative (one fp32 rounding, 6e-8, plus 1e-6 LU = 1.2e-7).  Every case asserts that no block lies within
1e-3 LU of a gate, so that no block can change sides inside the tolerance."""
import numpy as np
import torch

FS = 24000
TOL_L, TOL_GAIN, GATE_MARGIN = 1e-6, 1e-6, 1e-3
LENGTHS = (0, 1, 9599, 9600, 9601, 12000, 25234)
AMPS = (0.0, 1e-5, 0.003, 0.05, 0.3)


def k_coefficients(fs=FS):
    """((b, a) of the high shelf, (b, a) of the high pass): the RBJ forms of pyloudnorm.Meter's K-weighting, fp64, normalised by a0 -- written out here
    independently of ops.loudness_filter"""
    out = []
    for kind, G, Q, fc in (("shelf", 4.0, 1.0 / np.sqrt(2.0), 1500.0), ("hp", 0.0, 0.5, 38.0)):
        A = 10.0 ** (G / 40.0)
        w0 = 2.0 * np.pi * (fc / fs)
        alpha = np.sin(w0) / (2.0 * Q)
        if kind == "shelf":
            b = [A * ((A + 1) + (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha), -2 * A * ((A - 1) + (A + 1) * np.cos(w0)),
                 A * ((A + 1) + (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha)]
            a = [(A + 1) - (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha, 2 * ((A - 1) - (A + 1) * np.cos(w0)), (A + 1) - (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha]
        else:
            b = [(1 + np.cos(w0)) / 2, -(1 + np.cos(w0)), (1 + np.cos(w0)) / 2]
            a = [1 + alpha, -2 * np.cos(w0), 1 - alpha]
        out.append((np.array(b, np.float64) / a[0], np.array(a, np.float64) / a[0]))
    return out


def oracle(x, target=None, ceiling=1.0, fs=FS):
    """The definition on one row, in fp64 -> dict(L, peak, gain (fp64), gain32, blocks, margin): margin = the least distance in LU of a block that is not silent
    (z > 0) from the absolute gate, and of a block inside the absolute gate from the relative one (inf when there is none)."""
    from scipy.signal import lfilter
    x = np.asarray(x)
    n, hop = len(x), fs // 10
    assert hop * 10 == fs
    y = np.asarray(x, np.float64)
    for b, a in k_coefficients(fs):
        y = lfilter(b, a, y)
    S = n // hop
    E = (y[: S * hop].reshape(S, hop) ** 2).sum(axis=1) if S else np.zeros(0)
    nb = max(0, S - 3)
    z = np.array([(E[j] + E[j + 1] + E[j + 2] + E[j + 3]) / (4.0 * hop) for j in range(nb)], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z) if nb else np.zeros(0)
        absg = l >= -70.0
        L, blocks, margin = -np.inf, 0, np.inf
        if nb and np.isfinite(l).any():
            margin = np.abs(l[np.isfinite(l)] + 70.0).min()
        if absg.any():
            gate = -0.691 + 10.0 * np.log10(z[absg].mean()) - 10.0
            margin = min(margin, np.abs(l[absg] - gate).min())
            use = absg & (l > gate)
            if use.any():
                L, blocks = -0.691 + 10.0 * np.log10(z[use].mean()), int(use.sum())
        peak = float(np.abs(x).max()) if n else 0.0
        g = 1.0
        if target is not None and not np.isnan(target):
            g = 10.0 ** ((target - L) / 20.0)
            if ceiling is not None and ceiling > 0 and peak * g > ceiling:
                g = ceiling / peak
            if not (np.isfinite(L) and np.isfinite(peak) and np.isfinite(g)):
                g = 1.0
    return dict(L=float(L), peak=peak, gain=float(g), gain32=np.float32(g), blocks=blocks, margin=float(margin))


def bursts(n, seed):
    """Noise bursts: every 1200 samples another amplitude of AMPS, so that blocks fall on both sides of both gates -- yet none near one (>= 1.19 LU at 25 234 and
    72 007 samples; every test asserts its own margin)"""
    rng = np.random.default_rng(seed)
    amp = np.repeat(rng.choice(AMPS, size=n // 1200 + 1), 1200)[:n]
    return (rng.standard_normal(n) * amp).astype(np.float32)


def sine(n, freq=997.0, amp=1.0, fs=FS):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(n) / fs)).astype(np.float32)


def padded_rows(signals, mis, device="cpu"):
    """The signals as views of ONE NaN-filled fp32 buffer, row r beginning (mis + r) % 4 floats above a 16-byte boundary, at least 4 NaNs between rows ->
    (buffer, rows, [(start, stop)])"""
    spans, pos = [], 8
    for r, s in enumerate(signals):
        pos = (pos + 3) // 4 * 4 + (mis + r) % 4
        spans.append((pos, pos + len(s)))
        pos += len(s) + 4
    buf = torch.full((pos + 8,), float("nan"), dtype=torch.float32)
    for (a, b), s in zip(spans, signals):
        buf[a:b] = torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32))
    buf = buf.to(device)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf[a:b] for a, b in spans], spans


def check_stats(stats, gain, signals, targets, ceiling=1.0, min_margin=GATE_MARGIN):
    """stats (R, 4) / gain (R,) as host arrays of a launch over `signals` against the oracle; returns the oracle's rows"""
    stats, gain = np.asarray(stats, np.float64), np.asarray(gain, np.float32)
    refs = []
    for r, (x, t) in enumerate(zip(signals, targets)):
        ref = oracle(x, t, ceiling)
        assert ref["margin"] >= min_margin, f"row {r}: a block lies {ref['margin']:.2e} LU from a gate: the inputs do not separate the gates"
        L, peak, g, used = stats[r]
        print(f"row {r}: n {len(x)} L {L!r} (oracle {ref['L']!r}) peak {peak!r} gain {g!r} (oracle {ref['gain']!r}) blocks {used} ({ref['blocks']}) margin {ref['margin']:.3g}")
        if np.isfinite(ref["L"]):
            assert abs(L - ref["L"]) <= TOL_L, f"row {r}: L = {L}, oracle {ref['L']}"
        else:
            assert L == ref["L"], f"row {r}: L = {L}, oracle {ref['L']}"
        assert peak == ref["peak"] or (np.isnan(peak) and np.isnan(ref["peak"])), f"row {r}: peak = {peak}, oracle {ref['peak']}"
        assert used == ref["blocks"], f"row {r}: {used} blocks used, oracle {ref['blocks']}"
        assert abs(g - ref["gain"]) <= TOL_GAIN * ref["gain"] and abs(float(gain[r]) - ref["gain"]) <= TOL_GAIN * ref["gain"], f"row {r}: gain {g} / {gain[r]}, oracle {ref['gain']}"
        assert gain[r] == np.float32(g), f"row {r}: the stored gain {gain[r]} is not (float){g}"
        refs.append(ref)
    return refs


# ----------------------------------------------------------------------------- the cases, and a launch against the oracle
GROUPS = ((0, 9601, 25234), (1, 9600, 12000), (9599, 25234, 0))   # R = 3: every length of LENGTHS, an empty row first, in the middle and last
TARGETS = (-30.0, None, -23.0)


def run_case(ops, signals, targets, mis, device="cpu", sync=lambda: None, ceiling=1.0):
    """One wave_loudness + wave_gain over `signals` as rows of one NaN-padded buffer at misalignment `mis`: stats and gain against the oracle, the rows bit for bit
    x * float32(gain), the padding still NaN.  Returns (stats, gain) as host arrays."""
    buf, rows, spans = padded_rows(signals, mis, device)
    stats, gain = ops.wave_loudness(rows, list(targets), ceiling)
    sync()
    st, g = stats.cpu().numpy(), gain.cpu().numpy()
    assert st.shape == (len(signals), 4) and st.dtype == np.float64 and g.dtype == np.float32
    check_stats(st, g, signals, targets, ceiling)
    assert np.array_equal(np.isnan(buf.cpu().numpy()), np.isnan(padded_rows(signals, mis)[0].numpy())), "the meter writes nothing into the waveforms"
    ops.wave_gain(rows, gain)
    sync()
    after = buf.cpu().numpy()
    keep = np.ones(len(after), bool)
    for (a, b), x, gr in zip(spans, signals, g):
        keep[a:b] = False
        assert np.array_equal(after[a:b], np.asarray(x, np.float32) * np.float32(gr), equal_nan=True), "a row is bit for bit x * float32(gain)"
    assert np.isnan(after[keep]).all(), "nothing outside the rows is touched"
    return st, g


def check_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    """Every -22 case of the two entries, each with the entry's name in cbx_last_error and nothing written; then (run_good) the good descriptor runs: rc 0 and
    the oracle's gain"""
    import ctypes
    x = torch.from_numpy(bursts(12000, 3)).to(device)
    stats = torch.full((1, 4), 7.0, dtype=torch.float64, device=device)
    gain = torch.full((1,), 7.0, dtype=torch.float32, device=device)
    ws = torch.zeros(6 * 5, dtype=torch.float64, device=device)
    f = ops.loudness_filter(FS)
    coef = (ctypes.c_double * 10)(*f["coef"].tolist())
    bad_coef = (ctypes.c_double * 10)(*([float("inf")] + f["coef"].tolist()[1:]))
    tg = (ctypes.c_double * 1)(-20.0)
    off, ln = (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(12000)
    neg_off, neg_len = (ctypes.c_long * 1)(-1), (ctypes.c_int * 1)(-1)
    A = ctypes.addressof
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), R=1, coef=A(coef), hop=f["hop"], tg=A(tg), ceiling=1.0, stats=stats.data_ptr(), gain=gain.data_ptr(),
                ws=ws.data_ptr(), cap=ws.numel())
    call = lambda d: lib.cbx_wave_loudness_f32(d["wav"], d["off"], d["len"], d["R"], d["coef"], d["hop"], d["tg"], d["ceiling"], d["stats"], d["gain"], d["ws"], d["cap"], stream)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "coef", "tg", "stats", "gain", "ws")]
    bad += [dict(good, R=0), dict(good, R=65), dict(good, len=A(neg_len)), dict(good, off=A(neg_off)), dict(good, hop=0), dict(good, hop=-5), dict(good, coef=A(bad_coef)),
            dict(good, cap=6 * 5 - 1)]
    for d in bad:
        assert call(d) == -22 and b"wave_loudness" in lib.cbx_last_error(), d
    g_good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), R=1, gain=gain.data_ptr())
    g_call = lambda d: lib.cbx_wave_gain_f32(d["wav"], d["off"], d["len"], d["R"], d["gain"], stream)
    for d in [dict(g_good, **{k: None}) for k in ("wav", "off", "len", "gain")] + [dict(g_good, R=0), dict(g_good, R=65), dict(g_good, len=A(neg_len)), dict(g_good, off=A(neg_off))]:
        assert g_call(d) == -22 and b"wave_gain" in lib.cbx_last_error(), d
    sync()
    assert float(stats.min()) == 7.0 and float(gain[0]) == 7.0 and float(ws.abs().max()) == 0.0 and np.array_equal(x.cpu().numpy(), bursts(12000, 3)), "a refusal writes nothing"
    if run_good:
        assert call(good) == 0 and g_call(g_good) == 0
        sync()
        ref = oracle(bursts(12000, 3), -20.0)
        assert float(gain[0]) == float(ref["gain32"]) and np.array_equal(x.cpu().numpy(), bursts(12000, 3) * ref["gain32"])
