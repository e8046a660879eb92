"""Shared by tests/test_stereo_host.py (SIMT emulator, CPU tensors), tests/test_stereo_kernels_gpu.py and tests/test_stereo_api_gpu.py: the NumPy restatements of
the three stereo entries (include/cbx.h cbx_wave_pan_mix_f32, cbx_wave_loudness_ch_f32, cbx_wave_limit_ch_f32), the cases, and the checks of a launch against
them.  Not a test module.

Pan mix: float32 arithmetic on top of wave_mix_common.faded (steps 1 - 3), one rounded multiply per plane, one rounded add per further row in ascending r:
compared BIT FOR BIT, no tolerance.
Meter: the stereo row step in fp64 on top of loudness_common's K-weighting (scipy.signal.lfilter): e_s = E_(0,s) + E_(1,s), then the blocks and the gates.  The
tolerances are loudness_common's (TOL_L = 1e-6 LU, gain 1e-6 relative, peak and blocks exact): the stereo step adds one fp64 add per segment to a sum of 2400
fp64 terms, which moves no digit that TOL_L sees.
Limiter: the linked steps on top of limit_common's _peaks / window: m = the maximum over the channels, one c, a, g, then out_c = u_c g.  The tolerances are
limit_common's TOL_G / TOL_OUT (relative to the larger channel's max |u|): the linked step adds a maximum, which is exact."""
import ctypes

import numpy as np
import torch

import limit_common as K
import loudness_common as L
import wave_mix_common as M

HOP = 2400
FADE = 240
LOG2 = 10.0 * np.log10(2.0)


# ----------------------------------------------------------------------------- pan mix
def pan_oracle(rows, starts, flags, pan, out_len, gain=None, gain_idx=None, fade=FADE, prev=None):
    """The definition -> (2, out_len) float32.  pan: R pairs (left, right); prev: None (accumulate = 0) or the (2, out_len) planes before the launch."""
    acc = np.zeros((2, out_len), np.float32) if prev is None else np.asarray(prev, np.float32).copy()
    has = np.zeros(out_len, bool) if prev is None else np.ones(out_len, bool)
    for r, x in enumerate(rows):          # ascending r: the order of summation
        n, a = len(x), int(starts[r])
        if n == 0:
            continue
        g = None if gain is None else gain[r if gain_idx is None else gain_idx[r]]
        s = M.faded(x, int(flags[r]), fade, g)
        h = has[a: a + n]
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(2):
                t = s * np.float32(pan[r][c])      # one rounded multiply per plane
                assert t.dtype == np.float32
                acc[c, a: a + n] = np.where(h, acc[c, a: a + n] + t, t)
        has[a: a + n] = True
    return acc


def pan_case():
    """R = 3 rows of 1, 4097 and 5000 samples at 0, 3 and 4090: they overlap, and the second and third cross the 4096-output tile; a balance gain per voice through
    gain_idx; every row fades in and out"""
    rows = [M.noise(n, 40 + n) for n in (1, 4097, 5000)]
    return dict(rows=rows, starts=[0, 3, 4090], flags=[3, 3, 3], out_len=9090, gain=[0.75, 1.5], gain_idx=[1, 0, 1])


def pan_launch(ops, case, pan, device="cpu", sync=lambda: None, subset=None, accumulate=False, prefill=None, mis=1, use_gain=True):
    """ops.wave_pan_mix over the case's rows (views of one NaN-padded buffer at mixed alignments) into the planes of a NaN-padded buffer whose left plane begins
    `mis` floats above a 16-byte boundary -> the (2, n) planes as a host array; the padding is asserted to be NaN still"""
    n = case["out_len"]
    idx = list(range(len(case["rows"]))) if subset is None else list(subset)
    buf, rows, _ = L.padded_rows(case["rows"], 1, device)
    obuf = torch.full((2 * n + 16,), float("nan"), dtype=torch.float32)
    if prefill is not None:
        obuf[4 + mis: 4 + mis + 2 * n] = torch.from_numpy(np.ascontiguousarray(prefill, np.float32).reshape(-1))
    obuf = obuf.to(device)
    assert obuf.data_ptr() % 16 == 0
    out = obuf[4 + mis: 4 + mis + 2 * n].view(2, n)
    gain = torch.tensor(case["gain"], dtype=torch.float32).to(device) if use_gain else None
    res = ops.wave_pan_mix([rows[k] for k in idx], [case["starts"][k] for k in idx], [case["flags"][k] for k in idx], [pan[k] for k in idx], out, gain=gain,
                           gain_idx=[case["gain_idx"][k] for k in idx] if use_gain else None, fade=FADE, accumulate=accumulate)
    sync()
    assert res is out
    host = obuf.cpu().numpy()
    assert np.isnan(host[: 4 + mis]).all() and np.isnan(host[4 + mis + 2 * n:]).all(), "nothing outside the two planes is written"
    return host[4 + mis: 4 + mis + 2 * n].reshape(2, n).copy()


def check_pan_mix(ops, device="cpu", sync=lambda: None):
    c = pan_case()
    pan = [ops.pan_gains(-0.5), ops.pan_gains(0.3), (0.25, 1.5)]
    kw = dict(gain=c["gain"], gain_idx=c["gain_idx"])
    ref = pan_oracle(c["rows"], c["starts"], c["flags"], pan, c["out_len"], **kw)
    for mis in (1, 0, 2):
        got = pan_launch(ops, c, pan, device, sync, mis=mis)
        assert M.same_bits(got, ref), f"one launch over the three rows, out {mis} floats above a 16-byte boundary: bit for bit the restatement"
    # two launches: rows 0 and 1 write both planes, row 2 accumulates
    first = pan_launch(ops, c, pan, device, sync, subset=[0, 1])
    ref1 = pan_oracle(c["rows"][:2], c["starts"][:2], c["flags"][:2], pan[:2], c["out_len"], gain=c["gain"], gain_idx=c["gain_idx"][:2])
    assert M.same_bits(first, ref1) and not first[:, 4100:].any(), "uncovered samples are written as zeros"
    second = pan_launch(ops, c, pan, device, sync, subset=[2], accumulate=True, prefill=first)
    ref2 = pan_oracle(c["rows"][2:], c["starts"][2:], c["flags"][2:], pan[2:], c["out_len"], gain=c["gain"], gain_idx=c["gain_idx"][2:], prev=ref1)
    assert M.same_bits(second, ref2) and np.array_equal(second, ref), "the accumulating launch adds to what the first left: the values of one launch"
    # {1, 1} for every row: the mono mixer's bits in both planes
    buf, rows, _ = L.padded_rows(c["rows"], 1, device)
    mono = torch.full((c["out_len"],), float("nan"), dtype=torch.float32, device=device)
    ops.wave_mix(rows, c["starts"], c["flags"], mono, gain=torch.tensor(c["gain"], dtype=torch.float32).to(device), gain_idx=c["gain_idx"], fade=FADE)
    sync()
    mono = mono.cpu().numpy()
    ones = pan_launch(ops, c, [(1.0, 1.0)] * 3, device, sync)
    assert M.same_bits(ones[0], mono) and M.same_bits(ones[1], mono), "pan = {1, 1}: cbx_wave_mix_f32's bits in both planes"
    # equal gains: L == R bit for bit; a gain of 0: a plane of zeros
    centre = pan_launch(ops, c, [ops.pan_gains(0.0)] * 3, device, sync, use_gain=False)
    assert M.same_bits(centre[0], centre[1]) and centre[0].any()
    left = pan_launch(ops, c, [ops.pan_gains(-1.0)] * 3, device, sync)
    assert not left[1].any() and M.same_bits(left[0], mono), "hard left: the right plane is zeros, the left one the mono mix"


def check_pan_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    """every -22 of cbx_wave_pan_mix_f32 beyond the mono entry's, and a few of those: the entry's name in cbx_last_error, nothing written"""
    x0 = M.noise(100, 1)
    x = torch.from_numpy(np.concatenate([x0, np.full(300, 7.0, np.float32)])).to(device)   # the rows, then room for planes that overlap them
    out = torch.full((240,), 7.0, dtype=torch.float32, device=device)
    A = ctypes.addressof
    off, ln, st, fl = (ctypes.c_long * 2)(0, 50), (ctypes.c_int * 2)(50, 50), (ctypes.c_long * 2)(0, 60), (ctypes.c_int * 2)(0, 0)
    pan = (ctypes.c_float * 4)(1.0, 0.5, 0.5, 1.0)
    bad_pan = [(ctypes.c_float * 4)(1.0, v, 0.5, 1.0) for v in (float("nan"), float("inf"), float("-inf"))]
    far = (ctypes.c_long * 2)(0, 71)
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), start=A(st), flags=A(fl), pan=A(pan), R=2, gain=None, G=0, gidx=None, ramp=None, fade=0, out=out.data_ptr(),
                ps=120, n=120, acc=0)
    call = lambda d: lib.cbx_wave_pan_mix_f32(d["wav"], d["off"], d["len"], d["start"], d["flags"], d["pan"], d["R"], d["gain"], d["G"], d["gidx"], d["ramp"], d["fade"],
                                              d["out"], d["ps"], d["n"], d["acc"], stream)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "start", "flags", "pan", "out")]
    bad += [dict(good, pan=A(p)) for p in bad_pan]
    bad += [dict(good, ps=119), dict(good, ps=0), dict(good, R=0), dict(good, R=65), dict(good, n=-1), dict(good, start=A(far)), dict(good, fade=3), dict(good, acc=2),
            dict(good, out=x.data_ptr() + 4 * 40)]   # the LEFT plane lies over row 0 and row 1
    # the RIGHT plane alone over the rows: out lies 130 floats before the rows' end, its right plane begins at the rows' first sample
    lead = torch.full((400,), 7.0, dtype=torch.float32, device=device)
    rows2 = lead[200:300]
    rows2.copy_(torch.from_numpy(x0))
    bad.append(dict(good, wav=lead.data_ptr() + 4 * 200, out=lead.data_ptr(), ps=180))   # planes [0, 120) and [180, 300): the right one meets the rows at [200, 300)
    for d in bad:
        assert call(d) == -22 and b"wave_pan_mix" in lib.cbx_last_error(), d
    sync()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(x[100:].min()) == 7.0 and np.array_equal(x[:100].cpu().numpy(), x0), "a refusal writes nothing"
    assert float(lead[:200].min()) == 7.0 and float(lead[300:].min()) == 7.0
    if run_good:
        assert call(good) == 0
        sync()
        ref = pan_oracle([x0[:50], x0[50:]], [0, 60], [0, 0], [(1.0, 0.5), (0.5, 1.0)], 120, fade=0)
        assert M.same_bits(out.cpu().numpy().reshape(2, 120), ref)


# ----------------------------------------------------------------------------- the meter over two channels
def loud_oracle(xs, target=None, ceiling=1.0, fs=L.FS):
    """The definition over the channels xs (1 or 2 float32 arrays of one length), in fp64 -> loudness_common.oracle's dict.  The K-weighting is loudness_common's;
    the segment energies are added in channel order, then the blocks and the gates as loudness_common.oracle writes them."""
    from scipy.signal import lfilter
    n, hop = len(xs[0]), fs // 10
    assert all(len(x) == n for x in xs) and len(xs) in (1, 2)
    S = n // hop
    e = None
    for x in xs:
        y = np.asarray(x, np.float64)
        for b, a in L.k_coefficients(fs):
            y = lfilter(b, a, y)
        E = (y[: S * hop].reshape(S, hop) ** 2).sum(axis=1) if S else np.zeros(0)
        e = E if e is None else e + E     # one fp64 add in channel order
    nb = max(0, S - 3)
    z = np.array([(e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * hop) for j in range(nb)], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z) if nb else np.zeros(0)
        absg = l >= -70.0
        Lk, blocks, margin = -np.inf, 0, np.inf
        if nb and np.isfinite(l).any():
            margin = np.abs(l[np.isfinite(l)] + 70.0).min()
        if absg.any():
            gate = -0.691 + 10.0 * np.log10(z[absg].mean()) - 10.0
            margin = min(margin, np.abs(l[absg] - gate).min())
            use = absg & (l > gate)
            if use.any():
                Lk, blocks = -0.691 + 10.0 * np.log10(z[use].mean()), int(use.sum())
        peak = max(float(np.abs(x).max()) if n else 0.0 for x in xs)
        g = 1.0
        if target is not None and not np.isnan(target):
            g = 10.0 ** ((target - Lk) / 20.0)
            if ceiling is not None and ceiling > 0 and peak * g > ceiling:
                g = ceiling / peak
            if not (np.isfinite(Lk) and np.isfinite(peak) and np.isfinite(g)):
                g = 1.0
    return dict(L=float(Lk), peak=peak, gain=float(g), gain32=np.float32(g), blocks=blocks, margin=float(margin))


LOUD_LENGTHS = (4 * HOP, 4 * HOP - 1, 5 * HOP + 1203)   # exactly one block; none; two blocks and a ragged end


def loud_signals():
    """per length (left, right): two tones of different level and pitch -- steady, so that no block lies near a gate"""
    return [(L.sine(n, 997.0, 0.3), L.sine(n, 440.0, 0.11)) for n in LOUD_LENGTHS]


def _loud(ops, channels, targets, device, sync, mis=1, ch=2, ceiling=1.0):
    buf, rows, _ = L.padded_rows(channels, mis, device)
    stats, gain = ops.wave_loudness_ch(rows, list(targets), ceiling, channels=ch)
    sync()
    return stats.cpu().numpy(), gain.cpu().numpy()


def check_loud_stats(st, g, groups, targets, ceiling=1.0):
    for s, (xs, t) in enumerate(zip(groups, targets)):
        ref = loud_oracle(xs, t, ceiling)
        assert ref["margin"] >= L.GATE_MARGIN, f"signal {s}: a block lies {ref['margin']:.2e} LU from a gate"
        Lk, peak, gn, used = st[s]
        print(f"signal {s}: n {len(xs[0])} L {Lk!r} (restatement {ref['L']!r}, |d| {abs(Lk - ref['L']) if np.isfinite(ref['L']) else 0.0:.3g}, allowed {L.TOL_L:g}) peak {peak!r} gain {gn!r} blocks {used}")
        if np.isfinite(ref["L"]):
            assert abs(Lk - ref["L"]) <= L.TOL_L, f"signal {s}: L = {Lk}, restatement {ref['L']}"
        else:
            assert Lk == ref["L"] and gn == 1.0 and g[s] == 1.0, f"signal {s}: no block: L = -inf and gain 1, got {Lk}, {gn}"
        assert peak == ref["peak"] and used == ref["blocks"], f"signal {s}: peak {peak} / blocks {used}, restatement {ref['peak']} / {ref['blocks']}"
        assert abs(gn - ref["gain"]) <= L.TOL_GAIN * ref["gain"] and g[s] == np.float32(gn), f"signal {s}: gain {gn} / {g[s]}, restatement {ref['gain']}"


def check_loudness_ch(ops, device="cpu", sync=lambda: None):
    pairs = loud_signals()
    flat = [x for p in pairs for x in p]
    targets = [-23.0, -23.0, None]
    st, g = _loud(ops, flat, targets, device, sync)
    assert st.shape == (3, 4) and st.dtype == np.float64 and g.shape == (3,) and g.dtype == np.float32
    check_loud_stats(st, g, pairs, targets)
    assert st[0][3] == 1 and st[1][0] == -np.inf and st[1][3] == 0 and st[2][3] == 2, "4 hop: one block; 4 hop - 1: none; 5 hop + 1203: two"
    # swapped channels: identical bits
    st2, g2 = _loud(ops, [x for p in pairs for x in p[::-1]], targets, device, sync, mis=2)
    assert st.tobytes() == st2.tobytes() and g.tobytes() == g2.tobytes(), "the channels' energies are added in fp64: the sum commutes"
    # C = 1: the mono entry bit for bit
    buf, rows, _ = L.padded_rows(flat, 1, device)
    ms, mg = ops.wave_loudness(rows, [-23.0] * 6, 1.0)
    s1, g1 = ops.wave_loudness_ch(rows, [-23.0] * 6, 1.0, channels=1)
    sync()
    ms, mg = ms.cpu().numpy(), mg.cpu().numpy()
    assert ms.tobytes() == s1.cpu().numpy().tobytes() and mg.tobytes() == g1.cpu().numpy().tobytes(), "C = 1 is cbx_wave_loudness_f32 bit for bit"
    # L == R: the mono reading plus 10 log10 2
    st3, g3 = _loud(ops, [x for p in pairs for x in (p[0], p[0])], [None] * 3, device, sync)
    check_loud_stats(st3, g3, [(p[0], p[0]) for p in pairs], [None] * 3)
    for s in (0, 2):
        print(f"signal {s}: equal channels read {st3[s][0]!r}, mono {ms[2 * s][0]!r}")
        assert abs(st3[s][0] - (ms[2 * s][0] + LOG2)) <= L.TOL_L and st3[s][1] == ms[2 * s][1] and st3[s][3] == ms[2 * s][3]
    assert st3[1][0] == -np.inf


def check_loud_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    x0 = np.concatenate([L.sine(9600, amp=0.3), L.sine(9600, 440.0, 0.1)])
    x = torch.from_numpy(x0).to(device)
    stats = torch.full((2, 4), 7.0, dtype=torch.float64, device=device)
    gain = torch.full((2,), 7.0, dtype=torch.float32, device=device)
    ws = torch.zeros(6 * 2 * 4, dtype=torch.float64, device=device)
    A = ctypes.addressof
    f = ops.loudness_filter()
    coef, nan_coef = (ctypes.c_double * 10)(*f["coef"].tolist()), (ctypes.c_double * 10)(*([float("nan")] + f["coef"].tolist()[1:]))
    off, ln, odd, tg = (ctypes.c_long * 2)(0, 9600), (ctypes.c_int * 2)(9600, 9600), (ctypes.c_int * 2)(9600, 9599), (ctypes.c_double * 2)(-23.0, -23.0)
    neg = (ctypes.c_int * 2)(-1, -1)
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), R=2, C=2, coef=A(coef), hop=2400, tg=A(tg), stats=stats.data_ptr(), gain=gain.data_ptr(), ws=ws.data_ptr(), cap=ws.numel())
    call = lambda d: lib.cbx_wave_loudness_ch_f32(d["wav"], d["off"], d["len"], d["R"], d["C"], d["coef"], d["hop"], d["tg"], 1.0, d["stats"], d["gain"], d["ws"], d["cap"], stream)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "coef", "tg", "stats", "gain", "ws")]
    bad += [dict(good, C=0), dict(good, C=3), dict(good, R=1), dict(good, R=0), dict(good, R=66), dict(good, len=A(odd)), dict(good, len=A(neg)), dict(good, hop=0),
            dict(good, coef=A(nan_coef)), dict(good, cap=47)]
    for d in bad:
        assert call(d) == -22 and b"wave_loudness_ch" in lib.cbx_last_error(), d
    sync()
    assert float(stats.min()) == 7.0 and float(gain.min()) == 7.0 and float(ws.abs().max()) == 0.0 and np.array_equal(x.cpu().numpy(), x0), "a refusal writes nothing"
    if run_good:
        assert call(good) == 0
        sync()
        check_loud_stats(stats.cpu().numpy(), gain.cpu().numpy(), [(x0[:9600], x0[9600:])], [-23.0])


# ----------------------------------------------------------------------------- the linked limiter
def limit_oracle(xs, db, gamma=1.0, H=K.LOOK, dtype=np.float64):
    """Steps 1 - 7 over the channels xs of one signal -> dict(u [per channel, float32], m, c, g, out [per channel], stats).  limit_common.oracle's code with the
    maximum over the channels in step 3."""
    from numpy.lib.stride_tricks import sliding_window_view
    us = [np.asarray(x, np.float32) * np.float32(gamma) for x in xs]
    n = len(us[0])
    C = dtype(np.float32(K.linear(db))) if db is not None and dtype is np.float32 else (np.nan if db is None else K.linear(db))
    if n == 0:
        z = np.zeros(0, dtype)
        return dict(u=us, m=z, c=z, g=z, out=[z for _ in us], stats=[0.0, 1.0, 0, 0], C=C)
    m = None
    for u in us:
        mc = K._peaks(u.astype(dtype), dtype)
        m = mc if m is None else np.maximum(m, mc)     # (np.maximum propagates a NaN)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = np.isfinite(m) & (m > C)
        c = np.where(over, dtype(C) / np.where(over, m, 1), dtype(1))
    ext = np.ones(n + 4 * H, dtype)
    ext[2 * H: 2 * H + n] = c
    d = dtype(1) - sliding_window_view(ext, 2 * H + 1).min(axis=1)
    w = K.window(H).astype(dtype)
    s = np.zeros(n, dtype)
    for k in range(2 * H + 1):
        s = s + w[k] * d[k: k + n]
    g = np.minimum(dtype(1) - s, c)
    with np.errstate(invalid="ignore"):
        n_over = int((m > C).sum())
    return dict(u=us, m=m, c=c, g=g, out=[u.astype(dtype) * g for u in us], stats=[float(m.max()), float(g.min()), int((g < 1).sum()), n_over], C=C)


LIMIT_LENGTHS = (1, 1025, 2300)
BURST = (1020, 1028)      # an over-ceiling burst in the left channel across the boundary of the first 1024-sample tile


def limit_signals():
    """per length (left, right).  1 and 1025: loud noise in both channels; 2300: a quiet tone in both, and eight samples of +-2 in the LEFT one alone"""
    out = [tuple(K.bursts(n, 60 + n + c) * np.float32(3.0) for c in range(2)) for n in LIMIT_LENGTHS[:2]]
    n = LIMIT_LENGTHS[2]
    left, right = L.sine(n, amp=0.05), L.sine(n, 440.0, 0.3)
    left[BURST[0]: BURST[1]] = np.float32(2.0) * np.where(np.arange(BURST[1] - BURST[0]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return out + [(left, right)]


def _limit(ops, channels, db, gamma, device, sync, ch=2, mis=1, H=K.LOOK):
    buf, rows, _ = L.padded_rows(channels, mis, device)
    obuf, orows, ospans = L.padded_rows([np.zeros(len(s), np.float32) for s in channels], mis + 1, device)
    before = buf.cpu().numpy().copy()
    gain = None if gamma is None else torch.tensor(gamma, dtype=torch.float32).to(device)
    out, stats = ops.wave_limit_ch(rows, list(db), gain=gain, look=H, out=orows, channels=ch)
    sync()
    after = obuf.cpu().numpy()
    assert np.array_equal(buf.cpu().numpy(), before, equal_nan=True), "wav is only read"
    keep = np.ones(len(after), bool)
    for a, b in ospans:
        keep[a:b] = False
    assert np.isnan(after[keep]).all(), "nothing outside the rows of out is written"
    return [after[a:b].copy() for a, b in ospans], stats.cpu().numpy()


def check_linked(name, xs, db, gam, got, st, H=K.LOOK):
    """the outputs of one signal's channels and its stats row against the fp64 restatement, within limit_common's bounds"""
    ref = limit_oracle(xs, db, gam, H)
    scale = max(max(float(np.abs(u).max()) for u in ref["u"]), 1e-30)
    for c, (o, r) in enumerate(zip(got, ref["out"])):
        err = float(np.abs(o.astype(np.float64) - r).max()) / scale
        print(f"{name} channel {c}: n {len(o)} |dout|/max|u| {err:.3g} (allowed {K.TOL_OUT:.3g})")
        assert err <= K.TOL_OUT, f"{name} channel {c}: out deviates from u_c g of the restatement by {err:.3g} max|u|"
    tp, gmin, n_g, n_m = ref["stats"]
    print(f"{name}: stats {list(st)} restatement {ref['stats']}")
    assert abs(st[0] - tp) <= K.TOL_OUT * scale and abs(st[1] - gmin) <= K.TOL_G
    if db is None or not np.any(np.abs(ref["m"] - ref["C"]) <= K.TOL_OUT * scale):
        assert st[3] == n_m
    sure, maybe = int((ref["g"] < 1.0 - K.TOL_G).sum()), int(((ref["g"] >= 1.0 - K.TOL_G) & (ref["g"] < 1.0)).sum())
    assert sure <= st[2] <= sure + maybe
    if db is None or n_m == 0:
        assert all(np.array_equal(o, u, equal_nan=True) for o, u in zip(got, ref["u"])) and st[1] == 1.0 and st[2] == 0 and st[3] == 0
    elif H >= K.LOOK:   # the ceiling, at the samples and at the oversampled points between them, per channel
        Cl = K.linear(db)
        for c, (o, r) in enumerate(zip(got, ref["out"])):
            tp_ref, tp_got = K.true_peak(r), K.true_peak(o)
            assert tp_ref <= Cl * (1.0 + K.CEIL_PRE), f"{name} channel {c}: the restatement's own output reads {tp_ref / Cl - 1:.3g} over C"
            print(f"{name} channel {c}: true peak of the output {tp_got!r} (restatement's {tp_ref!r}, C {Cl!r})")
            assert tp_got <= max(Cl, tp_ref) + K.TOL_OUT * scale
    return ref


def check_limit_ch(ops, device="cpu", sync=lambda: None):
    pairs = limit_signals()
    flat = [x for p in pairs for x in p]
    db, gam = [-1.0, -1.0, K.DB09], [1.0, 0.9, 1.0]
    got, st = _limit(ops, flat, db, gam, device, sync)
    assert st.shape == (3, 4) and st.dtype == np.float64
    refs = [check_linked(f"signal {s}", pairs[s], db[s], gam[s], got[2 * s: 2 * s + 2], st[s]) for s in range(3)]
    # the burst in L lowers R by the same g: every sample over the ceiling is L's (the oversampler rings a few samples past the burst), g < 1 reaches 2 H beyond
    # them (the minimum over +- H, then the sum over +- H) and is 1 elsewhere, where R comes back untouched
    g, over = refs[2]["g"], np.flatnonzero(refs[2]["m"] > refs[2]["C"])
    quiet = float(K._peaks(pairs[2][1].astype(np.float64), np.float64).max())
    assert quiet < K.linear(K.DB09), "the right channel alone lies under the ceiling: alone it would pass untouched"
    assert BURST[0] - 8 <= over.min() <= BURST[0] and BURST[1] - 1 <= over.max() < BURST[1] + 8 and over.min() < 1024 <= over.max(), "the burst crosses the tile boundary"
    lo, hi = over.min() - 2 * K.LOOK, over.max() + 2 * K.LOOK + 1
    assert g[BURST[0]: BURST[1]].max() < 0.5 and (g[:lo] == 1.0).all() and (g[hi:] == 1.0).all() and st[2][2] > 0
    assert np.array_equal(got[5][:lo], pairs[2][1][:lo]) and np.array_equal(got[5][hi:], pairs[2][1][hi:]), "away from the burst R is untouched"
    assert np.abs(got[5][BURST[0]: BURST[1]]).max() < 0.5 * float(np.abs(pairs[2][1]).max()) + 1e-6, "R is pulled down with L"
    # a NaN ceiling: the signal passes through as u
    got_n, st_n = _limit(ops, flat, [None, -1.0, None], gam, device, sync, mis=2)
    for s in (0, 2):
        assert all(np.array_equal(got_n[2 * s + c], np.asarray(pairs[s][c], np.float32) * np.float32(gam[s])) for c in range(2)) and list(st_n[s][1:]) == [1.0, 0.0, 0.0]
    assert all(M.same_bits(got_n[2 + c], got[2 + c]) for c in range(2)), "a signal's result does not depend on its neighbours or its alignment"
    # C = 1: the mono entry bit for bit
    buf, rows, _ = L.padded_rows(flat, 1, device)
    gain6 = torch.tensor([1.0, 0.9, 1.0, 0.9, 1.0, 0.9], dtype=torch.float32).to(device)
    mono, ms = ops.wave_limit(rows, [-1.0] * 6, gain=gain6)
    one, s1 = ops.wave_limit_ch(rows, [-1.0] * 6, gain=gain6, channels=1)
    sync()
    assert ms.cpu().numpy().tobytes() == s1.cpu().numpy().tobytes() and all(M.same_bits(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(mono, one)), \
        "C = 1 is cbx_wave_limit_f32 bit for bit"
    # L == R: the mono limiter's output in both planes
    same, ss = _limit(ops, [x for p in pairs for x in (p[0], p[0])], [-1.0] * 3, None, device, sync)
    buf, rows, _ = L.padded_rows([p[0] for p in pairs], 3, device)
    mono, ms = ops.wave_limit(rows, [-1.0] * 3)
    sync()
    for s in range(3):
        m = mono[s].cpu().numpy()
        assert M.same_bits(same[2 * s], m) and M.same_bits(same[2 * s + 1], m), "equal channels: the mono output in both planes"
    assert ss.tobytes() == ms.cpu().numpy().tobytes()
    # measure only
    buf, rows, _ = L.padded_rows(flat, 1, device)
    none, sm = ops.wave_limit_ch(rows, None)
    sync()
    sm = sm.cpu().numpy()
    assert none is None and sm[2][0] == st[2][0] and list(sm[2][1:]) == [1.0, 0.0, 0.0], "measure only: the true peak over both channels, nothing limited"


def check_limit_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    x0 = np.concatenate([K.bursts(1276, 3), K.bursts(1276, 4)])
    x = torch.from_numpy(x0).to(device)
    out = torch.full((2552,), 7.0, dtype=torch.float32, device=device)
    stats = torch.full((1, 4), 7.0, dtype=torch.float64, device=device)
    ws = torch.zeros(8, dtype=torch.float64, device=device)
    f = ops.true_peak_filter()
    tab, win = torch.from_numpy(f["tab"]).to(device), torch.from_numpy(ops.limit_window(K.LOOK)).to(device)
    A = ctypes.addressof
    dbl = lambda v: (ctypes.c_double * 1)(v)
    off, ln, odd, neg = (ctypes.c_long * 2)(0, 1276), (ctypes.c_int * 2)(1276, 1276), (ctypes.c_int * 2)(1276, 1275), (ctypes.c_int * 2)(-1, -1)
    cl = dbl(0.5)
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), R=2, C=2, gain=None, ceil=A(cl), tab=tab.data_ptr(), U=f["U"], T=f["T"], win=win.data_ptr(), H=K.LOOK,
                out=out.data_ptr(), ooff=A(off), ocap=2552, stats=stats.data_ptr(), ws=ws.data_ptr(), cap=ws.numel())
    call = lambda d: lib.cbx_wave_limit_ch_f32(d["wav"], d["off"], d["len"], d["R"], d["C"], d["gain"], d["ceil"], d["tab"], d["U"], d["T"], d["win"], d["H"], d["out"],
                                               d["ooff"], d["ocap"], d["stats"], d["ws"], d["cap"], stream)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "ceil", "tab", "win", "stats", "ws", "ooff")]
    bad += [dict(good, C=0), dict(good, C=3), dict(good, R=1), dict(good, R=0), dict(good, R=66), dict(good, len=A(odd)), dict(good, len=A(neg)), dict(good, U=0),
            dict(good, H=481), dict(good, ceil=A(dbl(0.0))), dict(good, ceil=A(dbl(float("inf")))), dict(good, ocap=2551), dict(good, out=x.data_ptr()), dict(good, cap=7)]
    for d in bad:
        assert call(d) == -22 and b"wave_limit_ch" in lib.cbx_last_error(), d
    sync()
    assert float(stats.min()) == 7.0 and float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(ws.abs().max()) == 0.0 and np.array_equal(x.cpu().numpy(), x0), \
        "a refusal writes nothing"
    if run_good:
        assert call(good) == 0
        sync()
        o = out.cpu().numpy()
        check_linked("good", (x0[:1276], x0[1276:]), 20.0 * np.log10(0.5), 1.0, [o[:1276], o[1276:]], stats.cpu().numpy()[0])
