"""Shared by tests/test_wave_mix_host.py (SIMT emulator, CPU tensors), tests/test_wave_mix_kernels_gpu.py and tests/test_dialogue_api_gpu.py: the oracle of the
dialogue mixer (include/cbx.h cbx_wave_mix_f32) -- the definition in NumPy float32, a Python loop over the rows in ascending order, every product and every sum a
float32 operation of its own, written independently of ops --, the cases, the launch of a case over NaN-padded buffers and check_refusals.  Not a test module.

Comparison is BITWISE (an int32 view of the float32 arrays) everywhere: the definition fixes every rounding and the order of summation, so there is no tolerance
to state.  The one exception is the split-launch check, which compares values (-0.0 == +0.0): where the first launch covers nothing it stores +0.0 and a later
launch adds to it, while one launch over all rows stores the first covering row's value itself, which may be -0.0."""
import numpy as np
import torch

import loudness_common as L

FADE = 240


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def ramp(fade):
    """the join's ramp: (2 i + 1) / (2 fade) in fp64, rounded to fp32"""
    return ((2.0 * np.arange(fade, dtype=np.float64) + 1.0) / (2.0 * fade)).astype(np.float32) if fade else np.zeros(0, np.float32)


def faded(x, flag, fade, g=None):
    """steps 1 - 3 of the definition over one row: x * g (one float32 multiply; none when g is None), then the fade-in, else the fade-out"""
    s = np.asarray(x, np.float32).copy()
    n = len(s)
    if g is not None:
        s = s * np.float32(g)
    F, rp = min(int(fade), n // 2), ramp(fade)
    i = np.arange(n)
    fin = (i < F) if flag & 1 else np.zeros(n, bool)
    fout = ((i >= n - F) & ~fin) if flag & 2 else np.zeros(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        s[fin] = s[fin] * rp[i[fin]]
        s[fout] = s[fout] * rp[n - 1 - i[fout]]
    assert s.dtype == np.float32
    return s


def oracle(rows, starts, flags, out_len, gain=None, gain_idx=None, fade=FADE, prev=None):
    """The definition.  rows: float32 arrays; gain: None or G numbers; gain_idx: None (row r uses gain[r]) or R ints; prev: None (accumulate = 0) or the
    out_len samples `out` holds before the launch (accumulate = 1).  Returns the out_len float32 samples after the launch."""
    acc = np.zeros(out_len, np.float32) if prev is None else np.asarray(prev, np.float32).copy()
    has = np.zeros(out_len, bool) if prev is None else np.ones(out_len, bool)
    assert len(acc) == out_len
    for r, x in enumerate(rows):          # ascending r: the order of summation
        n, a = len(x), int(starts[r])
        if n == 0:
            continue
        assert 0 <= a and a + n <= out_len
        g = None if gain is None else gain[r if gain_idx is None else gain_idx[r]]
        s = faded(x, int(flags[r]), fade, g)
        seg, h = acc[a: a + n], has[a: a + n]
        with np.errstate(invalid="ignore", over="ignore"):
            acc[a: a + n] = np.where(h, seg + s, s)   # the first covering row's value itself, then one rounded add per further row
        has[a: a + n] = True
    return acc


# ----------------------------------------------------------------------------- the cases
def noise(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)


def _order_rows(T):
    vals = (2.0 ** 24, 1.0, 1.0, -(2.0 ** 24))
    rows = []
    for r in range(8):
        x = noise(1100, 40 + r)
        x[500 if r < 4 else 599] = vals[r % 4]
        rows.append(x)
    return rows


def cases(T):
    """name -> dict(rows, starts, flags, out_len, gain, gain_idx, fade); T = the kernel's tile (ops.WAVE_MIX_TILE)"""
    out = {}
    out["one_row"] = dict(rows=[noise(T + 1, 1)], starts=[0], flags=[3], out_len=T + 1, gain=None, gain_idx=None)
    out["tile_edge"] = dict(rows=[noise(T + 7, 2), noise(19, 3), noise(3, 4)], starts=[0, T - 5, T - 1], flags=[3, 3, 3], out_len=T + 14, gain=[0.5, 1.7, 0.9], gain_idx=None)
    # ascending order gives exactly 0.0 at samples 500 and T - 1; pairwise summation 1.0, descending 2.0
    out["order"] = dict(rows=_order_rows(T), starts=[0] * 4 + [T - 600] * 4, flags=[0] * 8, out_len=T - 600 + 1100, gain=None, gain_idx=None)
    for o, lens in enumerate(((0, 1, 2, 3, 5), (1, 2, 0, 3, 5), (1, 2, 3, 5, 0))):   # F = 0, 0, 1, 1, 2; an empty row first, in the middle, last
        for f in range(4):
            starts = [0 if n == 0 and k == 0 else (9 if n == 0 and k == 4 else min(k, 9 - n)) for k, n in enumerate(lens)]
            out[f"tiny{o}_flags{f}"] = dict(rows=[noise(n, 60 + n) + np.float32(1.0) for n in lens], starts=starts, flags=[f] * 5, out_len=9,
                                            gain=[2.0, 3.0], gain_idx=[k % 2 for k in range(5)])
    out["tiny_mixed"] = dict(rows=[noise(n, 70 + n) + np.float32(1.0) for n in (5, 3, 2, 1, 0)], starts=[2, 0, 6, 7, 3], flags=[0, 1, 2, 3, 3], out_len=8, gain=None, gain_idx=None)
    out["gap"] = dict(rows=[noise(300, 5), noise(400, 6)], starts=[0, 1000], flags=[3, 3], out_len=1400, gain=[1.5, 0.25], gain_idx=None)
    out["stack64"] = dict(rows=[noise(1100 + r, 100 + r) for r in range(64)], starts=[0] * 64, flags=[r % 4 for r in range(64)], out_len=1100 + 63,
                          gain=[0.5, 1.25, 3.0], gain_idx=[r % 3 for r in range(64)])
    for c in out.values():
        c.setdefault("fade", FADE)
    return out


# ----------------------------------------------------------------------------- a launch over NaN-padded buffers
def launch(ops, case, mis=0, device="cpu", sync=lambda: None, accumulate=False, prefill=None, subset=None, obuf=None, **over):
    """ops.wave_mix over the case's rows (subset: a range of them) as views of ONE NaN-padded buffer at misalignments mis + r, into `out`, a view of another
    NaN-padded buffer at misalignment (mis + 1) % 4 (obuf: the buffer of an earlier launch of the same case, to accumulate into).  Checks that the padding of
    out is still NaN and that wav is unchanged.  Returns (the out_len samples as a host array, obuf)."""
    c = dict(case, **over)
    idx = list(range(len(c["rows"]))) if subset is None else list(subset)
    buf, rows, _ = L.padded_rows([c["rows"][r] for r in idx], mis, device)
    before = buf.cpu().numpy().copy()
    n, lo = c["out_len"], 8 + (mis + 1) % 4
    if obuf is None:
        obuf = torch.full((n + 24,), float("nan"), dtype=torch.float32)
        if prefill is not None:
            obuf[lo: lo + n] = torch.from_numpy(np.ascontiguousarray(prefill, dtype=np.float32))
        obuf = obuf.to(device)
    assert obuf.data_ptr() % 16 == 0
    out = obuf[lo: lo + n]
    gain = None if c["gain"] is None else torch.tensor(c["gain"], dtype=torch.float32).to(device)
    gidx = None if c["gain_idx"] is None else [c["gain_idx"][r] for r in idx]
    if gain is not None and gidx is None and subset is not None:
        gidx = idx
    res = ops.wave_mix(rows, [c["starts"][r] for r in idx], [c["flags"][r] for r in idx], out, gain=gain, gain_idx=gidx, fade=c["fade"], accumulate=accumulate)
    sync()
    assert res is out
    after = obuf.cpu().numpy()
    assert np.array_equal(buf.cpu().numpy().view(np.int32), before.view(np.int32)), "wav is only read"
    assert np.isnan(after[:lo]).all() and np.isnan(after[lo + n:]).all(), "nothing outside out[0, out_len) is written"
    return after[lo: lo + n].copy(), obuf


def run_case(ops, name, case, mis, device="cpu", sync=lambda: None):
    """One launch with accumulate=False and one with accumulate=True over a pre-filled out, each bitwise against the oracle"""
    ref = oracle(case["rows"], case["starts"], case["flags"], case["out_len"], case["gain"], case["gain_idx"], case["fade"])
    got, _ = launch(ops, case, mis, device, sync)
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert bad.size == 0, f"{name} (misalignment {mis}): {bad.size} samples differ from the oracle, the first at {bad[0]}: {got[bad[0]]!r} against {ref[bad[0]]!r}"
    pre = noise(case["out_len"], 7)
    ref = oracle(case["rows"], case["starts"], case["flags"], case["out_len"], case["gain"], case["gain_idx"], case["fade"], prev=pre)
    got, _ = launch(ops, case, mis, device, sync, accumulate=True, prefill=pre)
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert bad.size == 0, f"{name} (misalignment {mis}, accumulate): {bad.size} samples differ from the oracle, the first at {bad[0]}: {got[bad[0]]!r} against {ref[bad[0]]!r}"
    return got


def check_order(ops, T, device="cpu", sync=lambda: None):
    got, _ = launch(ops, cases(T)["order"], 0, device, sync)
    assert bits(got[[500, T - 1]]).tolist() == [0, 0], f"ascending order gives +0.0 (pairwise 1.0, descending 2.0): got {got[[500, T - 1]].tolist()}"


def check_gap(ops, T, device="cpu", sync=lambda: None):
    c = cases(T)["gap"]
    got, _ = launch(ops, c, 2, device, sync)
    assert bits(got[300:1000]).tolist() == [0] * 700, "uncovered samples are written as +0.0"
    pre = np.arange(1400, dtype=np.float32) * np.float32(-0.5) - np.float32(1.0)
    got, _ = launch(ops, c, 2, device, sync, accumulate=True, prefill=pre)
    assert same_bits(got[300:1000], pre[300:1000]), "with accumulate the uncovered samples keep what they held"
    assert same_bits(got, oracle(c["rows"], c["starts"], c["flags"], 1400, c["gain"], None, FADE, prev=pre))
    nanpre = np.full(1400, np.nan, np.float32)
    nanpre[:300], nanpre[1000:] = pre[:300], pre[1000:]
    got, _ = launch(ops, c, 1, device, sync, accumulate=True, prefill=nanpre)
    assert np.isnan(got[300:1000]).all() and not np.isnan(got[:300]).any() and not np.isnan(got[1000:]).any()


def check_gain_null(ops, T, device="cpu", sync=lambda: None):
    c = cases(T)["tile_edge"]
    a, _ = launch(ops, c, 1, device, sync, gain=None)
    b, _ = launch(ops, c, 1, device, sync, gain=[1.0, 1.0, 1.0])
    assert same_bits(a, b), "gain = NULL is a gain of ones, bit for bit"
    d, _ = launch(ops, c, 1, device, sync, gain_idx=[0, 1, 2])
    e, _ = launch(ops, c, 1, device, sync)
    assert same_bits(d, e), "gain_idx = NULL is range(R)"
    s = cases(T)["stack64"]
    g64 = [s["gain"][r % 3] for r in range(64)]
    a, _ = launch(ops, s, 0, device, sync)
    b, _ = launch(ops, s, 0, device, sync, gain=g64, gain_idx=None)
    assert same_bits(a, b), "one gain per voice through gain_idx is one gain per row"


def check_split(ops, T, device="cpu", sync=lambda: None):
    s = cases(T)["stack64"]
    whole, _ = launch(ops, s, 3, device, sync)
    g64 = dict(gain=s["gain"], gain_idx=s["gain_idx"])
    part, obuf = launch(ops, s, 3, device, sync, subset=range(0, 20), **g64)
    part, obuf = launch(ops, s, 3, device, sync, subset=range(20, 21), accumulate=True, obuf=obuf, **g64)
    part, obuf = launch(ops, s, 3, device, sync, subset=range(21, 64), accumulate=True, obuf=obuf, **g64)
    assert np.array_equal(part, whole), "rows given in groups over several launches give the values of one launch"


def check_nan(ops, T, device="cpu", sync=lambda: None):
    c = cases(T)["tile_edge"]
    clean, _ = launch(ops, c, 0, device, sync)
    rows = [x.copy() for x in c["rows"]]
    rows[1][3] = np.nan
    got, _ = launch(ops, dict(c, rows=rows), 0, device, sync)
    p = T - 5 + 3
    assert np.isnan(got[p]) and not np.isnan(np.delete(got, p)).any() and same_bits(np.delete(got, p), np.delete(clean, p))


def check_join(ops, device="cpu", sync=lambda: None):
    """with every after >= 0, no gain and the join's flags the mixer stores the join's bits"""
    sig, gaps = [noise(2051, 11), noise(0, 12), noise(1276, 13)], [3600, 5, 0]
    buf, rows, _ = L.padded_rows(sig, 1, device)
    piece = ops.wave_join(rows, gaps, trim_db=None, fade=FADE)
    sync()
    total = int(piece["layout"].cpu()[3])
    want = piece["out"].cpu().numpy()[:total]
    starts, n = ops.mix_layout([len(s) for s in sig], gaps)
    assert (starts, n) == ([0, 2051, 5651], 6927) and total == n
    c = dict(rows=sig, starts=starts, flags=[2, 3, 1], out_len=n, gain=None, gain_idx=None, fade=FADE)
    got, _ = launch(ops, c, 2, device, sync)
    assert same_bits(got, want) and same_bits(got, oracle(sig, starts, [2, 3, 1], n))


def check_mix_layout(ops):
    assert ops.mix_layout([100, 10, 50], [-30, 5, 0]) == ([0, 70, 105], 155), "the backchannel lies inside the first turn; the front stays at 100"
    assert ops.mix_layout([100, 50], [-500, 0]) == ([0, 0], 100), "a lead that would go below 0 is clipped"
    assert ops.mix_layout([0, 100, 0, 50, 0], [7, -30, 9, 4, 3]) == ([0, 0, 100, 70, 120], 120), "an empty row starts at the front and changes neither it nor the pending gap"
    assert ops.mix_layout([5, 7], [3, 99]) == ([0, 8], 15) and ops.mix_layout([0, 0], [5, 5]) == ([0, 0], 0)
    for bad in (lambda: ops.mix_layout([1, 2], [0]), lambda: ops.mix_layout([-1], [0])):
        try:
            bad()
        except ValueError as e:
            assert "mix_layout" in str(e)
        else:
            raise AssertionError("mix_layout accepted a bad argument")


# ----------------------------------------------------------------------------- the C ABI's refusals
def check_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    """Every -22 case of the entry, each with the entry's name in cbx_last_error and nothing written; then (run_good) the good descriptor runs: rc 0 and the
    oracle's output"""
    import ctypes
    x0 = noise(1276, 3)
    x = torch.from_numpy(x0).to(device)
    out = torch.full((1400,), 7.0, dtype=torch.float32, device=device)
    gain = torch.tensor([0.5, 2.0], dtype=torch.float32).to(device)
    rp = torch.from_numpy(ramp(FADE)).to(device)
    A = ctypes.addressof
    i2, l2 = (lambda a, b: (ctypes.c_int * 2)(a, b)), (lambda a, b: (ctypes.c_long * 2)(a, b))
    off, ln, st, fl, gi = l2(0, 600), i2(600, 676), l2(0, 500), i2(3, 1), i2(1, 0)
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), start=A(st), flags=A(fl), R=2, gain=gain.data_ptr(), G=2, gidx=A(gi), ramp=rp.data_ptr(), fade=FADE,
                out=out.data_ptr(), out_len=1400, acc=0)
    call = lambda d: lib.cbx_wave_mix_f32(d["wav"], d["off"], d["len"], d["start"], d["flags"], d["R"], d["gain"], d["G"], d["gidx"], d["ramp"], d["fade"], d["out"],
                                          d["out_len"], d["acc"], stream)
    keep = [l2(0, -1), i2(600, -1), l2(-1, 500), i2(3, 4), i2(-1, 1), i2(1, 2), i2(-1, 0)]   # (held here: the descriptors keep only addresses)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "start", "flags", "out")]
    bad += [dict(good, R=0), dict(good, R=65), dict(good, off=A(keep[0])), dict(good, len=A(keep[1])), dict(good, start=A(keep[2])), dict(good, out_len=1175),
            dict(good, out_len=-1), dict(good, fade=-1), dict(good, ramp=None), dict(good, gain=None), dict(good, G=0), dict(good, G=1),
            dict(good, gidx=A(keep[5])), dict(good, gidx=A(keep[6])), dict(good, gidx=None, G=1), dict(good, flags=A(keep[3])), dict(good, flags=A(keep[4])),
            dict(good, acc=2), dict(good, acc=-1), dict(good, out=x.data_ptr(), out_len=1276), dict(good, out=x.data_ptr() + 4 * 1275, out_len=1400)]
    for d in bad:
        assert call(d) == -22 and b"wave_mix" in lib.cbx_last_error(), d
    sync()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and np.array_equal(x.cpu().numpy(), x0), "a refusal writes nothing"
    if run_good:
        assert call(good) == 0
        sync()
        assert same_bits(out.cpu().numpy(), oracle([x0[:600], x0[600:]], [0, 500], [3, 1], 1400, [0.5, 2.0], [1, 0]))
        assert call(dict(good, gain=None, gidx=None, G=0, fade=0, ramp=None, acc=1)) == 0, "no gain, no fade: NULL gain, gain_idx and ramp"
        z_len, z_start = i2(0, 0), l2(0, 0)
        assert call(dict(good, out_len=0, len=A(z_len), start=A(z_start))) == 0, "an empty output: rc 0, no launch"
        sync()
