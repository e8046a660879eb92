"""Shared by tests/test_wave_pitch_host.py (SIMT emulator, CPU tensors), tests/test_turbo_stream_wave_pitch_kernels_gpu.py and tests/test_pitch_api_gpu.py: the
oracle of the pitch step (include/cbx.h cbx_wave_pitch_f32) -- the fp32 table built here from the formula, an fp64 restatement of the
definition on that table which also gives the bound's S_j and D_j, the input builder and the checks of a launch against them.  Not a test module.

The definition.  Output j of a row x of n samples read at `step`, c = min(1, 1 / step): x_j = j step; for i ascending over max(0, ceil(x_j - Z / c)) ..
min(n - 1, floor(x_j + Z / c)): u = |x_j - i| c L (skipped if u >= Z L), k = floor(u), a = u - k, w = a (H[k + 1] - H[k]) + H[k], y[j] = c sum_i w x[i].  The
kernel takes a as an fp32 value, forms w by one fp32 subtraction and one fmaf, accumulates by fmaf in that order from 0 and multiplies by (float)c.

The bound, per element: |y - y64[j]| <= (T + 3) 2^-24 S_j + 2^-23 D_j + 2^-24 |y64[j]|, with S_j = c sum_i |w_i| |x_i|, D_j = c sum_i |H[k_i + 1] - H[k_i]| |x_i| and
T = floor(2 Z / c) + 2, the most taps an output of the row can have (|x_j - i| < Z / c admits at most floor(2 Z / c) + 1 integers; one more for the rounding of
x_j +- Z / c).  First order, term by term:
  * w: the fp32 difference d = H[k + 1] - H[k] errs by at most 2^-24 |d|, a = fl32(u - k) < 1 by at most 2^-25, so a d errs by at most (2^-24 + 2^-25) |d| <= 2^-23
    |d| -- summed over the taps against |x_i| and scaled by c that is 2^-23 D_j; the fmaf that forms w rounds once more, 2^-24 |w|, in sum 2^-24 S_j;
  * the chain: each of the <= T fmaf rounds its partial sum, whose magnitude is at most sum |w_i| |x_i|, by 2^-24: T 2^-24 S_j; the product with c rounds once more,
    2^-24 |y| <= 2^-24 S_j.  That is (T + 2) 2^-24 S_j; one more unit covers every second-order term (the products of two of the above, each below 2^-24 of a
    first-order term, and the fp64 arithmetic of u, whose 2^-53 moves w by less than 2^-44 |d| L because h is continuous);
  * (float)c differs from c by at most 2^-24 c: 2^-24 |y64|, the last term.
Derived, not measured; an off-by-one tap or a table index one step off misses it by orders of magnitude (a table step changes w by about 1 / L = 2^-8)."""
import ctypes
import math

import numpy as np
import torch

EPS = 2.0 ** -24
Z, L, BETA = 16, 256, 9.0
SEMITONES = (-12, -6, -1, 0.5, 3.3, 6, 12)
_TAB = {}


def ratio(p):
    return 2.0 ** (float(p) / 12.0)


def h_exact(t):
    """h(t) = sinc(t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta) for |t| < Z, else 0, in fp64"""
    t = np.abs(np.asarray(t, np.float64))
    win = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / Z) ** 2))) / np.i0(BETA)
    return np.where(t < Z, np.sinc(t) * win, 0.0)


def table():
    """H[k] = h(k / L) as fp32, k = 0 .. Z L + 1; H[0] = 1, exact zeros at every other multiple of L and from Z L on"""
    if "H" not in _TAB:
        h = h_exact(np.arange(Z * L + 2, dtype=np.float64) / L)
        h[0] = 1.0
        h[L::L] = 0.0
        h[Z * L:] = 0.0
        _TAB["H"] = h.astype(np.float32)
    return _TAB["H"]


def taps(step):
    c = min(1.0, 1.0 / float(step))
    return int(math.floor(2 * Z / c)) + 2


def restate(x, step, N, H=None):
    """The definition in fp64 on the fp32 table -> (y64, S, D), N outputs each"""
    H = (table() if H is None else np.asarray(H)).astype(np.float64)
    x = np.asarray(x, np.float64)
    n, step = len(x), float(step)
    c = min(1.0, 1.0 / step)
    half = Z / c
    pos = np.arange(N, dtype=np.float64) * step
    lo = np.maximum(0.0, np.ceil(pos - half)).astype(np.int64)
    hi = np.minimum(float(n - 1), np.floor(pos + half)).astype(np.int64)
    acc, S, D = np.zeros(N), np.zeros(N), np.zeros(N)
    assert N == 0 or int((hi - lo).max()) + 1 <= taps(step), "more taps than the bound's T"
    for t in range(taps(step)):
        i = lo + t
        u = np.abs(pos - i.astype(np.float64)) * c * L
        ok = (i <= hi) & (u < Z * L)
        k = np.where(ok, u, 0.0).astype(np.int64)
        a = np.where(ok, u, 0.0) - k
        d = H[k + 1] - H[k]
        w = a * d + H[k]
        xv = np.where(ok, x[np.clip(i, 0, max(n - 1, 0))] if n else 0.0, 0.0)
        w, d = np.where(ok, w, 0.0), np.where(ok, d, 0.0)
        acc += w * xv
        S += np.abs(w) * np.abs(xv)
        D += np.abs(d) * np.abs(xv)
    return c * acc, c * S, c * D


def check_bound(y, x, step, what=""):
    """the fp32 result against the restatement, every element; -> the worst error as a fraction of its bound"""
    y = np.asarray(y)
    assert y.dtype == np.float32, (what, y.dtype)
    y64, S, D = restate(x, step, len(y))
    if not len(y):
        return 0.0
    bound = (taps(step) + 3) * EPS * S + 2.0 * EPS * D + EPS * np.abs(y64)
    err = np.abs(y.astype(np.float64) - y64)
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err - bound)))
    assert np.all(err <= bound), f"{what}: element {worst} of {len(y)}: |y - y64| = {err[worst]:.3e} > {bound[worst]:.3e} (y {y[worst]!r}, y64 {y64[worst]!r})"
    return float(np.max(err / np.maximum(bound, 1e-300)))


# ----------------------------------------------------------------------------- CPU checks of the oracle itself
def check_table(tab):
    """the project's table is the formula's, and its linear interpolation is within pi^2 / (8 L^2) + 2^-24 of the exact h: the interpolation error of a function
    whose second derivative is bounded by pi^2 (sinc's; the window is at most 1 and flat against it) over steps of 1 / L, plus the fp32 rounding of a value <= 1"""
    H = table()
    assert np.asarray(tab).dtype == np.float32 and np.array_equal(np.asarray(tab), H) and H.shape == (Z * L + 2,)
    assert H[0] == 1.0 and not H[L::L].any() and not H[Z * L:].any()
    t = np.random.default_rng(0).uniform(0.0, Z, 200000)
    u = t * L
    k = u.astype(np.int64)
    w = (u - k) * (H[k + 1].astype(np.float64) - H[k]) + H[k]
    err = float(np.abs(w - h_exact(t)).max())
    assert err <= math.pi ** 2 / (8 * L * L) + EPS, err
    return err


def check_sine(p, H=None, f=1000.0, n=9600):
    """the restatement (on the table H: the project's) moves a sine of f Hz to f r Hz: away from the ends the result is sin(2 pi f r j / 24000) to better than
    90 dB -- Kaiser's design formula gives a window of beta = 9 a stopband 9 / 0.1102 + 8.7 = 90.4 dB down; unit gain in the pass band"""
    r = ratio(p)
    x = np.sin(2 * np.pi * f * np.arange(n) / 24000.0)
    N = int(n / r)
    y, _, _ = restate(x, r, N, H)
    want = np.sin(2 * np.pi * f * r * np.arange(N) / 24000.0)
    edge = int(2 * Z * max(1.0, r) / r) + 2
    e = (y - want)[edge: N - edge]
    snr = 10 * np.log10(np.mean(want[edge: N - edge] ** 2) / np.mean(e ** 2))
    assert snr >= 90.0, (p, snr)
    return snr


# ----------------------------------------------------------------------------- inputs
def signal(kind, n, seed):
    if kind == "uniform":
        return np.random.default_rng(seed).uniform(-0.99, 0.99, n).astype(np.float32)
    if kind == "sine":  # 3.1 kHz under a slow envelope: a signal the filter passes
        t = np.arange(n)
        return (0.8 * np.sin(2 * np.pi * 3100.0 * t / 24000.0) * (0.6 + 0.4 * np.cos(t / 700.0))).astype(np.float32)
    assert kind == "zeros"
    return np.zeros(n, np.float32)


# name -> [(length, kind)]; A: every short length; B: several workgroups per row at every step; C: its stand-in on the emulator
SETS = {"A": [(1931, "uniform"), (0, "zeros"), (7, "uniform"), (479, "sine"), (480, "uniform"), (1, "uniform")], "B": [(70000, "uniform")], "C": [(2309, "uniform")]}


def build(name, dev, aligned):
    """-> (host rows [np.float32], device views): the rows of SETS[name] as views of ONE padded (R, ld) tensor whose padding holds NaN, so a read outside a row
    shows in the result.  aligned: every row begins on a 16-byte boundary; else row r begins r mod 3 + 1 floats behind one (every 4-byte misalignment)."""
    spec = SETS[name]
    R, nmax = len(spec), max(n for n, _ in spec)
    ld = (nmax + 8 + 3) // 4 * 4
    host = np.full((R, ld), np.nan, np.float32)
    rows, shifts = [], []
    for r, (n, kind) in enumerate(spec):
        sh = 0 if aligned else r % 3 + 1
        x = signal(kind, n, 200 + r)
        host[r, sh: sh + n] = x
        rows.append(x)
        shifts.append(sh)
    big = torch.from_numpy(host).to(dev)
    views = [big[r, sh: sh + n] for r, (sh, (n, _)) in enumerate(zip(shifts, spec))]
    assert big.data_ptr() % 16 == 0
    if not aligned:
        assert {(v.data_ptr() // 4) % 4 for v in views if v.numel()} >= ({1, 2, 3} if R >= 3 else {1})
    return rows, views


def out_lens(rows, step, tail):
    """N per row.  "below": short of n / step, every output has taps inside the row; "above": past it by up to 300 source samples -- the tail reads beyond the
    row's end, as the engine's last frame does (N step - n_src < 480)"""
    if tail == "below":
        return [max(0, int(len(x) / step) - 3) for x in rows]
    return [int(math.ceil((len(x) + 300) / step)) for x in rows]


def check_launch(ops, dev, name, p, aligned, tail, sync=lambda: None):
    """one ops.wave_pitch launch of a set against the restatement: every element of every row within the bound"""
    rows, views = build(name, dev, aligned)
    step = ratio(p)
    N = out_lens(rows, step, tail)
    outs = ops.wave_pitch(views, [step] * len(rows), N)
    sync()
    assert len(outs) == len(rows) and len({o.untyped_storage().data_ptr() for o in outs}) == 1, "R views of one packed buffer"
    worst = 0.0
    for r, (x, o) in enumerate(zip(rows, outs)):
        y = o.cpu().numpy()
        assert y.shape == (N[r],), (name, p, r, y.shape)
        worst = max(worst, check_bound(y, x, step, f"{name} p = {p} {tail} row {r}"))
    return worst


def check_identity(ops, dev, name, aligned, sync=lambda: None):
    """step = 1 returns the input's bits, and zeros past the row's end"""
    rows, views = build(name, dev, aligned)
    N = [len(x) + 5 for x in rows]
    outs = ops.wave_pitch(views, [1.0] * len(rows), N)
    sync()
    for x, o in zip(rows, outs):
        y = o.cpu().numpy()
        assert np.array_equal(y[: len(x)].view(np.int32), x.view(np.int32)) and not y[len(x):].any() and not np.signbit(y[len(x):]).any()


# ----------------------------------------------------------------------------- the raw entry
def raw_args(base, offs, lens, steps, N, tab, out_ptr, out_offs, out_cap, stream, Zs=Z, Ls=L):
    """the argument list of cbx_wave_pitch_f32 and the ctypes arrays it points into (keep them alive)"""
    R = len(lens)
    keep = [(ctypes.c_long * R)(*offs), (ctypes.c_int * R)(*lens), (ctypes.c_double * R)(*steps), (ctypes.c_int * R)(*N), (ctypes.c_long * R)(*out_offs)]
    a = ctypes.addressof
    return [base, a(keep[0]), a(keep[1]), a(keep[2]), a(keep[3]), R, tab, Zs, Ls, out_ptr, a(keep[4]), out_cap, stream], keep


def refused(lib, good):
    """every refused descriptor returns -22 with the entry's name; `good` = raw_args of two rows of 960 samples at offsets 0 and 960, outputs at 3 and 700 of a
    buffer of 1500"""
    a = ctypes.addressof
    neg_len, neg_off, neg_n = (ctypes.c_int * 2)(960, -1), (ctypes.c_long * 2)(0, -4), (ctypes.c_int * 2)(600, -1)
    neg_out, over = (ctypes.c_long * 2)(-1, 700), (ctypes.c_long * 2)(3, 901)
    steps = [(ctypes.c_double * 2)(1.5, v) for v in (0.49, 2.01, float("nan"), float("inf"), -1.0, 0.0)]
    wav = good[0]
    bad = [(0, None), (1, None), (2, None), (3, None), (4, None), (6, None), (9, None), (10, None), (5, 0), (5, -1), (5, 65), (2, a(neg_len)), (1, a(neg_off)),
           (4, a(neg_n)), (10, a(neg_out)), (10, a(over)), (7, 0), (8, 0), (7, -16), (8, 257), (7, 17), (11, 1299), (11, 0),
           (9, wav), (9, wav + 4 * 1916), (9, wav - 4 * 1200)] + [(3, a(s)) for s in steps]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.cbx_wave_pitch_f32(*args) == -22 and b"wave_pitch" in lib.cbx_last_error(), (i, v)
    return neg_len, neg_off, neg_n, neg_out, over, steps


def check_sentinels(ops, dev, p, sync=lambda: None):
    """through the raw entry: an oversized, prefilled output is untouched outside the rows' spans, and the spans hold what ops.wave_pitch returns"""
    rows, views = build("A", dev, aligned=False)
    step = ratio(p)
    N = out_lens(rows, step, "above")
    offs, pos = [], 5
    for c in N:
        offs.append(pos)
        pos += c + 3
    out = torch.full((pos + 9,), 7.0, device=dev)
    base = views[0].untyped_storage().data_ptr()
    args, keep = raw_args(base, [(v.data_ptr() - base) // 4 if v.numel() else 0 for v in views], [len(x) for x in rows], [step] * len(rows), N,
                          ops._pitch_table(dev).data_ptr(), out.data_ptr(), offs, out.numel(), ops._stream())
    assert ops.lib.cbx_wave_pitch_f32(*args) == 0, ops.lib.cbx_last_error()
    ref = ops.wave_pitch(views, [step] * len(rows), N)
    sync()
    o, mask = out.cpu(), torch.ones(out.numel(), dtype=torch.bool)
    for r, (a, c) in enumerate(zip(offs, N)):
        assert torch.equal(o[a: a + c], ref[r].cpu()), (p, r)
        mask[a: a + c] = False
    assert bool((o[mask] == 7.0).all()), "the output buffer is untouched outside the rows"
