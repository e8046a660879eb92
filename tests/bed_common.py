"""Shared by tests/test_bed_host.py (SIMT emulator, CPU tensors), tests/test_bed_kernels_gpu.py and tests/test_bed_api_gpu.py: the oracle of the music bed
(include/cbx.h cbx_wave_duck_f32 / cbx_wave_duck_level_f32) -- the definition's seven steps in NumPy fp64 over the two tables as their fp32
values, written independently of ops --, its float32 restatement, the signal builders, the cases and the check of a launch against the oracle.  Not a test module.

Tolerances.  The float32 restatement (oracle(dtype=np.float32): the same order, a rounded multiply and a rounded add where the kernel uses fmaf) deviates from the
fp64 oracle over every committed case (measure(): all of cases()) by at most
    |dout| / max(|s|, |b L|) = 8.26e-8 -- measured by measure() on the CPU; REF_OUT is that rounded up, and test_bed_host.py asserts that measure() stays within it --,
and the kernel is allowed FACTOR = 4 times that, the factor and the reason of limit_common.py: an fma differs from a multiply-add by at most one rounding, and the
kernel's order is the restatement's.  TOL_OUT = 3.32e-7 (relative to max(|s|, |b L|) of the row).  The activity count, the frame count and the gain in the stats
must match exactly; the peak in the stats is the maximum of the kernel's own output, bit for bit.  L from the level launch: within 2 ulp (fp32) of the oracle's.
Where g is exactly 1 by the definition (duck = 0 dB, a row without an active frame) the output is compared BITWISE against s' + bed' e L evaluated as the kernel
does (oracle(dtype=np.float32, fma=fma32): two rounded products and one exact fused multiply-add, fma32 below)."""
import numpy as np
import torch

import loudness_common as L

FS, Q = 24000, 240
FACTOR = 4.0
REF_OUT = 8.3e-8                          # the float32 restatement against the fp64 oracle (measure())
TOL_OUT = FACTOR * REF_OUT
SPEECH_AMP = 0.3


def linear(db):
    return 10.0 ** (float(db) / 20.0)


def window(S):
    """the limiter's normalised raised cosine for H = S, as the fp32 table holds it"""
    k = np.arange(-S, S + 1, dtype=np.float64)
    w = 0.5 * (1.0 + np.cos(np.pi * k / (S + 1)))
    return (w / w.sum()).astype(np.float32).astype(np.float64)


def seam_ramp(xf):
    """the join's ramp (2 i + 1) / (2 xf), as the fp32 table holds it"""
    return ((2.0 * np.arange(xf, dtype=np.float64) + 1.0) / (2.0 * xf)).astype(np.float32).astype(np.float64)


def fma32(a, b, c):
    """fmaf over float32 arrays: the product is exact in fp64; the sum is rounded to ODD in fp64 (TwoSum gives the error; an inexact sum with an even last bit moves
    to its odd neighbour on the error's side), which makes the final rounding to float32 the correctly rounded one (53 >= 24 + 2 bits)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def oracle(s, b, p, gain=1.0, dtype=np.float64, fma=None):
    """The definition on one row -> dict(sp = s' (float32), act, A, G, g, bed = bed', e, out, N, F, stats = [L, frames with A, F, max |out| (NaN: the row holds
    one)]).  p: dict(duck, threshold (dB), lead, tail, pre, post, S, loop, xf, fi, fo).  dtype = np.float32: the restatement in the kernel's precision; with
    fma=fma32 every fmaf of the kernel is an exact fused multiply-add: the kernel's own arithmetic."""
    madd = fma if fma is not None else (lambda x, y, z: x * y + z)
    s32, b32 = np.asarray(s, np.float32), np.asarray(b, np.float32)
    n, nb, lead, tail = len(s32), len(b32), int(p["lead"]), int(p["tail"])
    N = lead + n + tail
    F = -(-N // Q)
    Lg = dtype(np.float32(gain))
    sp = np.zeros(N, np.float32)
    sp[lead: lead + n] = s32
    if N == 0:
        z = np.zeros(0, dtype)
        return dict(sp=sp, act=np.zeros(0, bool), A=np.zeros(0, bool), G=z, g=z, bed=z, e=z, out=z, N=0, F=0, stats=[float(Lg), 0, 0, 0.0])
    thr, d = np.float32(linear(p["threshold"])), np.float32(linear(p["duck"]))
    pad = np.zeros(F * Q, np.float32)
    pad[:N] = np.abs(sp)
    with np.errstate(invalid="ignore"):
        act = ~(pad.reshape(F, Q).max(axis=1) <= thr)            # (np.max propagates a NaN: the frame is active)
    pre, post, S = int(p["pre"]), int(p["post"]), int(p["S"])
    A = np.array([act[max(0, f - post): f + pre + 1].any() for f in range(F)])
    one_t = np.zeros(F + 2 * S, dtype)
    one_t[S: S + F] = np.where(A, dtype(1) - dtype(d), dtype(0))
    w = window(S).astype(dtype)
    acc = np.zeros(F, dtype)
    for k in range(2 * S + 1):
        acc = madd(np.full(F, w[k], dtype), one_t[k: k + F], acc).astype(dtype)
    G = dtype(1) - acc
    i = np.arange(N, dtype=np.int64)
    j = i - Q // 2
    f0 = j // Q
    a = (j - f0 * Q).astype(dtype) / dtype(240)
    Gl, Gh = G[np.clip(f0, 0, F - 1)], G[np.clip(f0 + 1, 0, F - 1)]
    g = madd(a, Gh - Gl, Gl).astype(dtype)
    bs = b32.astype(dtype)
    bed, end = np.zeros(N, dtype), 0
    if nb > 0 and not p["loop"]:
        end = min(N, nb)
        bed[:end] = bs[:end]
    elif nb > 0:
        xf, end = int(p["xf"]), N
        P = nb - xf
        assert P > xf, "a looped source is longer than twice the cross-fade"
        k, r = i // P, i % P
        bed = bs[r]
        seam = (k > 0) & (r < xf)
        if seam.any():
            rr = r[seam]
            bed[seam] = madd(seam_ramp(xf).astype(dtype)[rr], bs[rr] - bs[P + rr], bs[P + rr]).astype(dtype)
    fi, fo = int(p["fi"]), int(p["fo"])
    up = np.where(i < fi, (i + 1).astype(dtype) / dtype(fi + 1), dtype(1))
    dn = np.where(end - 1 - i < fo, (end - i).astype(dtype) / dtype(fo + 1), dtype(1))
    e = np.where(i < end, up * dn, dtype(0)).astype(dtype)
    with np.errstate(invalid="ignore"):
        v = ((bed * e).astype(dtype) * g).astype(dtype)
        out = madd(v, np.full(N, Lg, dtype), sp.astype(dtype)).astype(dtype)
        peak = float(np.abs(out).max())
    return dict(sp=sp, act=act, A=A, G=G, g=g, bed=bed, e=e, out=out, N=N, F=F, stats=[float(Lg), int(A.sum()), F, peak])


def level_oracle(Ls, Lb, level):
    both = np.isfinite(Ls) and np.isfinite(Lb)
    return np.float32(10.0 ** (((Ls + level - Lb) if both else level) / 20.0))


# ----------------------------------------------------------------------------- the signals
def speech(n, seed, p, first=True, last=False):
    """bursts of amplitude 0.3 (a 200 Hz sine under seeded noise, 150 .. 400 samples) separated by zeros; the gap lengths go round (pre + post) Q -+ 60 and
    (pre + post + 2 S) Q -+ 60: one short of the hold, one beyond it, one short of hold plus smoothing, one beyond that.  first / last: a burst covers the first /
    the last sample (else the row begins / ends with silence)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.float32)
    hold = (int(p["pre"]) + int(p["post"])) * Q
    gaps = [max(1, hold - 60), hold + 60, hold + 2 * int(p["S"]) * Q - 60, hold + 2 * int(p["S"]) * Q + 60]
    pos, k = (0 if first else 130), 0
    while pos < n:
        m = int(rng.integers(150, 400))
        t = np.arange(min(m, n - pos))
        x[pos: pos + m] = (SPEECH_AMP * (0.7 * np.sin(2 * np.pi * 200.0 * t / FS + 1.0) + 0.3 * rng.uniform(-1, 1, len(t)))).astype(np.float32)
        pos += m + gaps[k % 4]
        k += 1
    if last and n:
        x[max(0, n - 100):] = np.float32(SPEECH_AMP * 0.9)
    elif n > 300:
        x[n - 250:] = 0.0
    return x


def bed(n, seed, amp=0.2):
    """a 440 Hz sine plus seeded noise"""
    rng = np.random.default_rng(1000 + seed)
    return (amp * np.sin(2 * np.pi * 440.0 * np.arange(n) / FS) + 0.05 * rng.standard_normal(n)).astype(np.float32)


P0 = dict(duck=-9.0, threshold=-40.0, lead=0, tail=0, pre=1, post=3, S=2, loop=True, xf=48, fi=30, fo=100)
DEFAULT_PLAN = dict(duck=-9.0, threshold=-40.0, lead=0, tail=0, pre=10, post=30, S=12, loop=True, xf=2400, fi=480, fo=12000)   # ops.BED_DEFAULTS in samples and frames
GROUPS = ((0, 1, 3333), (239, 240, 241), (1023, 1024, 1025), (2051, 0, 11))   # every length; an empty row first, in the middle and last
N = 2051


def plan(**kw):
    return dict(P0, **kw)


def cases():
    """name -> dict(speech, bed (per row), plan, gain (per row, or None: no gain vector)).  Every case but `defaults` is R <= 3 rows of at most 4400 outputs."""
    out = {}
    for g, lens in enumerate(GROUPS):
        p = plan(S=1 + g % 2, pre=(0, 1, 3)[g % 3], post=(3, 0, 1)[g % 3])
        out[f"lengths{g}"] = dict(speech=[speech(n, 20 + n, p) for n in lens], bed=[bed(700 + 13 * r, r) for r in range(3)], plan=p, gain=[0.25, 0.5, 1.0])
    for lead in (0, 1, 239, 241, 1000):
        p = plan(lead=lead, tail=37, pre=3, post=1, S=1)
        out[f"lead{lead}"] = dict(speech=[speech(1100, 3, p), speech(500, 4, p, last=True)], bed=[bed(900, 1), bed(301, 2)], plan=p, gain=[0.5, 0.7])
    out["empty_bed"] = dict(speech=[speech(N, 5, P0), speech(1025, 6, P0)], bed=[np.zeros(0, np.float32), bed(700, 3)], plan=P0, gain=[0.5, 0.5])
    out["no_bed"] = dict(speech=[speech(N, 5, P0), speech(0, 6, P0)], bed=None, plan=plan(lead=7), gain=None)
    out["long_bed_loop"] = dict(speech=[speech(N, 7, P0)], bed=[bed(5000, 4)], plan=P0, gain=[0.5])
    out["long_bed_once"] = dict(speech=[speech(N, 7, P0)], bed=[bed(5000, 4)], plan=plan(loop=False), gain=[0.5])
    out["seam_tile_edge"] = dict(speech=[speech(3333, 8, P0)] * 3, bed=[bed(1024, 5), bed(1023 + 48, 6), bed(1025 + 48, 7)], plan=P0, gain=[0.5] * 3)   # P = 1024 - xf, 1023, 1025
    out["seam_frame_edge"] = dict(speech=[speech(3333, 8, P0)], bed=[bed(960 + 48, 5)], plan=P0, gain=None)   # P = 4 Q
    out["seam_no_fade"] = dict(speech=[speech(N, 8, P0)], bed=[bed(1024, 5)], plan=plan(xf=0), gain=[0.5])
    out["short_bed_once"] = dict(speech=[speech(3333, 9, P0), speech(1500, 10, P0)], bed=[bed(1500, 8), bed(1, 9)], plan=plan(loop=False), gain=[0.5, 0.5])
    out["long_fades"] = dict(speech=[speech(N, 11, P0), speech(700, 12, P0)], bed=[bed(900, 10), bed(2500, 11)], plan=plan(fi=5000, fo=5000), gain=[0.5, 1.0])
    out["long_fades_once"] = dict(speech=[speech(N, 11, P0)], bed=[bed(900, 10)], plan=plan(fi=5000, fo=5000, loop=False), gain=[0.5])
    p = plan(pre=3, post=3, S=2)
    out["first_last_frames"] = dict(speech=[speech(N, 13, p, first=True, last=True), speech(1276, 14, p, first=False, last=True), speech(1276, 15, p, first=True)],
                                    bed=[bed(800, 12)] * 3, plan=p, gain=[0.5] * 3)
    x = speech(N, 16, P0)
    x[700] = np.nan
    out["nan_sample"] = dict(speech=[speech(1025, 17, P0), x, speech(1276, 18, P0)], bed=[bed(800, 13)] * 3, plan=P0, gain=[0.5] * 3)
    out["duck_0db"] = dict(speech=[speech(N, 19, P0), speech(1025, 20, P0)], bed=[bed(800, 14), bed(1100, 15)], plan=plan(duck=0.0), gain=[0.5, 0.3], exact=True)
    out["silent_speech"] = dict(speech=[np.zeros(N, np.float32), np.full(1025, 0.009, np.float32)], bed=[bed(800, 14), bed(1100, 15)], plan=P0, gain=[0.5, 0.3], exact=True)
    out["gain_zero"] = dict(speech=[speech(N, 21, P0), speech(1025, 22, P0)], bed=[bed(800, 16), bed(1100, 17)], plan=P0, gain=[0.0, 0.0])
    out["defaults"] = dict(speech=[speech(24000, 23, DEFAULT_PLAN)], bed=[bed(9000, 18)], plan=DEFAULT_PLAN, gain=[0.25])
    return out


def _beds(case):
    return [np.zeros(0, np.float32)] * len(case["speech"]) if case["bed"] is None else case["bed"]


def _scale(s, b, gain):
    return max(float(np.nanmax(np.abs(s), initial=0.0)), float(np.abs(b).max(initial=0.0)) * abs(float(np.float32(gain))), 1e-30)


def measure():
    """max |dout| / max(|s|, |b L|) of the float32 restatement against the fp64 oracle over every row of cases()"""
    worst = 0.0
    for name, c in cases().items():
        for r, (s, b) in enumerate(zip(c["speech"], _beds(c))):
            gain = 1.0 if c["gain"] is None else c["gain"][r]
            a, f = oracle(s, b, c["plan"], gain), oracle(s, b, c["plan"], gain, np.float32)
            if a["N"]:
                assert np.array_equal(a["A"], f["A"])
                worst = max(worst, float(np.nanmax(np.abs(a["out"] - f["out"]), initial=0.0)) / _scale(s, b, gain))
    return worst


# ----------------------------------------------------------------------------- a launch against the oracle
def check_row(name, r, s, b, p, gain, got, st, exact=False):
    """the output `got` and the stats row `st` of a launch over (s, b) against the fp64 oracle.  Returns the oracle's dict."""
    ref = oracle(s, b, p, gain)
    assert len(got) == ref["N"], f"{name} row {r}: {len(got)} outputs, the definition gives {ref['N']}"
    assert st[0] == ref["stats"][0] and st[1] == ref["stats"][1] and st[2] == ref["stats"][2], f"{name} row {r}: stats {list(st)}, oracle {ref['stats']}"
    if ref["N"] == 0:
        assert st[3] == 0.0
        return ref
    scale = _scale(s, b, gain)
    bad = np.isnan(ref["out"])
    assert np.array_equal(np.isnan(got), bad), f"{name} row {r}: NaNs where the oracle has them, and nowhere else"
    err = float(np.abs(got.astype(np.float64) - ref["out"])[~bad].max(initial=0.0)) / scale
    print(f"{name} row {r}: N {ref['N']} F {ref['F']} ducked {ref['stats'][1]} scale {scale:.4g} |dout|/scale {err:.3g} (allowed {TOL_OUT:.3g}) stats {list(st)} oracle {ref['stats']}")
    assert err <= TOL_OUT, f"{name} row {r}: out deviates from the oracle by {err:.3g} of the scale, allowed {TOL_OUT:.3g}"
    if bad.any():
        assert np.isnan(st[3]), f"{name} row {r}: the peak of a row with a NaN is NaN, got {st[3]}"
    else:
        assert st[3] == float(np.abs(got).max()), f"{name} row {r}: the peak {st[3]!r} is the maximum of the output, {float(np.abs(got).max())!r}"
    if exact:
        assert np.all(ref["g"] == 1.0), f"{name} row {r}: the case has g == 1 everywhere"
        want = oracle(s, b, p, gain, np.float32, fma32)["out"]
        assert np.array_equal(got, want), f"{name} row {r}: with g == 1 the output is s' + bed' e L bit for bit"
    if float(np.float32(gain)) == 0.0 or len(b) == 0:
        nz = got != 0
        assert np.array_equal(got[nz].view(np.int32), ref["sp"][nz].view(np.int32)) and not np.any(ref["sp"][~nz] != 0), f"{name} row {r}: without a bed the output is s' bit for bit"
    return ref


def _rows(signals, mis, device):
    return L.padded_rows(signals, mis, device)


def launch(ops, case, mis, device="cpu", sync=lambda: None, out=True):
    """One wave_duck over the case's rows: speech as views of one NaN-padded buffer at misalignment mis, the beds of another at mis + 2, into rows of a third at
    mis + 1 (out=False: into the allocation wave_duck makes).  Returns (outputs, stats, (buffers before / after for the caller's checks))."""
    sp, bd, p = case["speech"], _beds(case), case["plan"]
    sbuf, srows, _ = _rows(sp, mis, device)
    bbuf, brows, _ = _rows(bd, mis + 2, device)
    obuf, orows, ospans = _rows([np.zeros(len(s) + p["lead"] + p["tail"], np.float32) for s in sp], mis + 1, device)
    gain = None if case["gain"] is None else torch.tensor(case["gain"], dtype=torch.float32).to(device)
    before = (sbuf.cpu().numpy().copy(), bbuf.cpu().numpy().copy())
    o, stats = ops.wave_duck(srows, None if case["bed"] is None else brows, p, gain=gain, out=orows if out else None)
    sync()
    assert np.array_equal(sbuf.cpu().numpy(), before[0], equal_nan=True) and np.array_equal(bbuf.cpu().numpy(), before[1], equal_nan=True), "speech and bed are only read"
    return [w.cpu().numpy() for w in o], stats.cpu().numpy(), (obuf, ospans)


def run_case(ops, name, case, mis, device="cpu", sync=lambda: None):
    """launch() against the oracle, the padding of `out` still NaN.  Returns (outputs, stats) as host arrays."""
    got, st, (obuf, ospans) = launch(ops, case, mis, device, sync)
    assert st.shape == (len(got), 4) and st.dtype == np.float64
    after = obuf.cpu().numpy()
    keep = np.ones(len(after), bool)
    for r, ((a, b), s, bb) in enumerate(zip(ospans, case["speech"], _beds(case))):
        keep[a:b] = False
        assert np.array_equal(after[a:b], got[r], equal_nan=True)
        check_row(name, r, s, bb, case["plan"], 1.0 if case["gain"] is None else case["gain"][r], got[r], st[r], exact=case.get("exact", False))
    assert np.isnan(after[keep]).all(), f"{name}: nothing outside the rows of out is written"
    return got, st


def check_nan_row(ops, device="cpu", sync=lambda: None):
    """one NaN sample: its frame is active, the output holds the NaN at that sample alone, the peak reads NaN -- and the rows beside it are what they are alone"""
    case = cases()["nan_sample"]
    got, st = run_case(ops, "nan_sample", case, 1, device, sync)
    ref = oracle(case["speech"][1], case["bed"][1], case["plan"], 0.5)
    assert ref["act"][700 // Q] and np.isnan(got[1][700]) and np.isnan(got[1]).sum() == 1 and np.isnan(st[1, 3]) and not np.isnan(st[[0, 2], 3]).any()
    clean = dict(case, speech=[case["speech"][0], np.nan_to_num(case["speech"][1]), case["speech"][2]])
    other, _, _ = launch(ops, clean, 1, device, sync)
    assert np.array_equal(other[0], got[0]) and np.array_equal(other[2], got[2]), "the rows beside the NaN are unaffected"


def check_determinism(ops, device="cpu", sync=lambda: None):
    """the same rows at two misalignments, into an allocation of the caller's or of wave_duck's, and as R = 1 calls against one R = 3 call: bit for bit equal"""
    p = plan(lead=241, tail=100)
    case = dict(speech=[speech(3333, 30, p), speech(N, 31, p), speech(1025, 32, p)], bed=[bed(1071, 20), bed(700, 21), bed(4000, 22)], plan=p, gain=[0.5, 0.25, 1.0])
    a, sa, _ = launch(ops, case, 0, device, sync)
    b, sb, _ = launch(ops, case, 3, device, sync)
    c, sc, _ = launch(ops, case, 2, device, sync, out=False)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c)) and np.array_equal(sa, sb) and np.array_equal(sa, sc), "the result does not depend on the rows' alignment"
    for r in range(3):
        one = dict(speech=[case["speech"][r]], bed=[case["bed"][r]], plan=p, gain=[case["gain"][r]])
        d, sd, _ = launch(ops, one, 1, device, sync)
        assert np.array_equal(d[0], a[r]) and np.array_equal(sd[0], sa[r]), "a row alone is the row in the batch"


def check_gain_null(ops, device="cpu", sync=lambda: None):
    case = cases()["lengths2"]
    a, sa, _ = launch(ops, dict(case, gain=None), 1, device, sync)
    b, sb, _ = launch(ops, dict(case, gain=[1.0, 1.0, 1.0]), 1, device, sync)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(sa, sb), "gain = NULL is a gain of ones, bit for bit"


def check_ducking(ops, device="cpu", sync=lambda: None):
    """what the step is for: under a long burst the bed sits at d, far from speech at 1, and g never leaves [d, 1]"""
    p = plan(pre=1, post=3, S=2, fi=0, fo=0)
    s = np.zeros(6000, np.float32)
    s[1000:2500] = SPEECH_AMP
    b = np.ones(700, np.float32)
    got, st, _ = launch(ops, dict(speech=[np.zeros(6000, np.float32)], bed=[b], plan=p, gain=None), 0, device, sync)
    assert np.array_equal(got[0], np.ones(6000, np.float32)) and st[0, 1] == 0
    got, st, _ = launch(ops, dict(speech=[s], bed=[b], plan=p, gain=None), 0, device, sync)
    g, d = got[0] - s, np.float32(linear(-9.0))
    assert abs(float(g[1750]) - float(d)) < 1e-6 and g[5500] == 1.0 and g[0] == 1.0 and g.min() >= d - 1e-6 and g.max() <= 1.0
    assert st[0, 1] == 7 + 1 + 3, "the burst's 7 frames (1000 .. 2499 meets frames 4 .. 10), pre 1 before, post 3 after"


def check_many_rows(ops, device="cpu", sync=lambda: None):
    """R = 64, the most rows a call takes, two tiles each: every row against the oracle"""
    p = plan(lead=5)
    case = dict(speech=[speech(1100 + r, 100 + r, p) for r in range(64)], bed=[bed(300 + 11 * r, r) for r in range(64)], plan=p, gain=[0.1 + 0.01 * r for r in range(64)])
    run_case(ops, "many_rows", case, 2, device, sync)


def check_level(ops, device="cpu", sync=lambda: None):
    """the level launch against 10^((Ls + level - Lb) / 20) in fp64: within 2 ulp of fp32; a reading that is not finite: the level alone"""
    Ls = [-23.1, -30.25, float("-inf"), -19.0, float("nan"), -16.5]
    Lb = [-14.7, -8.5, -20.0, float("-inf"), -20.0, -41.25]
    lv = [-12.0, -6.0, -12.0, -18.5, 0.0, 3.0]
    ss = torch.tensor([[a, 0.5, 1.0, 9.0] for a in Ls], dtype=torch.float64).to(device)
    sb = torch.tensor([[a, 0.25, 1.0, 7.0] for a in Lb], dtype=torch.float64).to(device)
    g = ops.wave_duck_level(ss, sb, lv)
    sync()
    g = g.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == (6,)
    for r in range(6):
        want = level_oracle(Ls[r], Lb[r], lv[r])
        print(f"level row {r}: {g[r]!r}, oracle {want!r}")
        assert abs(float(g[r]) - float(want)) <= 2.0 * float(np.spacing(want)), (r, g[r], want)
    assert np.array_equal(ops.wave_duck_level(ss[:2], sb[:2], -12.0).cpu().numpy(), ops.wave_duck_level(ss[:2], sb[:2], [-12.0, -12.0]).cpu().numpy())


def check_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    """Every -22 case of the two entries, each with the entry's name in cbx_last_error and nothing written; then (run_good) the good descriptor runs: rc 0 and the
    oracle's output"""
    import ctypes
    s0, b0, p = speech(1276, 3, P0), bed(700, 1), P0
    s, b = torch.from_numpy(s0).to(device), torch.from_numpy(b0).to(device)
    out = torch.full((1276,), 7.0, dtype=torch.float32, device=device)
    stats = torch.full((1, 4), 7.0, dtype=torch.float64, device=device)
    ws = torch.zeros(6 + 8, dtype=torch.float32, device=device)
    gain = torch.full((1,), 0.5, dtype=torch.float32, device=device)
    win = torch.from_numpy(ops.limit_window(p["S"])).to(device)
    ramp = ops.join_ramp(p["xf"], torch.device(device))
    A = ctypes.addressof
    off, ln, bl = (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(1276), (ctypes.c_int * 1)(700)
    neg_off, neg_len, far_off, short, none = (ctypes.c_long * 1)(-1), (ctypes.c_int * 1)(-1), (ctypes.c_long * 1)(1), (ctypes.c_int * 1)(96), (ctypes.c_int * 1)(0)
    good = dict(s=s.data_ptr(), soff=A(off), slen=A(ln), b=b.data_ptr(), boff=A(off), blen=A(bl), R=1, gain=gain.data_ptr(), lead=0, tail=0, thr=linear(p["threshold"]),
                duck=linear(p["duck"]), pre=p["pre"], post=p["post"], S=p["S"], win=win.data_ptr(), loop=1, xf=p["xf"], ramp=ramp.data_ptr(), fi=p["fi"], fo=p["fo"],
                out=out.data_ptr(), ooff=A(off), ocap=1276, stats=stats.data_ptr(), ws=ws.data_ptr(), cap=ws.numel())
    keys = ("s", "soff", "slen", "b", "boff", "blen", "R", "gain", "lead", "tail", "thr", "duck", "pre", "post", "S", "win", "loop", "xf", "ramp", "fi", "fo", "out", "ooff",
            "ocap", "stats", "ws", "cap")
    call = lambda d: lib.cbx_wave_duck_f32(*[d[k] for k in keys], stream)
    bad = [dict(good, **{k: None}) for k in ("s", "soff", "slen", "b", "boff", "blen", "win", "ramp", "out", "ooff", "stats", "ws")]
    bad += [dict(good, R=0), dict(good, R=65), dict(good, slen=A(neg_len)), dict(good, soff=A(neg_off)), dict(good, blen=A(neg_len)), dict(good, boff=A(neg_off)),
            dict(good, ooff=A(neg_off)), dict(good, lead=-1), dict(good, tail=-1), dict(good, lead=1 << 31), dict(good, lead=(1 << 31) - 1000, ocap=1 << 40),
            dict(good, thr=0.0), dict(good, thr=-1.0), dict(good, thr=float("inf")), dict(good, thr=float("nan")), dict(good, thr=1e-60),
            dict(good, duck=0.0), dict(good, duck=1.5), dict(good, duck=float("nan")), dict(good, duck=1e-60), dict(good, pre=-1), dict(good, pre=201), dict(good, post=-1),
            dict(good, post=201), dict(good, S=0), dict(good, S=101), dict(good, loop=2), dict(good, loop=-1), dict(good, xf=-1), dict(good, xf=24001), dict(good, fi=-1),
            dict(good, fi=24001), dict(good, fo=-1), dict(good, fo=24001), dict(good, blen=A(short)), dict(good, xf=350), dict(good, ocap=1275), dict(good, ooff=A(far_off)),
            dict(good, lead=1), dict(good, out=s.data_ptr()), dict(good, out=s.data_ptr() + 4 * 1275, ocap=1 << 20), dict(good, out=b.data_ptr() + 4 * 699, ocap=1 << 20),
            dict(good, cap=13)]
    for d in bad:
        assert call(d) == -22 and b"wave_duck" in lib.cbx_last_error(), d
    st2 = torch.zeros(1, 4, dtype=torch.float64, device=device)
    lv, nan_lv = (ctypes.c_double * 1)(-12.0), (ctypes.c_double * 1)(float("nan"))
    lgood = dict(a=st2.data_ptr(), b=st2.data_ptr(), lv=A(lv), R=1, g=gain.data_ptr())
    lcall = lambda d: lib.cbx_wave_duck_level_f32(d["a"], d["b"], d["lv"], d["R"], d["g"], stream)
    for d in [dict(lgood, **{k: None}) for k in ("a", "b", "lv", "g")] + [dict(lgood, R=0), dict(lgood, R=65), dict(lgood, lv=A(nan_lv))]:
        assert lcall(d) == -22 and b"wave_duck_level" in lib.cbx_last_error(), d
    sync()
    assert float(stats.min()) == 7.0 and float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(ws.abs().max()) == 0.0 and float(gain[0]) == 0.5 \
        and np.array_equal(s.cpu().numpy(), s0) and np.array_equal(b.cpu().numpy(), b0), "a refusal writes nothing"
    if run_good:
        assert call(good) == 0
        sync()
        check_row("good", 0, s0, b0, p, 0.5, out.cpu().numpy(), stats.cpu().numpy()[0])
        assert call(dict(good, b=None, blen=A(none), ramp=None, loop=0)) == 0, "no bed at all: bed and ramp NULL"
        sync()
        assert np.array_equal(out.cpu().numpy()[s0 != 0], s0[s0 != 0])
