"""Shared by tests/test_vocoder_edges_gpu.py (-m gpu) and tests/test_simt_kernels.py (SIMT emulator, CPU tensors): the HiFT tail kernels -- source, STFT, iSTFT
(chatterbox_amd/csrc/hift.hip) -- and the elementwise kernels the vocoder calls, at the shapes and values that can break them, and the implicit-GEMM convolution
at every geometry x dispatch form the vocoder reaches, ragged rows included.  Bodies take (ops, dev).  Not a test module.

References are fp64 (torch.istft / torch.stft / F.conv1d / F.conv_transpose1d on the row CUT to its own length); padding the kernels must not read holds NaN.

The iSTFT bound, per sample m (include/cbx.h cbx_hift_istft_rows_f32):
    |y_m - ref_m| <= c 2^-24 S_m / env_m + 2^-24 |ref_m|
    S_m   = sum over the frames t that reach m and the 16 bins f of the full (Hermitian) spectrum of |mag[t][f]| w[q - 4 t] / 16  (q = m + 8),
    env_m = sum over the same frames of w[q - 4 t]^2,
both computed here in fp64 from the formula.  S_m / env_m is the largest value the sample can take, so c counts the fp32 roundings (exp, sin, cos, the 16-term
sum, the window products, the division) an implementation spends per term.  c is not derived but MEASURED on torch's own fp32 torch.istft against fp64 on the very
inputs of this file (CPU, measure_torch_fp32_ratio() below: the rule of test_ops_gpu.py::test_gelu_erf_accuracy, "not worse than torch's own fp32"):
    C_TORCH_FP32 = 4.72  (worst (|err| - 2^-24 |ref|) / (2^-24 S / env) over the geometry set, the value case and the ragged case; measured 4.713:
                          4.70 at frames 361, 4.71 on the value case, 0.35 .. 0.46 at frames 2)
and the kernel is allowed twice that (the device's expf / sinf / cosf are a different libm feeding 9 bins): ISTFT_C = 2 C_TORCH_FP32.
The kernel's own worst ratio, same measure: SIMT emulator (host libm) 1.73 geometry / 1.69 ragged / 0.96 value case; first run on the MI355X 1.74 (frames 361, B 3) /
1.69 / 1.02 (profiles/vocoder_edges_measure.log) -- a third of torch's own fp32 (the kernel's 9-bin direct sum is shorter than a 16-point FFT plus a separate overlap-add)."""
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
C_TORCH_FP32 = 4.72
ISTFT_C = 2.0 * C_TORCH_FP32
NAN = float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed)) * scale


# ----------------------------------------------------------------------------------------------------------------- iSTFT
ISTFT_FRAMES = (2, 3, 17, 65, 66, 121, 361)  # out_len 4, 8, 64, 256 (one full workgroup), 260 (a 4-sample tail), 480 (< 960: the fade is longer than the row), 1440
_W64 = torch.hann_window(16, periodic=True, dtype=torch.float64)


def _fade_table():
    """O.trim_fade's 960-sample table (first 480 silenced, then the raised cosine of torch.linspace in fp32), as fp64"""
    tf = torch.zeros(960)
    tf[480:] = (torch.cos(torch.linspace(math.pi, 0, 480)) + 1) / 2
    return tf.double()


def istft_reference(x, fade_n=0, clamp=0.99):
    """x (n, >= 18) fp32, one row ALREADY CUT to its n frames -> (ref, bound1) fp64 of 4 (n - 1) samples: torch.istft in fp64 of exp(.).clip(100) e^{i sin(.)},
    the clamp, O.trim_fade cut to the row; bound1 = S_m / env_m; clipped = the samples the clamp changed."""
    assert fade_n in (0, 480)
    xd = x[:, :18].double()
    n = xd.shape[0]
    mag, ph = torch.exp(xd[:, :9]).clamp(max=100.0), torch.sin(xd[:, 9:])
    spec = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)).t()[None]
    y = torch.istft(spec, 16, 4, 16, window=_W64)[0]
    L = 4 * (n - 1)
    assert y.shape == (L,)
    # S and env from the formula: frame t adds to padded positions 4 t .. 4 t + 15, sample m sits at padded position m + 8
    a = (mag[:, 0] + mag[:, 8] + 2.0 * mag[:, 1:8].sum(1)) / 16.0  # sum over the 16 bins of |X_f| / 16
    S, env = torch.zeros(4 * n + 12, dtype=torch.float64), torch.zeros(4 * n + 12, dtype=torch.float64)
    for k in range(16):
        S[k: k + 4 * n: 4] += a * _W64[k]
        env[k: k + 4 * n: 4] += _W64[k] ** 2
    b1 = S[8: 8 + L] / env[8: 8 + L]
    clipped = y.abs() > clamp
    y = y.clamp(-clamp, clamp)
    if fade_n:
        g = _fade_table()[:L]
        y[: 2 * fade_n] *= g  # (b1 stays: the gain is itself an fp32 (cos + 1) / 2 on both sides, wrong by up to 2^-25 of the UNFADED sample)
    return y, b1, clipped


def istft_ratio(got, ref, b1):
    """(|got - ref| - 2^-24 |ref|) / (2^-24 S / env), elementwise: what ISTFT_C bounds"""
    return ((got.double() - ref).abs() - EPS * ref.abs()) / (EPS * b1).clamp(min=1e-300)


def _check_istft_row(got, x_cut, fade_n, what, tight=False):
    ref, b1, _ = istft_reference(x_cut, fade_n)
    assert torch.isfinite(got).all(), f"{what}: NaN or inf in the output"
    err = (got.double() - ref).abs()
    bound = ISTFT_C * EPS * b1 + EPS * ref.abs()
    worst = int(torch.argmax(err - bound)) if len(err) else 0
    assert bool((err <= bound).all()), f"{what}: sample {worst}: |y - ref| = {float(err[worst]):.3e} > {float(bound[worst]):.3e} (y {float(got[worst])!r}, ref {float(ref[worst])!r})"
    if tight:  # inputs in the range of test_ops_gpu.py::test_hift_source_stft_istft: its tolerance stays
        assert bool((err <= 1e-5 * (1 + ref.abs())).all()), f"{what}: over 1e-5 (1 + |ref|): {float(err.max()):.3e}"
    r = istft_ratio(got, ref, b1)
    return float(r.max()) if len(r) else 0.0


def istft_input(B, frames, ldx, seed, dev=None):
    """(x (B, frames, ldx) with columns 18.. NaN): log-magnitudes 1.5 N(0, 1) - 1, phases N(0, 1) -- the range of test_hift_source_stft_istft"""
    x = torch.full((B, frames, ldx), NAN)
    v = _randn((B, frames, 18), seed)
    v[:, :, :9] = v[:, :, :9] * 1.5 - 1.0
    x[:, :, :18] = v
    return x


def check_istft_geometry(ops, dev, frames, B, ldx):
    """One (frames, B, ldx) of the geometry set, fade_n = 0 and 480, against fp64 torch.istft within the bound AND within the existing 1e-5 (1 + |ref|); the output
    buffer is one sample longer per call than the kernel may write (NaN sentinel).  Returns the worst ratio to the bound's first term.
    Worst ratios of the kernel: emulator 1.73, MI355X 1.74 (both at frames 361); per case in the module docstring."""
    x = istft_input(B, frames, ldx, 100 + frames)
    xd = x.to(dev)
    L, worst = 4 * (frames - 1), 0.0
    for fade_n in (0, 480):
        buf = torch.full((B * L + 1,), NAN, device=dev)
        wav = buf[: B * L].view(B, L)
        ops.hift_istft(xd, wav, fade_n=fade_n)
        assert math.isnan(float(buf[-1])), "a write past the last row"
        got = wav.cpu()
        for b in range(B):
            worst = max(worst, _check_istft_row(got[b], x[b], fade_n, f"frames {frames} B {B} ldx {ldx} fade {fade_n} row {b}", tight=True))
    return worst


RAGGED_FRAMES, RAGGED_LENS = 121, (121, 61, 2)


def ragged_istft_input():
    x = istft_input(3, RAGGED_FRAMES, 32, 77)
    for b, n in enumerate(RAGGED_LENS):
        x[b, n:] = NAN
    return x


def check_istft_ragged(ops, dev):
    """B = 3, frames = 121, frame_lens = [121, 61, 2]; NaN in columns 18 .. 31 and in every frame at or beyond frame_lens[b].  Every row's valid samples are
    torch.equal to a solo launch on the cut row (a sample depends on nothing but its own row) and within the bound of fp64 torch.istft of the cut row; every sample
    beyond the row is == 0.  On the kernel without frame_lens the last three samples of rows 1 and 2 are NaN here (the frame after the row)."""
    x = ragged_istft_input()
    xd, fl = x.to(dev), torch.tensor(RAGGED_LENS, dtype=torch.int32, device=dev)
    L, worst = 4 * (RAGGED_FRAMES - 1), 0.0
    for fade_n in (0, 480):
        wav = torch.full((3, L), NAN, device=dev)
        ops.hift_istft(xd, wav, fade_n=fade_n, frame_lens=fl)
        got = wav.cpu()
        for b, n in enumerate(RAGGED_LENS):
            Lb = 4 * (n - 1)
            solo = torch.full((1, Lb), NAN, device=dev)
            ops.hift_istft(xd[b: b + 1, :n].contiguous(), solo, fade_n=fade_n)
            assert torch.equal(got[b, :Lb], solo[0].cpu()), f"fade {fade_n} row {b}: differs from the solo launch on the cut row, first at sample {int((got[b, :Lb] != solo[0].cpu()).nonzero()[0])}"
            assert bool((got[b, Lb:] == 0).all()), f"fade {fade_n} row {b}: samples beyond the row are not all 0"
            worst = max(worst, _check_istft_row(got[b, :Lb], x[b, :n], fade_n, f"ragged fade {fade_n} row {b}", tight=True))
    return worst


def istft_value_input():
    """frames = 121, B = 1, ldx = 32: log-magnitudes 1.5 N - 1 with entries above ln 100 (5, 7.5, 20: the clip), 89.0 (expf overflows to inf; the clip must give
    100) and -100 (magnitude 3.7e-44: a denormal in fp32, 0 where denormals are flushed); phases uniform in +-50."""
    x = istft_input(1, 121, 32, 5)
    g = _gen(6)
    x[0, :, 9:18] = (torch.rand(121, 9, generator=g) * 2 - 1) * 50.0
    x[0, 0, 9], x[0, 1, 17] = 50.0, -50.0
    idx = torch.randperm(121 * 9, generator=g)
    for k, val in enumerate([5.0, 7.5, 20.0, 89.0, -100.0] * 4):
        t, f = divmod(int(idx[k]), 9)
        if 20 <= t < 60:  # keep the clip out of part of the row, so that both kinds of samples exist
            continue
        x[0, t, f] = val
    x[0, 100, 0], x[0, 101, 8], x[0, 102, 3], x[0, 70, 4] = 89.0, 89.0, -100.0, 4.7
    return x


def value_case_claims():
    """What the value case is chosen for, checked on the fp64 reference alone (host test)"""
    x = istft_value_input()
    lm, ph = x[0, :, :9], x[0, :, 9:18]
    assert int((lm > math.log(100.0)).sum()) >= 4 and bool((lm == 89.0).any()) and bool((lm == -100.0).any())
    assert torch.isinf(torch.exp(torch.tensor(89.0))) and 0.0 < float(torch.exp(torch.tensor(-100.0))) < 2.0 ** -126, "89 overflows expf, -100 lands in its denormals"
    assert float(ph.max()) == 50.0 and float(ph.min()) == -50.0
    ref, _, clipped = istft_reference(x[0])
    assert int(clipped.sum()) >= 10 and int((~clipped).sum()) >= 10, f"{int(clipped.sum())} of {len(ref)} samples hit the clamp: both kinds are needed"
    assert float(ref.abs().max()) == 0.99
    return int(clipped.sum()), len(ref)


def check_istft_values(ops, dev):
    x = istft_value_input()
    value_case_claims()
    worst = 0.0
    for fade_n in (0, 480):
        wav = torch.full((1, 480), NAN, device=dev)
        ops.hift_istft(x.to(dev), wav, fade_n=fade_n)
        worst = max(worst, _check_istft_row(wav[0].cpu(), x[0], fade_n, f"value case fade {fade_n}"))
    return worst


def check_istft_refusals(ops, dev):
    """fade_n = 1 (the ramp would divide 0 by 0) is refused with -22 by both entries and nothing is written.  frame_lens lives in device memory and the entry never
    synchronises, so its VALUES cannot be refused; they are defined instead: fewer than 2 frames = the row owns no sample (all 0), more than `frames` = frames."""
    x = istft_input(3, 17, 32, 9).to(dev)
    wav = torch.full((3, 64), NAN, device=dev)
    p, st = ops._p, ops._stream()
    fl = torch.tensor([17, 9, 2], dtype=torch.int32, device=dev)
    assert ops.lib.cbx_hift_istft_f32(p(x), p(wav), 3, 17, 32, 0.99, 1, st) == -22 and b"fade_n" in ops.lib.cbx_last_error()
    assert ops.lib.cbx_hift_istft_rows_f32(p(x), p(wav), p(fl), 3, 17, 32, 0.99, 1, st) == -22
    assert ops.lib.cbx_hift_istft_rows_f32(p(x), p(wav), p(fl), 3, 1, 32, 0.99, 0, st) == -22, "frames < 2"
    assert ops.lib.cbx_hift_istft_rows_f32(p(x), p(wav), p(fl), 3, 17, 17, 0.99, 0, st) == -22, "ldx < 18"
    assert ops.lib.cbx_hift_istft_rows_f32(p(x), None, p(fl), 3, 17, 32, 0.99, 0, st) == -22
    assert bool(torch.isnan(wav).all()), "a refused call wrote something"
    full = torch.empty(3, 64, device=dev)
    ops.hift_istft(x, full)
    ops.hift_istft(x, wav, frame_lens=torch.tensor([1, 0, 22], dtype=torch.int32, device=dev))
    assert bool((wav[:2] == 0).all()) and torch.equal(wav[2], full[2])
    ops.hift_istft(x, wav, fade_n=2, frame_lens=torch.tensor([-3, 17, 17], dtype=torch.int32, device=dev))
    got = wav.cpu()
    assert bool((got[0] == 0).all()) and bool((got[1:, :2] == 0).all()) and torch.equal(got[1:, 4:], full[1:, 4:].cpu()), "fade_n = 2: two samples silenced, gains 0 and 1"


def measure_torch_fp32_ratio():
    """C_TORCH_FP32's measurement: torch's own fp32 pipeline (exp / sin / cos / torch.istft / clamp in fp32) against istft_reference on every input of this file."""
    w32 = torch.hann_window(16, periodic=True)
    rows = [istft_input(3, fr, 32, 100 + fr)[b] for fr in ISTFT_FRAMES for b in range(3)] + [istft_value_input()[0]]
    rows += [ragged_istft_input()[b, :n] for b, n in enumerate(RAGGED_LENS)]
    worst = 0.0
    for x in rows:
        v = x[:, :18]
        mag, ph = torch.exp(v[:, :9]).clamp(max=100.0), torch.sin(v[:, 9:])
        y = torch.istft(torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)).t()[None], 16, 4, 16, window=w32)[0].clamp(-0.99, 0.99)
        ref, b1, _ = istft_reference(x)
        worst = max(worst, float(istft_ratio(y, ref, b1).max()))
    return worst


# ----------------------------------------------------------------------------------------------------------------- source
def _source_sd():
    return {"mel2wav.m_source.l_linear.weight": _randn((1, 9), 4, 0.5), "mel2wav.m_source.l_linear.bias": torch.tensor([0.05])}


def _source_inputs(B, T, seed):
    f0 = torch.rand(B, T, generator=_gen(seed)) * 300
    phase = (torch.rand(B, 9, 1, generator=_gen(seed + 1)) * 2 - 1) * math.pi
    phase[:, 0] = 0
    return f0, phase, _randn((B, 9, 480 * T), seed + 2)


def _run_source(ops, dev, f0, phase, noise, sd):
    B, T = f0.shape
    s = torch.full((B, 480 * T), NAN, device=dev)  # (a sample the kernel never writes stays NaN, and every comparison below counts NaN as bad)
    cum = torch.empty(B, 9, T, dtype=torch.float64, device=dev)
    ops.hift_source(f0.to(dev), phase.to(dev), noise.to(dev), sd["mel2wav.m_source.l_linear.weight"].to(dev), 0.05, s, cum)
    return s.cpu()


def check_source_thresholds(ops, dev):
    """uv = f0 > 10 is strict: f0 exactly 10.0 and 0.0 are unvoiced (noise at 0.1 / 3, no sine), the next float above 10 is voiced."""
    from oracle import ref_torch as O
    sd = _source_sd()
    f0, phase, noise = _source_inputs(2, 8, 11)
    above = float(torch.nextafter(torch.tensor(10.0), torch.tensor(20.0)))
    f0[0, 1], f0[0, 2], f0[0, 3], f0[1, 0], f0[1, 6], f0[1, 7] = 10.0, 0.0, above, above, 10.0, 0.0
    ref = O.source_module(sd, f0, phase, noise)[:, 0]
    got = _run_source(ops, dev, f0, phase, noise, sd)
    err = (got.double() - ref.double()).abs()
    assert bool((err <= 2e-5 * (1 + ref.abs())).all()), f"source at the f0 thresholds: {float(err.max()):.3e}"
    # the three frames really differ in kind: an unvoiced frame is tanh(sum_h w_h noise / 30 + b), whatever f0 is
    w = sd["mel2wav.m_source.l_linear.weight"][0].double()
    for b, fr in ((0, 1), (0, 2), (1, 6), (1, 7)):
        sl = slice(480 * fr, 480 * fr + 480)
        unv = torch.tanh((noise[b, :, sl].double() * w[:, None]).sum(0) * (0.1 / 3) + 0.05)
        assert float((got[b, sl].double() - unv).abs().max()) <= 2e-6, f"frame {fr} of row {b} (f0 {float(f0[b, fr])}) is not unvoiced"
    sl = slice(480 * 3, 480 * 4)
    unv = torch.tanh((noise[0, :, sl].double() * w[:, None]).sum(0) * (0.1 / 3) + 0.05)
    assert float((got[0, sl].double() - unv).abs().max()) > 1e-3, "f0 just above 10 is voiced"


SOURCE_LAP_EXCLUDED_MAX = 1e-5  # measured on the CPU at seed 1: 2 of 10 368 000 (sample, harmonic) pairs, at most 2 of 1 152 000 samples = 1.7e-6


def source_lap_exclusions(f0, up=480, sr=24000.0):
    """Samples where the kernel's closed form frame_cum + (k + 1) F and torch's serial fp64 cumsum round to DIFFERENT fp32 cycle counts -- from this function's own
    fp64 arithmetic, never from the kernel's output.  Both are legitimate; one fp32 ulp of ~2e4 cycles is a visible phase step.  -> bool (B, up T)"""
    B, T = f0.shape
    mult = torch.arange(1, 10, dtype=torch.float32)[None, :, None]
    Fm = (f0[:, None, :] * mult / sr)  # (B, 9, T) fp32, rounded as harmonic_inc / the oracle round it
    serial = torch.cumsum(Fm.repeat_interleave(up, dim=2).double(), dim=-1).float()
    step = float(up) * Fm.double()
    frame_cum = torch.cumsum(step, dim=-1) - step  # exclusive scan over frames, the additions in the kernel's order
    k1 = torch.arange(1, up + 1, dtype=torch.float64)
    closed = (frame_cum[..., None] + k1 * Fm.double()[..., None]).reshape(B, 9, T * up).float()
    return (serial != closed).any(1)


def check_source_second_lap(ops, dev):
    """B = 3, T = 800: 1 152 000 samples against the grid cap of 4096 x 256 = 1 048 576 threads -- the grid-stride loop's second lap.  Excluded share (see
    source_lap_exclusions) asserted <= 1e-5; measured 1.7e-6 at seed 1."""
    from oracle import ref_torch as O
    sd = _source_sd()
    f0, phase, noise = _source_inputs(3, 800, 1)
    f0[:, 5:9] = 3.0
    excl = source_lap_exclusions(f0)
    share = float(excl.double().mean())
    assert share <= SOURCE_LAP_EXCLUDED_MAX, f"{int(excl.sum())} of {excl.numel()} samples excluded"
    ref = O.source_module(sd, f0, phase, noise)[:, 0]
    got = _run_source(ops, dev, f0, phase, noise, sd)
    assert got.numel() > 4096 * 256
    assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} samples NaN or inf (not written?), first at {(~torch.isfinite(got)).nonzero()[0].tolist()}"
    err = (got.double() - ref.double()).abs()
    bad = ~(err <= 2e-5 * (1 + ref.double().abs())) & ~excl
    assert not bool(bad.any()), f"{int(bad.sum())} samples over 2e-5 (1 + |ref|), first at {bad.nonzero()[0].tolist()}; max {float(err[~excl].max()):.3e}"
    return share


# ----------------------------------------------------------------------------------------------------------------- STFT
def check_stft(ops, dev, B, L, ld):
    """fp64 torch.stft (n_fft 16, hop 4, periodic hann, center / reflect); bound per element (16 + 2) 2^-24 sum_n |x_n w_n| + 2^-24 |ref| (the derivation of
    wave_format_common.py: a 16-term fp32 chain over rounded coefficients); columns 18 .. ld - 1 are written as 0; nothing is written past the last row."""
    x = torch.tanh(_randn((B, L), 21 + L % 97))
    frames = L // 4 + 1
    buf = torch.full((B * frames * ld + 1,), NAN, device=dev)
    spec = buf[: B * frames * ld].view(B, frames, ld)
    ops.hift_stft(x.to(dev), spec)
    assert math.isnan(float(buf[-1])), "a write past the last row"
    got = spec.cpu().double()
    sp = torch.stft(x.double(), 16, 4, 16, window=_W64, return_complex=True).transpose(1, 2)  # (B, frames, 9)
    S = (F.pad(x.double()[:, None], (8, 8), mode="reflect")[:, 0].abs().unfold(1, 16, 4) * _W64).sum(-1)  # (B, frames)
    assert sp.shape == (B, frames, 9) and S.shape == (B, frames)
    for name, g, r in (("re", got[:, :, :9], sp.real), ("im", got[:, :, 9:18], sp.imag)):
        err, bound = (g - r).abs(), 18 * EPS * S[:, :, None] + EPS * r.abs()
        assert bool((err <= bound).all()), f"stft {name} B {B} L {L} ld {ld}: {int((err > bound).sum())} over the bound, worst excess {float((err - bound).max()):.3e}"
    if ld > 18:
        assert bool((got[:, :, 18:] == 0).all())


# ----------------------------------------------------------------------------------------------------------------- elementwise second laps
def _close(got, ref, tol, what):
    err = (got.detach().cpu().double() - ref).abs()
    bad = ~(err <= tol * (1.0 + ref.abs()))  # (NaN -- an element the kernel never wrote into a NaN-prefilled buffer -- counts as bad)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {bad.numel()} over tol {tol} or NaN, first at {bad.nonzero()[0].tolist()}, "
                                 f"max err {float(err[~torch.isnan(err)].max()) if (~torch.isnan(err)).any() else NAN:.3e}")


def check_act_second_lap(ops, dev, rows=16400):
    """SNAKE with a per-channel parameter on (16 400, 256): 1 049 600 float4s against the cap of 4096 x 256 = 1 048 576; 3e-6 (1 + |ref|) as test_elementwise"""
    x, a = _randn((rows, 256), 1, 2.0), 1 + 0.2 * _randn((256,), 2)
    out = torch.full((rows, 256), NAN, device=dev)
    ops.act(x.to(dev), out, ops.SNAKE, param=a.to(dev))
    xd, ad = x.double(), a.double()
    _close(out, xd + (1 / (ad + 1e-9)) * torch.sin(xd * ad) ** 2, 3e-6, "snake, second lap")


def check_axpby_second_lap(ops, dev, rows=4100, C=260):
    """rows * C = 1 066 000 > 1 048 576 items on strided views (row stride C + 4, the pad NaN resp. a sentinel): b = 0 is a copy that does not read y, b != 0
    within 2e-6 (1 + |ref|) of fp64"""
    x, y = _randn((rows, C), 3), _randn((rows, C), 4)
    xb, yb = torch.full((rows, C + 4), NAN), torch.full((rows, C + 4), NAN)
    xb[:, :C] = x
    xd, yd = xb.to(dev), yb.to(dev)
    ops.axpby(xd[:, :C], yd[:, :C], 1.0, 0.0)
    assert torch.equal(yd[:, :C].cpu(), x), "b = 0: a plain copy, y (NaN) is not read"
    yb[:, :C], yb[:, C:] = y, 7.0
    yd = yb.to(dev)
    ops.axpby(xd[:, :C], yd[:, :C], 0.75, -1.25)
    _close(yd[:, :C], 0.75 * x.double() - 1.25 * y.double(), 2e-6, "axpby, second lap")
    assert bool((yd[:, C:] == 7.0).all()), "the pad columns of y are untouched"


def check_cfm_euler_second_lap(ops, dev, B=2, T=6600, C=80):
    """B T C = 1 056 000 > 1 048 576 items, cfg on (rows B.. receive the same x) and off (rows B.. untouched); 2e-6 (1 + |ref|) as test_elementwise"""
    xin, v = _randn((2 * B, T, 320), 5), _randn((2 * B, T, C), 6)
    dx = xin.clone().to(dev)
    ops.cfm_euler(dx, v.to(dev), B, T, C, 0.07, 0.7)
    xn = xin[:B, :, :C].double() + 0.07 * (1.7 * v[:B].double() - 0.7 * v[B:].double())
    _close(dx[:B, :, :C], xn, 2e-6, "euler cond rows")
    _close(dx[B:, :, :C], xn, 2e-6, "euler uncond rows")
    assert torch.equal(dx[:, :, C:].cpu(), xin[:, :, C:]), "euler leaves mu / spk / cond"
    dx = xin.clone().to(dev)
    ops.cfm_euler(dx, v.to(dev), B, T, C, 0.07, 0.7, cfg=False)
    _close(dx[:B, :, :C], xin[:B, :, :C].double() + 0.07 * v[:B].double(), 2e-6, "euler without cfg")
    assert torch.equal(dx[B:].cpu(), xin[B:]) and torch.equal(dx[:B, :, C:].cpu(), xin[:B, :, C:]), "cfg off: rows B.. and the other columns untouched"


# ----------------------------------------------------------------------------------------------------------------- conv geometry x dispatch form
# One table for the implicit-GEMM convolution (ops.conv1d -> cbx_gemm_f32; dispatchers: chatterbox_amd/csrc/gemm_f32.hip cbx_gemm_f32, gemm_split.hip
# cbx_gemm_split_dispatch).  kind "conv": w (cout, cin, k), reference F.conv1d(pad(x, (pad, pad_r)), stride, dilation) after a nearest x `up` upsample;
# kind "convT": ConvTranspose1d (cin -> cout, k, stride, padding = pad) in its phase-packed 3-tap form, reference F.conv_transpose1d.  lens = valid INPUT rows per
# batch row (None: all T); input rows at or beyond lens[b] hold NaN (the loader's contract is zeros there, so any read of them shows in the output), and a row is
# compared only below ITS OWN output length, against the fp64 reference of the row CUT to lens[b].  ldc: row stride of the output buffer (NaN-prefilled; the
# columns beyond cout must stay NaN).  precisions: cbx_gemm_t.precision values the case runs at (0 = exact fp32).
def _case(name, cin, cout, k, dil=1, stride=1, pad=0, up=1, T=0, B=2, lens=None, kind="conv", pad_r=None, ldc=None, precisions=(0, 3, 6, 16), epilogues=("plain",)):
    return dict(name=name, cin=cin, cout=cout, k=k, dil=dil, stride=stride, pad=pad, up=up, T=T, B=B if lens is None else len(lens), lens=lens, kind=kind,
                pad_r=pad if pad_r is None else pad_r, ldc=ldc, precisions=precisions, epilogues=epilogues)


RAGGED_EPILOGUES = ("plain", "snake", "res_snake2", "res_third_acc_snake2")  # the two resblock forms: c1 (act = SNAKE), c2 (+ residual, out2 = SNAKE; last: alpha 1/3, beta 1)
CONV_CASES = [
    _case("conv_pre_T5", 80, 512, 7, pad=3, T=5),                                                    # a short streaming window: M <= 32 with taps
    _case("conv_pre_T32", 80, 512, 7, pad=3, T=32), _case("conv_pre_T33", 80, 512, 7, pad=3, T=33),  # the skinny boundary
    _case("resblock_k11_d5_T20", 64, 64, 11, dil=5, pad=25, T=20),                                   # T shorter than the receptive field 51
    _case("resblock_k11_d5_ragged", 64, 64, 11, dil=5, pad=25, T=140, lens=(140, 51, 50, 1, 0), epilogues=RAGGED_EPILOGUES),
    _case("resblock_k7_d3_ragged", 128, 128, 7, dil=3, pad=9, T=90, lens=(90, 33, 2), epilogues=RAGGED_EPILOGUES),
    _case("source_down_s15_ragged", 32, 256, 30, stride=15, pad=7, T=601, lens=(601, 300, 16), epilogues=RAGGED_EPILOGUES),
    _case("source_down_s3_ragged", 32, 128, 6, stride=3, pad=1, T=241, lens=(241, 100, 7), epilogues=RAGGED_EPILOGUES),
    _case("source_down_1x1", 32, 64, 1, T=77, lens=(77, 40)),
    _case("source_down_1x1_wide", 32, 64, 1, T=2800, B=3),
    _case("ups_k16_s8_ragged", 64, 32, 16, stride=8, pad=4, T=41, lens=(41, 17, 1), kind="convT", epilogues=RAGGED_EPILOGUES),
    _case("ups_k11_s5_ragged", 32, 16, 11, stride=5, pad=3, T=41, lens=(41, 17, 1), kind="convT", epilogues=RAGGED_EPILOGUES),
    _case("up2_k5_ragged", 32, 128, 5, pad=4, pad_r=0, up=2, T=50, lens=(50, 31, 7), epilogues=RAGGED_EPILOGUES),
    _case("up2_k5_T10", 32, 128, 5, pad=4, pad_r=0, up=2, T=10, lens=(10, 3)),
    _case("k64_form_k7_d3", 256, 256, 7, dil=3, pad=9, T=200, B=1, precisions=(0,)),
    _case("k64_form_k11", 128, 64, 11, pad=5, T=200, B=1, precisions=(0,)),                           # N <= 64 wins over the 64-wide-K form: expected_form says so
    _case("split_tile_128x64", 32, 256, 3, pad=1, T=1400, B=3), _case("split_tile_64", 32, 256, 3, pad=1, T=77, B=3),
    _case("conv_post", 64, 18, 7, pad=3, T=77, lens=(77, 30), ldc=32),
]
CASES = {c["name"]: c for c in CONV_CASES}
SPLIT_TOL = {6: 3e-5, 16: 3e-5, 3: 1e-4}  # test_ops_gpu.py::_SPLIT_TOL


def gemm_shape(c):
    """(M, N, K, Cin, taps, nz) of the launch ops.conv1d makes for a case"""
    if c["kind"] == "convT":
        return c["T"], c["stride"] * c["cout"], 3 * c["cin"], c["cin"], 3, c["B"]
    return out_rows(c, c["T"]), c["cout"], c["k"] * c["cin"], c["cin"], c["k"], c["B"]


def out_rows(c, n):
    """output rows of a row of n input rows (its own output length)"""
    if c["kind"] == "convT":
        return n * c["stride"]
    return max(0, (n * c["up"] + c["pad"] + c["pad_r"] - c["dil"] * (c["k"] - 1) - 1) // c["stride"] + 1)


def expected_form(c, precision):
    """The kernel form the two dispatchers choose for a case -- a pure-Python mirror of cbx_gemm_f32 (gemm_f32.hip) and cbx_gemm_split_dispatch (gemm_split.hip):
    ("skinny",) 32x128 tiles, M <= 32 at every precision; ("n64",) N <= 64; ("fast16",) / ("fast64",) the buffer-load loader on 16- / 64-wide K tiles; ("generic",);
    ("split", tile, loader) with tile 64 or 12864 (128x64) and loader 0 (generic), 1 (Linear) or 2 (Conv1d)."""
    M, N, K, cin, taps, nz = gemm_shape(c)
    up = c["up"] if c["kind"] == "conv" else 1
    if M <= 32:
        return ("skinny",)
    if precision in (3, 6, 16) and not (taps > 1 and cin % 32):
        g128 = -(-M // 128) * -(-N // 128) * nz
        tile = 12864 if g128 >= 64 and N >= 64 else 64
        fast = up == 1 and K % 32 == 0
        return ("split", tile, 0 if not fast else 1 if taps == 1 else 2)
    if N <= 64:
        return ("n64",)
    fast_ok = lambda bk: up == 1 and K % bk == 0 and cin % bk == 0
    wgs = -(-M // 128) * -(-N // 64) * nz
    if wgs <= 128 and K >= 1024 and fast_ok(64):
        return ("fast64",)
    return ("fast16",) if fast_ok(16) else ("generic",)


# every form a conv of the vocoder (chatterbox_amd/hift.py, stage_seams.hip cbx_hift_decode) or of the encoder's Upsample1D can reach
REACHABLE_FORMS = {("skinny",), ("n64",), ("fast16",), ("fast64",), ("generic",), ("split", 64, 0), ("split", 64, 1), ("split", 64, 2), ("split", 12864, 1), ("split", 12864, 2)}
UNREACHED_FORMS = {
    ("split", 12864, 0): "the generic loader on 128x64 tiles needs up > 1 (or K % 32 != 0, which a conv with taps cannot have: it falls back to fp32) on a grid of 64+ "
                         "tiles; no vocoder conv upsamples -- covered at tile 64 by up2_k5_ragged, the tile shape by split_tile_128x64",
}


def form_coverage():
    """{form: [(case, precision), ...]} over the table; asserts that every reachable form is reached (the pattern of wave_format_common.what_the_sets_cover)"""
    reached = {}
    for c in CONV_CASES:
        for p in c["precisions"]:
            reached.setdefault(expected_form(c, p), []).append((c["name"], p))
    missing = REACHABLE_FORMS - set(reached)
    assert not missing, f"forms no case of the table reaches: {sorted(missing)}"
    assert not set(reached) - REACHABLE_FORMS, f"forms reached but not listed: {sorted(set(reached) - REACHABLE_FORMS)}"
    assert not set(UNREACHED_FORMS) & set(reached)
    return reached


def _conv_data(c):
    """inputs of a case (CPU): x (B, T, cin) channel-last with NaN rows beyond lens, the torch weight, the packed weight and bias, the per-channel parameters"""
    seed = 1000 + sum(map(ord, c["name"]))
    B, T, cin, cout, k = c["B"], c["T"], c["cin"], c["cout"], c["k"]
    x = _randn((B, T, cin), seed)
    lens = c["lens"] if c["lens"] is not None else (T,) * B
    for b, n in enumerate(lens):
        x[b, n:] = NAN
    from chatterbox_amd import weights
    if c["kind"] == "convT":
        w, bias = _randn((cin, cout, k), seed + 1, 1 / math.sqrt(cin * k / c["stride"])), _randn((cout,), seed + 2)
        wp, bp = weights.pack_conv_transpose(w, bias, c["stride"], c["pad"])
    else:
        w, bias = _randn((cout, cin, k), seed + 1, 1 / math.sqrt(cin * k)), _randn((cout,), seed + 2)
        wp, bp = weights.pack_conv(w), bias
    N = wp.shape[0]
    return dict(x=x, w=w, bias=bias, wp=wp, bp=bp, lens=lens, a1=1 + 0.2 * _randn((N,), seed + 3), a2=1 + 0.2 * _randn((N,), seed + 4))


def _conv_ref_row(c, d, b, absolute=False):
    """fp64 reference of batch row b CUT to its own length: (rows, N) in the kernel's output layout, or None for an empty row.  absolute: the bound's S (the conv of
    |x| with |w|, plus |bias|)."""
    n = d["lens"][b]
    if out_rows(c, n) == 0:
        return None
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    xr = f(d["x"][b, :n]).t()[None]  # (1, cin, n)
    if c["kind"] == "convT":
        y = F.conv_transpose1d(xr, f(d["w"]), f(d["bias"]), stride=c["stride"], padding=c["pad"])  # (1, cout, n s)
        y = y[0].t().reshape(n, c["stride"] * c["cout"])  # row t of the packed output holds samples t s .. t s + s - 1
    else:
        if c["up"] > 1:
            xr = xr.repeat_interleave(c["up"], dim=2)
        y = F.conv1d(F.pad(xr, (c["pad"], c["pad_r"])), f(d["w"]), f(d["bias"]), stride=c["stride"], dilation=c["dil"])[0].t()
    assert y.shape[0] == (n if c["kind"] == "convT" else out_rows(c, n)), (c["name"], y.shape)
    return y


def _snake64(v, a):
    return v + (1.0 / (a.double() + 1e-9)) * torch.sin(v * a.double()) ** 2


def check_conv_case(ops, dev, name, precision):
    """One row of the table at one precision, every epilogue it lists.  plain at precision 0: per element (K + 2) 2^-24 S + 2^-24 |ref|, S = the fp64 conv of |x|
    with |w| plus |b| (a K-term fp32 accumulation in any order, one rounding for the bias).  Otherwise the project's tolerances: 4e-5 (1 + |ref|) at precision 0
    (test_conv1d), 1.5 _SPLIT_TOL[p] (1 + |ref|) at the split precisions (test_split_gemm_conv), both times max(1, sqrt(K / 256)).  The second output (Snake of the
    first) is held to the FIRST OUTPUT THE LAUNCH WROTE at the elementwise tolerance 3e-6 (test_elementwise), which does not widen with the conv's own error."""
    c = CASES[name]
    d = _conv_data(c)
    M, N, K, cin, taps, B = gemm_shape(c)
    ldc = c["ldc"] or N
    xd, wd, bd = d["x"].to(dev), d["wp"].to(dev), d["bp"].to(dev)
    lens_d = None if c["lens"] is None else torch.tensor(c["lens"], dtype=torch.int32, device=dev)
    conv_kw = dict(taps=taps, cin=cin, bias=bd, lens=lens_d)
    if c["kind"] == "conv":
        conv_kw.update(dil=c["dil"], stride=c["stride"], pad_left=c["pad"], up=c["up"])
    else:
        conv_kw.update(pad_left=1)
    refs = [_conv_ref_row(c, d, b) for b in range(B)]
    tol = (4e-5 if precision == 0 else 1.5 * SPLIT_TOL[precision]) * max(1.0, math.sqrt(K / 256))
    res, c0 = _randn((B, M, N), 7), _randn((B, M, N), 8)
    for epi in c["epilogues"]:
        buf = torch.full((B, M, ldc), NAN, device=dev)
        out, out2, kw = buf[:, :, :N], None, {}
        if epi == "snake":
            kw = dict(act=ops.SNAKE, act_param=d["a1"].to(dev))
        elif epi in ("res_snake2", "res_third_acc_snake2"):
            out2 = torch.full((B, M, N), NAN, device=dev)
            kw = dict(residual=res.to(dev), out2=out2, act2=ops.SNAKE, act2_param=d["a2"].to(dev))
            if epi == "res_third_acc_snake2":
                out.copy_(c0.to(dev))
                kw.update(alpha=1.0 / 3, beta=1.0)
        with ops.gemm_precision(precision):
            ops.conv1d(xd, wd, out, **conv_kw, **kw)
        got = buf.cpu()
        if ldc > N:
            assert bool(torch.isnan(got[:, :, N:]).all()), f"{name} p{precision} {epi}: columns {N} .. {ldc - 1} of the output buffer were written"
        for b in range(B):
            if refs[b] is None:
                continue
            r, rows = refs[b], refs[b].shape[0]
            if epi == "snake":
                r = _snake64(r, d["a1"])
            elif epi == "res_snake2":
                r = r + res[b, :rows].double()
            elif epi == "res_third_acc_snake2":
                r = c0[b, :rows].double() + (r + res[b, :rows].double()) / 3
            g = got[b, :rows, :N].double()
            err = (g - r).abs()
            if epi == "plain" and precision == 0:
                lim = (K + 2) * EPS * _conv_ref_row(c, d, b, absolute=True) + EPS * r.abs()
            else:
                lim = tol * (1.0 + r.abs())
            bad = ~(err <= lim)  # (NaN counts as bad)
            assert not bool(bad.any()), (f"{name} p{precision} {epi} row {b} ({rows} of {M} output rows): {int(bad.sum())} / {bad.numel()} over the bound, first at "
                                         f"{bad.nonzero()[0].tolist()}, max err {float(err[~torch.isnan(err)].max()) if (~torch.isnan(err)).any() else NAN:.3e}")
            if out2 is not None:
                g2, r2 = out2[b, :rows].cpu().double(), _snake64(g, d["a2"])
                bad = ~((g2 - r2).abs() <= 3e-6 * (1.0 + r2.abs()))
                assert not bool(bad.any()), f"{name} p{precision} {epi} row {b}: second output is not Snake of the first: {int(bad.sum())} / {bad.numel()}"
