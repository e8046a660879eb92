"""Kernel-level tests (-m gpu; the same bodies run on the SIMT emulator) of the front-end kernels (csrc/frontend.hip) and of the glue
entry points no other kernel-level test calls: each kernel against fp64 torch on seeded inputs, on strided views whose pad columns
hold a sentinel that must come back bit-identical, into outputs pre-filled with a sentinel so that an unwritten element is seen.

Tolerances are those of tests/test_ops_gpu.py: moves, masks, max and index arithmetic are exact; element-wise maps follow
test_gelu_erf_accuracy (error against fp64, relative to max(1, |ref|), at most 2.5 x the error of torch's own fp32 expression,
floor 6e-8); reductions over time or channels follow test_layernorm_rmsnorm (2e-5 * (1 + |ref|)).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = -12345.0


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(got, ref, tol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > tol * (1.0 + ref.abs())
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.3e} (tol {tol} * (1 + |ref|))")
    assert not bad.any(), f"{what}: max err {err.max():.3e} (ref max {ref.abs().max():.3e}), {int(bad.sum())} / {bad.numel()} over tol {tol}"


def _map_rule(got, ref64, torch32, what="", ulps=0):
    """test_gelu_erf_accuracy's rule for an element-wise map: not worse than 2.5 x torch's own fp32 expression (floor 6e-8), relative to max(1, |ref|).
    ulps: the documented accuracy of the device math function the map IS (test_unary), as a floor of the bound."""
    got, t32 = got.detach().cpu().double(), torch32.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    den = ref64.abs().clamp(min=1.0)
    err, f32 = float(((got - ref64).abs() / den).max()), float(((t32 - ref64).abs() / den).max())
    print(f"{what}: max scaled err {err:.3e}, torch fp32 {f32:.3e}")
    assert err <= max(2.5 * max(f32, 6e-8), ulps * 2.0 ** -23), f"{what}: max err {err:.3e} against fp64, torch's fp32 expression has {f32:.3e}"


class _View:
    """A (.., rows, C) tensor placed in a wider, longer buffer full of SENT: `v` is the strided view handed to the kernel."""

    def __init__(self, t, dev, pad=8, extra_rows=0):
        shape = list(t.shape)
        shape[-1] += pad
        shape[-2] += extra_rows
        buf = torch.full(shape, SENT)
        buf[..., : t.shape[-2], : t.shape[-1]] = t
        self.buf, self.shape = buf.to(dev), t.shape
        self.v = self.buf[..., : t.shape[-2], : t.shape[-1]]

    def pads_intact(self, what):
        b = self.buf.cpu().clone()
        b[..., : self.shape[-2], : self.shape[-1]] = SENT
        assert bool((b == SENT).all()), f"{what}: pad elements written"


def _out(shape, dev, pad=8, extra_rows=0):
    return _View(torch.full(shape, SENT), dev, pad, extra_rows)


@pytest.mark.parametrize("B,T,C,taps,pad_left,add", [(2, 50, 1280, 31, 15, 1), (5, 20, 8, 4, 0, 0), (5, 20, 4, 5, 4, 1), (5, 7, 8, 31, 15, 0), (3, 1, 4, 3, 1, 1),
                                                     (5, 33, 12, 2, 1, 1)])
def test_dwconv1d(dev, B, T, C, taps, pad_left, add):
    """Depthwise conv against F.conv1d(groups = C) in fp64 on the input zero-masked beyond lens[b]; the masked input rows hold 1e6 (row
    lens[b] - 1 must not see row lens[b]); rows >= lens[b] come back exactly zero; lens beyond T are clamped; lens = None reads every row."""
    from chatterbox_amd import ops
    x, w = _r((B, T, C), 1), _r((C, taps), 2, 0.3)
    for lens in ([T, T - 1, 1, 0, T + 9][:B] if B > 3 else [T, 0, T + 9][:B], None):
        n = [T] * B if lens is None else [max(0, min(T, v)) for v in lens]
        xin = x.clone()
        for b in range(B):
            xin[b, n[b]:] = 1e6
        xm = x.double().clone()
        for b in range(B):
            xm[b, n[b]:] = 0
        ref = F.conv1d(F.pad(xm.transpose(1, 2), (pad_left, taps - 1 - pad_left)), w.double()[:, None], groups=C).transpose(1, 2)
        if add:
            ref = ref + xm
        for b in range(B):
            ref[b, n[b]:] = 0
        xv, y = _View(xin, dev, 12, 3), _out((B, T, C), dev, 4, 2)
        ops.dwconv1d(xv.v, w.to(dev), y.v, taps, pad_left, None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev), bool(add))
        _close(y.v, ref, 2e-5, f"dwconv1d {B}x{T}x{C} taps {taps} lens {lens}")
        for b in range(B):
            assert float(y.v[b, n[b]:].abs().sum()) == 0.0, "rows beyond lens[b] are exactly zero"
        y.pads_intact("dwconv1d y")
        xv.pads_intact("dwconv1d x")


@pytest.mark.parametrize("B,H", [(1, 256), (5, 40)])
def test_lstm_cell(dev, B, H):
    """torch.nn.LSTMCell arithmetic, gate order (i, f, g, o), a different scale per gate; three chained steps updating c in place; then gates at +-60."""
    from chatterbox_amd import ops
    sc = torch.tensor([0.5, 1.0, 1.5, 2.0]).repeat_interleave(H)
    c = _View(_r((B, H), 9), dev, 4)
    h = _out((B, H), dev, 12)

    def step(pre, hh, what):
        pv, qv = _View(pre, dev, 8), _View(hh, dev, 16)
        c0 = c.v.cpu().clone()
        ops.lstm_cell(pv.v, qv.v, c.v, h.v)
        outs = []
        for dt in (torch.float64, torch.float32):
            i, f, g, o = (pre.to(dt) + hh.to(dt)).view(B, 4, H).unbind(1)
            cn = torch.sigmoid(f) * c0.to(dt) + torch.sigmoid(i) * torch.tanh(g)
            outs.append((cn, torch.sigmoid(o) * torch.tanh(cn)))
        _map_rule(c.v, outs[0][0], outs[1][0], f"lstm c {what}")
        _map_rule(h.v, outs[0][1], outs[1][1], f"lstm h {what}")
        for v in (pv, qv, c, h):
            v.pads_intact("lstm_cell")

    for s in range(3):
        step(_r((B, 4 * H), 10 + s) * sc, _r((B, 4 * H), 20 + s) * sc * 0.5, f"step {s}")
    sat = torch.where(_r((B, 4 * H), 30) > 0, 60.0, -60.0)
    step(sat, torch.zeros(B, 4 * H), "saturated")


@pytest.mark.parametrize("C", [4, 128, 1000])
def test_affine_act(dev, C):
    from chatterbox_amd import ops
    rows = 37
    x, sc, sh = _r((rows, C), 1, 2.0), 1 + 0.3 * _r((C,), 2), _r((C,), 3)
    for act, fn in ((ops.NONE, lambda t: t), (ops.LRELU, torch.relu)):  # (LRELU with slope 0: the ReLU of CAMPPlus)
        xv, y = _View(x, dev, 4), _out((rows, C), dev, 8)
        ops.affine_act(xv.v, y.v, sc.to(dev), sh.to(dev), act)
        _map_rule(y.v, fn(x.double() * sc.double() + sh.double()), fn(x * sc + sh), f"affine_act C {C} act {act}")
        y.pads_intact("affine_act")


@pytest.mark.parametrize("F_", [201, 257, 513, 1])
def test_cplx_power(dev, F_):
    from chatterbox_amd import ops
    rows = 23
    spec = _r((rows, 2 * F_), 1, 3.0)
    spec[5] = 0.0
    for mode, eps in ((0, 0.0), (1, 0.0), (1, 1e-9)):
        sv, o = _View(spec, dev, 6), _out((rows, F_), dev, 3)  # ld_spec = 2 F + 6: the imaginary half starts at F, not at ld_spec / 2
        ops.cplx_power(sv.v, o.v, mode, eps)
        res = []
        for dt in (torch.float64, torch.float32):
            p = spec[:, :F_].to(dt) ** 2 + spec[:, F_:].to(dt) ** 2
            res.append(torch.sqrt(p + eps) if mode else p)
        _map_rule(o.v, res[0], res[1], f"cplx_power F {F_} mode {mode} eps {eps}")
        if eps == 0.0:
            assert float(o.v[5].abs().sum()) == 0.0, "a zero row gives exactly zero"
        o.pads_intact("cplx_power")


def test_unary(dev):
    """The four maps, inputs below / at / above the clamp, C odd; CBX_UN_FLOOR_AFFINE fed by reduce_max on the device (the S3 log-mel chain).

    The two log maps are one call of the device library's logf / log10f each, and the rule of test_gelu_erf_accuracy (2.5 x torch's CPU fp32 op, which is
    correctly rounded here: 5.8e-8) is tighter than what that library promises: measured on the MI355X, relative to max(1, |ref|), log 1.45e-7 and log10
    1.51e-7 against torch's 5.8e-8 (bound 1.5e-7: log10 misses it by 1 %).  The HIP math API documents logf at 1 ulp and log10f at 2 ulp; the bound for
    these two maps is therefore that documented 2 ulp (2.4e-7), not a figure taken from the kernel."""
    from chatterbox_amd import ops
    rows, C = 19, 129
    a = 1e-5
    x = _r((rows, C), 1).abs() * 1e-2
    x[0, :6] = torch.tensor([a, a * 0.5, a * 2, 0.0, -1.0, 1e-30])
    for op, fn in ((ops.UN_LOG_CLAMP, torch.log), (ops.UN_LOG10_CLAMP, torch.log10)):
        xv, y = _View(x, dev, 3), _out((rows, C), dev, 5)
        ops.unary(xv.v, y.v, op, a=a)
        _map_rule(y.v, fn(x.double().clamp(min=float(torch.tensor(a)))), fn(x.clamp(min=a)), f"unary op {op}", ulps=2)
        assert len(set(y.v[0, [0, 1, 3, 4, 5]].tolist())) == 1 and float(y.v[0, 2]) > float(y.v[0, 0]), "at and below the clamp: the clamp's value"
        y.pads_intact("unary")
    z = _r((rows, C), 2, 3.0)
    xv, y = _View(z, dev, 3), _out((rows, C), dev, 5)
    ops.unary(xv.v, y.v, ops.UN_AFFINE, a=0.25, b=-1.5)
    _map_rule(y.v, z.double() * 0.25 - 1.5, z * 0.25 - 1.5, "unary affine")
    gmax = torch.full((1,), SENT).to(dev)
    ops.reduce_max(xv.v, gmax)
    assert float(gmax) == float(z.max())
    ops.unary(xv.v, y.v, ops.UN_FLOOR_AFFINE, a=8.0, b=4.0, dev_scalar=gmax)
    _map_rule(y.v, (torch.maximum(z.double(), z.double().max() - 8.0) + 4.0) / 4.0, (torch.maximum(z, z.max() - 8.0) + 4.0) / 4.0, "unary floor-affine")
    y.pads_intact("unary")
    xv.pads_intact("unary x")


def test_reduce_max(dev, big=True):
    """Exact; an all-negative input (neither 0 nor a stale value); the maximum at the first / last element; larger values in the pad columns are ignored."""
    from chatterbox_amd import ops
    for rows, C in [(1, 1), (1, 63), (3, 341), (1, 1024), (5, 205)] + ([(300, 1001)] if big else []):
        x = -_r((rows, C), rows + C).abs() - 0.5
        for where in (None, (0, 0), (rows - 1, C - 1)):
            t = x.clone()
            if where:
                t[where] = -0.25
            xv = _View(t, dev, 5)
            xv.buf[..., C:] = 7.0  # pad columns hold LARGER values
            out = torch.full((1,), 99.0).to(dev)
            ops.reduce_max(xv.v, out)
            assert float(out) == float(t.max()), f"reduce_max {rows}x{C} max at {where}: {float(out)} vs {float(t.max())}"


@pytest.mark.parametrize("seg_len", [100, 37])
def test_seg_context_and_gate(dev, seg_len, C=8):
    """CAMPPlus context: x.mean(0) + avg_pool1d(ceil_mode = True) (the last window averages the frames it has), then y * sigmoid(m[t // seg_len])."""
    from chatterbox_amd import ops
    for T in (seg_len * 3, seg_len * 3 + 1, seg_len - 1, 1, 63, 64, 65, seg_len * 9 + 50):
        x = _r((T, C), T) + 0.3
        n_seg = (T + seg_len - 1) // seg_len
        xv, ctx = _View(x, dev, 4), _out((n_seg, C), dev, 4, 2)
        ops.seg_context(xv.v, ctx.v, seg_len)
        xd = x.double()
        ref = xd.mean(0) + F.avg_pool1d(xd.t()[None], seg_len, ceil_mode=True)[0].t()
        _close(ctx.v, ref, 2e-5, f"seg_context T {T} seg_len {seg_len}")
        ctx.pads_intact("seg_context")
        y, m = _r((T, C), T + 1), _r((n_seg, C), T + 2, 2.0)
        yv, mv = _View(y, dev, 8, 1), _View(m, dev, 4)
        ops.seg_gate_mul(yv.v, mv.v, seg_len)
        seg = torch.arange(T) // seg_len
        _map_rule(yv.v, y.double() * torch.sigmoid(m.double()[seg]), y * torch.sigmoid(m[seg]), f"seg_gate_mul T {T} seg_len {seg_len}")
        yv.pads_intact("seg_gate_mul")


@pytest.mark.parametrize("C", [1, 3, 512])
def test_stats_pool(dev, C):
    """Mean and unbiased std over time; channel 0 has mean 100 and std 0.1 (a one-pass variance fails it)."""
    from chatterbox_amd import ops
    for T in (2, 3, 255, 256, 257, 1000):
        x = _r((T, C), T + C, 1.5) + 0.2
        x[:, 0] = 100.0 + 0.1 * _r((T,), 5)
        xv = _View(x, dev, 7)
        out = torch.full((2 * C + 2,), SENT).to(dev)
        ops.stats_pool(xv.v, out)
        ref = torch.cat([x.double().mean(0), x.double().std(0, unbiased=True)])
        _close(out[: 2 * C], ref, 2e-5, f"stats_pool T {T} C {C}")
        assert out[2 * C:].tolist() == [SENT, SENT]


def test_fsq_index(dev, n_random=20000):
    """(i) every one of the 6561 codes from exact digits; (ii) random h, rows within 1e-4 of a rounding boundary |tanh(h) * 0.999| = 0.5 (fp64) left out
    (at most 1 % of the rows, asserted), the rest exactly equal."""
    from chatterbox_amd import ops
    codes = torch.arange(6561)
    digits = torch.stack([(codes // 3 ** d) % 3 - 1 for d in range(8)], 1)  # digit d has weight 3^d
    hv = _View(digits.float() * 2.0, dev, 5)
    idx = torch.full((6561 + 2,), -9, dtype=torch.int64).to(dev)
    ops.fsq_index(hv.v, idx)
    assert torch.equal(idx[:6561].cpu(), codes) and idx[6561:].tolist() == [-9, -9]
    h = _r((n_random, 8), 3, 1.2)
    q = torch.tanh(h.double()) * 0.999
    near = ((q.abs() - 0.5).abs() < 1e-4).any(1)
    assert int(near.sum()) <= 0.01 * n_random, f"{int(near.sum())} of {n_random} rows next to a rounding boundary"
    print(f"fsq_index: {int(near.sum())} of {n_random} rows set aside")
    ref = ((torch.round(q) + 1).long() * 3 ** torch.arange(8)).sum(1)
    hv = _View(h, dev, 3)
    idx = torch.full((n_random,), -9, dtype=torch.int64).to(dev)
    ops.fsq_index(hv.v, idx)
    assert torch.equal(idx.cpu()[~near], ref[~near])


# ----------------------------------------------------------------------------- glue entry points

def test_axpby(dev):
    """y = a x + b y on strided views, C odd, in place; b = 0 does not read y (NaN in y must not come through)."""
    from chatterbox_amd import ops
    rows, C = 29, 77
    x, y = _r((rows, C), 1), _r((rows, C), 2)
    xv, yv = _View(x, dev, 3), _View(torch.full((rows, C), float("nan")), dev, 9)
    ops.axpby(xv.v, yv.v, a=1.0, b=0.0)
    assert torch.equal(yv.v.cpu(), x), "b = 0: a plain copy"
    yv = _View(y, dev, 9)
    ops.axpby(xv.v, yv.v, a=0.75, b=-1.25)
    _map_rule(yv.v, 0.75 * x.double() - 1.25 * y.double(), 0.75 * x - 1.25 * y, "axpby")
    yv.pads_intact("axpby")
    ops.axpby(xv.v, xv.v, a=2.0, b=0.5)  # in place: x = 2.5 x
    assert torch.equal(xv.v.cpu(), 2.5 * x)
    xv.pads_intact("axpby in place")


@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("C", [768, 1024])
def test_add_norm_layernorm_form(dev, C, ks):
    """ops.add_rmsnorm(..., bias=, rms=False): x += sum_k part[k]; h = LayerNorm(x) * w + b (GPT-2 ln_1 / ln_2 / ln_f of the 7-launch path)."""
    from chatterbox_amd import ops
    for rows in (1, 5, 16):
        x, part = _r((rows, C), 1, 2.0) + 0.5, _r((ks, rows, C), 2)
        w, b = 1 + 0.1 * _r((C,), 3), 0.1 * _r((C,), 4)
        xv, h = _View(x, dev, 4), _out((rows, C), dev, 8)
        ops.add_rmsnorm(xv.v, part.to(dev), w.to(dev), h.v, 1e-5, bias=b.to(dev), rms=False)
        s = x.double() + part.double().sum(0)
        _close(xv.v, s, 2e-5, f"add_norm residual stream rows {rows} C {C} ks {ks}")
        _close(h.v, F.layer_norm(s, (C,), w.double(), b.double(), 1e-5), 2e-5, f"add_norm layernorm rows {rows} C {C} ks {ks}")
        h.pads_intact("add_norm h")
        xv.pads_intact("add_norm x")


def test_softmax_rows(dev):
    """The bd == NULL, Tk != Tq path of cbx_softmax_relpos_f32 (perceiver attention): 32 queries, 150 keys, pad columns zeroed."""
    from chatterbox_amd import ops
    Z1, Z2, Tq, Tk, ld = 2, 4, 32, 150, 152
    s = _r((Z1, Z2, Tq, Tk), 1, 3.0)
    sv = _View(s, dev, 2)
    for lens in (None, [150, 61]):
        p = torch.full((Z1, Z2, Tq, ld), 7.0).to(dev)
        ops.softmax_rows(sv.v, p, 0.125, Tk, None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev))
        sc = s.double() / 8
        if lens is not None:
            m = torch.arange(Tk)[None, :] >= torch.tensor(lens)[:, None]
            sc = sc.masked_fill(m[:, None, None], float("-inf"))
        ref = torch.softmax(sc, -1)
        _close(p[..., :Tk], ref, 1e-5, f"softmax_rows lens {lens}")
        assert float(p[..., Tk:].abs().max()) == 0.0, "pad columns zeroed"
        if lens is not None:
            assert float(p[1, :, :, 61:].abs().max()) == 0.0, "masked keys are exactly zero"


def test_hift_stft_ragged(dev):
    """cbx_hift_stft_f32 with sample_lens.  Contract (chatterbox_amd/hift.py::decode): row b holds sample_lens[b] = 480 * lens[b] valid samples; its
    first sample_lens[b] / 4 + 1 frames equal torch.stft (centre, reflect) of the row CUT to its own length -- the reflection happens at the row's
    own end, not at the batch's.  The frames beyond are masked by every consumer (spec_len = 120 * lens + 1): they only have to be finite, and
    columns 18.. of every frame are zero."""
    from chatterbox_amd import ops
    L, lens = 480, [480, 236, 16]
    s = _r((3, L), 1)
    for b, n in enumerate(lens):
        s[b, n:] = 1e6  # what lies behind a row's end must not be read into its own frames
    spec = torch.full((3, L // 4 + 1, 32), SENT).to(dev)
    ops.hift_stft(s.to(dev), spec, torch.tensor(lens, dtype=torch.int32).to(dev))
    win = torch.hann_window(16, periodic=True).double()
    for b, n in enumerate(lens):
        sp = torch.stft(s[b, :n].double(), 16, 4, 16, window=win, return_complex=True)
        _close(spec[b, : n // 4 + 1, :9], sp.real.t(), 1e-5, f"stft re row {b}")
        _close(spec[b, : n // 4 + 1, 9:18], sp.imag.t(), 1e-5, f"stft im row {b}")
    assert torch.isfinite(spec).all() and float(spec[:, :, 18:].abs().max()) == 0.0


def test_embed_negative_ids_and_scale(dev):
    from chatterbox_amd import ops
    C = 64
    tab, tab2 = _r((50, C), 3), _r((20, C), 4)
    ids, ids2 = torch.tensor([3, -1, 49, -1, 0], dtype=torch.int64), torch.tensor([0, 5, -1, -1, 19], dtype=torch.int32)
    scale = math.sqrt(512)
    o = _out((5, C), dev, 4)
    ops.embed(ids.to(dev), tab.to(dev), o.v, table2=tab2.to(dev), ids2=ids2.to(dev), scale=scale)
    def ref(dt):
        zero = torch.zeros(1, dtype=dt)
        a = torch.where(ids[:, None] >= 0, tab[ids.clamp(min=0)].to(dt) * torch.tensor(scale, dtype=torch.float32).to(dt), zero)
        return a + torch.where(ids2[:, None] >= 0, tab2[ids2.clamp(min=0).long()].to(dt), zero)

    _map_rule(o.v, ref(torch.float64), ref(torch.float32), "embed")
    assert float(o.v[3].abs().sum()) == 0.0 and torch.equal(o.v[1].cpu(), tab2[5]), "negative ids give zero rows, negative ids2 are skipped"
    o.pads_intact("embed")


def test_act_kinds(dev, n=1 << 20):
    """cbx_act_f32's TANH, ABS, SILU, MISH, ELU, GELU_TANH through ops.act on the grid of test_gelu_erf_accuracy extended to +-100 (SiLU / Mish / ELU must
    not overflow)."""
    from chatterbox_amd import ops
    x = torch.cat([torch.linspace(-8, 8, n), torch.linspace(-100, 100, n // 16), torch.linspace(19.9, 20.1, 4096),
                   torch.tensor([0.0, 1e-30, -1e-30, 1e-8, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4])])
    x = x[: x.numel() // 8 * 8].reshape(-1, 8).contiguous()
    xv = _View(x, dev, 4)
    for kind, fn in ((ops.TANH, torch.tanh), (ops.ABS, torch.abs), (ops.SILU, F.silu), (ops.MISH, F.mish), (ops.ELU, F.elu),
                     (ops.GELU_TANH, lambda t: F.gelu(t, approximate="tanh"))):
        o = _out(x.shape, dev, 4)
        ops.act(xv.v, o.v, kind)
        if kind == ops.ABS:
            assert torch.equal(o.v.cpu(), x.abs())
        else:
            _map_rule(o.v, fn(x.double()), fn(x), f"act kind {kind}")
        o.pads_intact(f"act kind {kind}")


def test_add_rmsnorm_first_abi_name(dev):
    """cbx_add_rmsnorm_f32 (the first ABI's name of cbx_add_norm_f32 with rms = 1 and no bias; no wrapper in ops.py): the same bits as ops.add_rmsnorm, and fp64."""
    from chatterbox_amd import ops
    from chatterbox_amd._lib import check
    rows, C, ks = 5, 1024, 2
    x, part, w = _r((rows, C), 1, 2.0), _r((ks, rows, C), 2).to(dev), (1 + 0.1 * _r((C,), 3)).to(dev)
    xa, xb, ha, hb = x.clone().to(dev), _View(x, dev, 4), torch.empty(rows, C).to(dev), _out((rows, C), dev, 8)
    ops.add_rmsnorm(xa, part, w, ha)
    check(ops.lib.cbx_add_rmsnorm_f32(xb.v.data_ptr(), part.data_ptr(), ks, part.stride(0), part.stride(1), w.data_ptr(), hb.v.data_ptr(), rows, C, xb.v.stride(0),
                                      hb.v.stride(0), 1e-5, ops._stream()), "cbx_add_rmsnorm_f32")
    assert torch.equal(xa.cpu(), xb.v.cpu()) and torch.equal(ha.cpu(), hb.v.cpu())
    s = x.double() + part.cpu().double().sum(0)
    _close(hb.v, s * torch.rsqrt((s * s).mean(-1, keepdim=True) + 1e-5) * w.cpu().double(), 2e-5, "add_rmsnorm")
    hb.pads_intact("add_rmsnorm h")


@pytest.mark.parametrize("T,causal", [(130, False), (103, True)])
def test_flash_attn_plane_output(dev, T, causal):
    """cbx_flash_attn_split_po (fp32 q / k / v in, plane-format output; no wrapper in ops.py): the split of what cbx_flash_attn_split_f32 gives at precision 16
    (the bound of tests/test_planes_gpu.py's plane outputs: 2**-21 of the largest value), and test_split_flash_attn's 2e-5 against torch."""
    from chatterbox_amd import ops
    from chatterbox_amd._lib import check
    Z, H = 2, 4
    qkv = _r((Z, T, 3, H, 64), 1)
    lens = torch.tensor([T, max(1, T - 37)], dtype=torch.int32)
    q, k, v = (qkv[:, :, i].transpose(1, 2).double() for i in range(3))
    if causal:
        ref, kl = F.scaled_dot_product_attention(q, k, v, is_causal=True), None
    else:
        bias = torch.zeros(Z, 1, 1, T, dtype=torch.float64)
        for z in range(Z):
            bias[z, ..., int(lens[z]):] = -1e10
        ref, kl = F.scaled_dot_product_attention(q, k, v, attn_mask=bias), lens.to(dev)
    d = qkv.to(dev)
    out, outP = torch.empty(Z, T, H, 64).to(dev), ops.Planes(Z * T, H * 64, dev, zero=True)
    with ops.gemm_precision(16):
        ops.flash_attn(d[:, :, 0], d[:, :, 1], d[:, :, 2], out, 0.125, key_lens=kl, causal=causal)
    qq, kk, vv = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    check(ops.lib.cbx_flash_attn_split_po(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), outP.ptr, None if kl is None else kl.data_ptr(), Z, H, T, T, qq.stride(0), qq.stride(1),
                                          kk.stride(0), kk.stride(1), vv.stride(0), vv.stride(1), T * outP.ld, outP.ld, outP.lo, 0.125, int(causal), ops._stream()),
          "cbx_flash_attn_split_po")
    got = outP.float().view(Z, T, H, 64)
    assert float((got - out).abs().max()) <= 2.0 ** -21 * float(out.abs().max()), "plane output = split of the fp32 output"
    _close(got, ref.transpose(1, 2), 2e-5, "flash attention, plane output")
