"""Adversarial-statistics tests (-m gpu; the same bodies run on the SIMT emulator) for every kernel that computes a row's mean, variance or rstd: the row
LayerNorm / RMSNorm kernels (generic, narrow, statistics-only, plane output), the LayerNorm epilogue of the plane GEMM, the LayerNorm-folded A operand of the
split GEMM, cbx_add_norm_f32, the RMSNorm- and LayerNorm-folded decode GEMVs (one-tile, column-tile, partial-sum operand, narrow tiles, bf16 weights, epilogue
prefetch), the LayerNorm operand of the few-row GEMV and the statistics pooling.  The other suites draw rows from N(0.3 .. 0.5, 1 .. 3): |mean| <= std and no
outlier channel, so every way of computing a variance agrees to rounding.  Here the ROWS are prescribed.

Construction (inputs exact, so the tolerances of the neighbouring suites apply unchanged and only the statistics machinery is measured):
  * d: seeded integers in [-32, 32] divided by 8, built in antisymmetric pairs (sum d = 0 exactly), then permuted over the channels with a seeded permutation so
    that the two members of a pair land in different lanes and waves.  Every value of a row has <= 14 significant bits (one plane pair holds it);
  * patterns over one row of C channels:  centred d | offset32, offset1024, neg1024: +-offset + d | outlier_first / _mid / _last: d with one channel (0, C/2,
    C - 1) set to 12 C and its pair partner to 0 -- the mean is exactly 12 -- | constant: every channel 7.5 (variance 0: a two-pass LayerNorm returns its bias
    bit for bit) | small_eps: d 2^-20 with eps = 1e-12 (variance comparable to eps) | big: d 2^40 (skipped where an operand must fit fp16 planes);
  * the reference (_stats) asserts that its fp64 row sum, mean and centred sum of squares equal the fp32 evaluation of the same expressions wherever
    sum |x| (resp. sum (x - mean)^2) in units of the row's granularity stays below 2^24 -- then every partial sum is exact in fp32 in ANY order.  That holds
    for every pattern at C <= 1024 except the centred squares of the outlier rows, and not for the +-1024 offsets at C = 4096 (the sum reaches 2^25 units);
  * LayerNorm weights and biases are seeded multiples of 1/64 near 1 and 0; GEMV / GEMM weights are plain N(0, 1/sqrt(K)): the contraction keeps its noise;
  * one launch holds rows of DIFFERENT patterns next to each other (37 rows for the row kernels -- 77 for the narrow C = 256 kernel, which serves >= 64 rows --,
    M in {1, 5, 16} for the decode GEMVs and 33 for the LayerNorm fold of the one-tile kernel (three row tiles), M <= 4 for the few-row GEMV); launches are grouped by eps (1e-5: every pattern but small_eps; 1e-12: small_eps,
    centred, constant); outputs are strided views whose pad elements must come back untouched.

Reference: fp64 on the CPU from the same fp32 inputs.  Tolerances, form err <= tol (1 + |ref|), those of each kernel's parity test: 2e-5 the row kernels,
planes and add_norm; 5e-5 the few-row GEMV and the folded GEMVs (one-tile forms); 1e-4 max(1, sqrt(K / 256)) the column-tile forms; 3e-5 the LayerNorm-folded
split GEMM at precision 16 (_SPLIT_TOL[16] of tests/test_ops_gpu.py).  Every comparison prints `NORMSTRESS <kernel> <pattern> <max err> (tol ...)` before it asserts (profiles/norm_stress_tests.log: the figures of the SIMT
emulator and of the MI355X; the one-pass fold on the unshifted row had 1.1e-2 at offset 1024).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PATTERNS = ("centred", "offset32", "offset1024", "neg1024", "outlier_first", "outlier_mid", "outlier_last", "constant", "small_eps", "big")
OFFSETS = {"offset32": 32.0, "offset1024": 1024.0, "neg1024": -1024.0}
SCALE = {"small_eps": 2.0 ** -20, "big": 2.0 ** 40}
EPS_GROUPS = ((1e-5, tuple(p for p in PATTERNS if p != "small_eps")), (1e-12, ("small_eps", "centred", "constant")))
RMS_FOLD_PATTERNS = ("centred", "outlier_first", "outlier_mid", "outlier_last", "constant", "big")
MEASURED = {}  # (kernel, pattern) -> largest |got - ref| seen in this process
SENT = -12345.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _row(pattern, C, seed):
    """One row of `pattern` as two exact fp64 summands (large part, small part): the offset / the outlier / the constant, and d."""
    g = _gen(seed)
    half = C // 2
    v = torch.randint(-32, 33, (half,), generator=g).double() / 8
    base = torch.cat([v, -v, torch.zeros(C - 2 * half, dtype=torch.float64)])
    perm = torch.randperm(C, generator=g)
    inv = torch.empty(C, dtype=torch.long)
    inv[perm] = torch.arange(C)
    d, big = base[perm].clone(), torch.zeros(C, dtype=torch.float64)
    if pattern in OFFSETS:
        big[:] = OFFSETS[pattern]
    elif pattern.startswith("outlier_"):
        p = {"first": 0, "mid": C // 2, "last": C - 1}[pattern[8:]]
        b = int(perm[p])
        if b < 2 * half:  # (an odd row's unpaired zero has no partner)
            d[inv[(b + half) % (2 * half)]] = 0.0
        d[p], big[p] = 0.0, 12.0 * C
    elif pattern == "constant":
        d[:], big[:] = 0.0, 7.5
    else:
        assert pattern in ("centred", "small_eps", "big"), pattern
        d *= SCALE.get(pattern, 1.0)
    return big, d


@functools.lru_cache(maxsize=None)
def _rows(names, C, seed):
    """Rows of the patterns `names` (a tuple): fp32 (large parts, small parts, rows) with rows == large + small exactly."""
    parts = [_row(p, C, seed * 1000 + r) for r, p in enumerate(names)]
    big, small = torch.stack([b for b, _ in parts]), torch.stack([s for _, s in parts])
    x = (big + small).float()
    assert torch.equal(x.double(), big + small) and torch.equal(big.float().double(), big) and torch.equal(small.float().double(), small), "the test's own inputs are not exact in fp32"
    return big.float(), small.float(), x


def _launches(M, patterns=None, groups=EPS_GROUPS):
    """(eps, names) of the launches of M rows that cover every pattern of each eps group (rows of a launch cycle through the group)."""
    for eps, group in groups:
        group = tuple(p for p in group if patterns is None or p in patterns)
        for i in range(-(-len(group) // M) if group else 0):
            yield eps, tuple(group[(i * M + r) % len(group)] for r in range(M))


def _stats(x, names, axis=-1):
    """fp64 (mean, biased variance) over `axis` of the fp32 rows x; asserted equal to the fp32 evaluation of the same expressions wherever every partial sum
    is exact in fp32 in any order (module docstring).  Returns also the rows whose sum resp. variance carries that promise."""
    x = x.transpose(axis, -1) if axis != -1 else x
    xd, C = x.double(), x.shape[-1]
    unit = torch.tensor([2.0 ** -3 * SCALE.get(p, 1.0) for p in names], dtype=torch.float64)
    s = xd.sum(-1)
    mean = s / C
    q = ((xd - mean[:, None]) ** 2).sum(-1)
    sum_ok = xd.abs().sum(-1) / unit < 2 ** 24
    mean_ok = sum_ok & (mean.float().double() == mean)
    var_ok = mean_ok & (q / unit ** 2 < 2 ** 24)
    m32 = x.sum(-1) / C
    q32 = ((x - m32[:, None]) ** 2).sum(-1)
    assert torch.equal(x.sum(-1).double()[sum_ok], s[sum_ok]) and torch.equal(m32.double()[mean_ok], mean[mean_ok]), "the test's own rows do not sum exactly in fp32"
    assert torch.equal(q32.double()[var_ok], q[var_ok]), "the test's own centred squares do not sum exactly in fp32"
    for r, p in enumerate(names):
        if C <= 1024 and C % 2 == 0:
            assert bool(mean_ok[r]), f"{p}: the row mean is promised exact at C = {C}"
            assert bool(var_ok[r]) or p.startswith("outlier_"), f"{p}: the variance is promised exact at C = {C}"
        if p.startswith("outlier_") and C % 2 == 0:
            assert float(mean[r]) == 12.0
    return mean, q / C, mean_ok, var_ok


def _ln_ref(x, names, w, b, eps, rms=False):
    xd = x.double()
    if rms:
        return xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps) * w.double()
    mean, var, _, _ = _stats(x, names)
    return (xd - mean[:, None]) * torch.rsqrt(var + eps)[:, None] * w.double() + (0 if b is None else b.double())


def _wb(C, seed):
    """LayerNorm weight and bias: seeded multiples of 1/64 near 1 and 0."""
    g = _gen(seed)
    return 1 + torch.randint(-8, 9, (C,), generator=g).float() / 64, torch.randint(-8, 9, (C,), generator=g).float() / 64


def _check(got, ref, kernel, names, what, tol, rel=False):
    """Rows of got / ref belong to the patterns `names`: one figure and one NORMSTRESS line per pattern, then the assertion over all of them."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and got.shape[0] == len(names), (got.shape, ref.shape, len(names))
    err = (got - ref).abs()
    err = torch.nan_to_num(err, nan=math.inf).reshape(len(names), -1)
    lim = (tol * (ref.abs() if rel else 1.0 + ref.abs())).reshape(len(names), -1)
    fails = []
    for p in dict.fromkeys(names):
        rows = [r for r, n in enumerate(names) if n == p]
        e = float(err[rows].max()) if err[rows].numel() else 0.0
        MEASURED[(kernel, p)] = max(MEASURED.get((kernel, p), 0.0), e)
        print(f"NORMSTRESS {kernel} {p} {e:.3e} (tol {tol:g}, {what})")
        bad = ~(err[rows] <= lim[rows])
        if bad.any():
            fails.append(f"{p}: max err {e:.3e} (ref max {float(ref.reshape(len(names), -1)[rows].abs().max()):.3e}), {int(bad.sum())} / {bad.numel()} over tol {tol}")
    assert not fails, f"{kernel} {what}: " + "; ".join(fails)


class _View:
    """tests/test_frontend_ops_gpu.py::_View: a (rows, C) tensor inside a wider buffer full of SENT; `v` is the strided view handed to the kernel."""

    def __init__(self, t, dev, pad=8):
        from test_frontend_ops_gpu import _View as V
        self._v = V(t, dev, pad)
        self.v, self.pads_intact = self._v.v, self._v.pads_intact


def _out(shape, dev, pad=8):
    return _View(torch.full(shape, SENT), dev, pad)


def _planes_exact(x):
    """What a planes tensor holds for fp32 x: h + l / 2048 in fp64 (tests/test_planes_gpu.py)."""
    h = x.half()
    l = ((x.double() - h.double()) * 2048.0).half()
    return h.double() + l.double() / 2048.0


def _const_rows(names):
    return [r for r, p in enumerate(names) if p == "constant"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) cbx_layernorm_f32, (b) cbx_row_stats_f32 + the ln_stats fold of cbx_gemm_f32, (c) cbx_layernorm_planes_f32, (d) the LayerNorm epilogue of cbx_gemm_planes
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows", [(80, 37), (512, 37), (1024, 37), (4096, 37), (256, 37), (256, 77)])
def test_layernorm_stress(dev, C, rows, patterns=None):
    """cbx_layernorm_f32: LayerNorm, LayerNorm + Mish + post_add and RMSNorm; the generic kernel (one wave per row) and, at C = 256 with >= 64 rows, the narrow
    one (16 lanes per row).  A constant row gives the bias bit for bit."""
    from chatterbox_amd import ops
    kind = "narrow" if C == 256 and rows >= 64 else "generic"
    w, b = _wb(C, 1)
    pa = _wb(C, 2)[1]
    for eps, names in _launches(rows, patterns):
        x = _rows(names, C, 3)[2]
        xv = _View(x, dev, 4)
        for form in ("ln", "ln_mish", "rms"):
            out = _out((rows, C), dev)
            if form == "ln":
                ops.layernorm(xv.v, w.to(dev), b.to(dev), out.v, eps)
                ref = _ln_ref(x, names, w, b, eps)
                cr = _const_rows(names)
                assert torch.equal(out.v[cr].cpu(), b.expand(len(cr), C)), "a constant row: the LayerNorm bias bit for bit"
            elif form == "ln_mish":
                ops.layernorm(xv.v, w.to(dev), b.to(dev), out.v, eps, act=ops.MISH, post_add=pa.to(dev))
                ref = F.mish(_ln_ref(x, names, w, b, eps)) + pa.double()
            else:
                ops.layernorm(xv.v, w.to(dev), None, out.v, eps, rms=True)
                ref = _ln_ref(x, names, w, None, eps, rms=True)
            _check(out.v, ref, f"layernorm_{kind}_{form}", names, f"C {C} rows {rows} eps {eps:g}", 2e-5)
            out.pads_intact(f"layernorm {form}")


def test_row_stats_stress(dev, rows=37, patterns=None):
    """cbx_row_stats_f32 (C = 256): the mean bit-equal to the fp64 mean wherever the row sums exactly, rstd within 5e-7 relative wherever the variance is exact
    (then: one division, one addition, one rsqrtf), 2e-5 otherwise; then the same statistics through the ln_stats fold of cbx_gemm_f32 at precision 16."""
    from chatterbox_amd import ops
    C, N = 256, 64
    g, be = _wb(C, 4)
    w, bias = torch.randn(N, C, generator=_gen(5)) / 16, torch.randn(N, generator=_gen(6))
    for eps, names in _launches(rows, patterns):
        x = _rows(names, C, 7)[2]
        mean, var, mean_ok, var_ok = _stats(x, names)
        xv = _View(x, dev, 4)
        stats = torch.full((rows, 2), SENT).to(dev)
        ops.row_stats(xv.v, stats, eps)
        st = stats.cpu()
        assert torch.equal(st[:, 0].double()[mean_ok], mean[mean_ok]), "row_stats: the mean of an exactly summable row"
        _check(st[:, :1], mean[:, None], "row_stats_mean", names, f"eps {eps:g}", 2e-5)
        rstd = torch.rsqrt(var + eps)[:, None]
        ex = [r for r in range(rows) if var_ok[r]]
        _check(st[ex, 1:], rstd[ex], "row_stats_rstd", tuple(names[r] for r in ex), f"exact variance, relative, eps {eps:g}", 5e-7, rel=True)
        _check(st[:, 1:], rstd, "row_stats_rstd_all", names, f"relative, eps {eps:g}", 2e-5, rel=True)
        out = _out((rows, N), dev)
        with ops.gemm_precision(16):
            assert ops.ln_fusable(rows, C, xv.v.stride(0))
            ops.linear(xv.v, w.to(dev), out.v, bias=bias.to(dev), ln=(stats, g.to(dev), be.to(dev)))
        _check(out.v, F.linear(_ln_ref(x, names, g, be, eps), w.double(), bias.double()), "gemm_ln_fold", names, f"M {rows} N {N} K {C} eps {eps:g}", 3e-5)
        out.pads_intact("gemm ln fold")


def test_layernorm_planes_stress(dev, rows=37, patterns=None):
    """cbx_layernorm_planes_f32 (C = 256) against the plane pair of the fp64 result."""
    from chatterbox_amd import ops
    C = 256
    w, b = _wb(C, 8)
    for eps, names in _launches(rows, patterns):
        x = _rows(names, C, 9)[2]
        out = ops.Planes(rows, C, dev, zero=True)
        ops.layernorm_planes(_View(x, dev, 4).v, w.to(dev), b.to(dev), out, eps)
        _check(out.float(), _planes_exact(_ln_ref(x, names, w, b, eps).float()), "layernorm_planes", names, f"rows {rows} eps {eps:g}", 2e-5)


@pytest.mark.parametrize("res", [False, True])
def test_gemm_planes_layernorm_epilogue_stress(dev, res, M=37, patterns=None):
    """The LayerNorm epilogue of cbx_gemm_planes (N = K = 256): the row is prescribed by A = pattern rows (planes) and W = the identity; with `res` the fp32
    residual carries the large part (offset, outlier, constant) and A the small one.  Both the fp32 row C and the plane LayerNorm LNP are checked."""
    from chatterbox_amd import ops
    N = K = 256
    lw, lb = _wb(N, 10)
    wP = ops.split_planes(torch.eye(N).to(dev))
    for eps, names in _launches(M, tuple(p for p in (patterns or PATTERNS) if p != "big")):
        big, small, x = _rows(names, K, 11)
        a = small if res else x
        row = (_planes_exact(a) + (big.double() if res else 0)).float()
        keep = [r for r in range(M) if torch.equal(_planes_exact(a[r]), a[r].double())]
        assert all(names[r] == "small_eps" for r in range(M) if r not in keep), "every row but the 2^-20 one fits a plane pair exactly"
        out = big.clone().to(dev) if res else torch.full((M, N), SENT).to(dev)
        lnP = ops.Planes(M, N, dev, zero=True)
        ops.gemm_planes(ops.split_planes(a.to(dev)), wP, M=M, N=N, K=K, C=out, R=out if res else None, ldc=N, ldr=N if res else 0, ln=(lw.to(dev), lb.to(dev)), lnp=lnP,
                        ln_eps=eps)
        _check(out, row, f"gemm_planes_row_res{int(res)}", names, f"M {M} eps {eps:g}", 2e-5)
        ref = _ln_ref(row[keep], tuple(names[r] for r in keep), lw, lb, eps)
        _check(lnP.float()[keep], _planes_exact(ref.float()), f"gemm_planes_ln_res{int(res)}", tuple(names[r] for r in keep), f"M {M} eps {eps:g}", 2e-5)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (e) cbx_add_norm_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _channel_parts(t, ks):
    """t as ks summands that partition its channels (channel c goes to part c % ks): their sum is t exactly, in any order."""
    m = torch.arange(t.shape[-1]) % ks
    return torch.stack([t * (m == j) for j in range(ks)])


@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("C", [768, 1024])
def test_add_norm_stress(dev, C, ks, rows=37, patterns=None):
    """cbx_add_norm_f32, LayerNorm and RMSNorm form: x + sum of the parts equals the pattern -- the large part in x and d in the parts, then the other way round."""
    from chatterbox_amd import ops
    w, b = _wb(C, 12)
    for eps, names in _launches(rows, patterns):
        big, small, x = _rows(names, C, 13)
        for where, (x0, rest) in (("offset_in_x", (big, small)), ("offset_in_parts", (small, big))):
            for rms in (False, True):
                xv, h = _View(x0, dev, 4), _out((rows, C), dev)
                ops.add_rmsnorm(xv.v, _channel_parts(rest, ks).to(dev), w.to(dev), h.v, eps, bias=None if rms else b.to(dev), rms=rms)
                assert torch.equal(xv.v.cpu(), x), "add_norm: the residual stream is x + sum of the parts, exactly"
                _check(h.v, _ln_ref(x, names, w, None if rms else b, eps, rms=rms), "add_norm_rms" if rms else "add_norm_ln", names, f"C {C} ks {ks} {where} eps {eps:g}", 2e-5)
                if not rms:
                    cr = _const_rows(names)
                    assert torch.equal(h.v[cr].cpu(), b.expand(len(cr), C)), "a constant row: the LayerNorm bias bit for bit"
                h.pads_intact("add_norm h")
                xv.pads_intact("add_norm x")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (f), (g) cbx_gemv_f32 with the RMSNorm / LayerNorm fold
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemv_w(N, K, seed):
    w, bias = torch.randn(N, K, generator=_gen(seed)) / math.sqrt(K), torch.randn(N, generator=_gen(seed + 1))
    return w, bias, w.double(), w.bfloat16().float()


def _unpack(img, rows, K):
    from test_ops_gpu import _unpack_operand
    return _unpack_operand(img, rows, K)[:rows].cpu()


@pytest.mark.parametrize("M", [1, 5, 16])
def test_gemv_rms_fold_stress(dev, M, patterns=RMS_FOLD_PATTERNS):
    """cbx_gemv_f32 with LlamaRMSNorm folded in (K = 1024): plain (N = 64), SwiGLU (64 features) and col_tiles = 2 (bit-identical to the one-tile form)."""
    from chatterbox_amd import ops
    K, N = 1024, 64
    nw_, _ = _wb(K, 14)
    w, _, wd, _ = _gemv_w(N, K, 15)
    gu, _, gud, _ = _gemv_w(2 * N, K, 17)
    wp, gup = ops.pack_gemv_weight(w.to(dev)), ops.pack_gemv_weight(gu.to(dev), swiglu=True)
    kw = dict(M=M, K=K, nw=8, w_packed=True, x_packed=True, norm_w=nw_.to(dev))
    for eps, names in _launches(M, patterns, EPS_GROUPS[:1]):
        x = _rows(names, K, 19)[2]
        xp = ops.pack_gemv_weight(x.to(dev))
        hn = _ln_ref(x, names, nw_, None, eps, rms=True)
        a, c, s = _out((M, N), dev), _out((M, N), dev), _out((M, N), dev)
        ops.gemv(xp, wp, a.v, N=N, eps=eps, **kw)
        ops.gemv(xp, wp, c.v, N=N, eps=eps, col_tiles=2, **kw)
        ops.gemv(xp, gup, s.v, N=N, eps=eps, swiglu=True, **kw)
        _check(a.v, hn @ wd.t(), "gemv_rms", names, f"M {M}", 5e-5)
        assert torch.equal(a.v, c.v), "col_tiles = 2 (RMSNorm form) differs from the one-tile kernel"
        _check(c.v, hn @ wd.t(), "gemv_rms_ct2", names, f"M {M}", 1e-4 * max(1.0, math.sqrt(K / 256)))
        _check(s.v, F.silu(hn @ gud[:N].t()) * (hn @ gud[N:].t()), "gemv_rms_swiglu", names, f"M {M}", 5e-5)
        for o in (a, c, s):
            o.pads_intact("gemv rms fold")


def test_gemv_rms_fold_split_k_into_attention_stress(dev, M=5, patterns=RMS_FOLD_PATTERNS):
    """col_tiles = 2 with ksplit = 2: un-normalised q | k | v partial sums + per-slice sums of squares, folded by cbx_decode_attn_rope (qkv_nparts = 2, qkv_ssq): one
    layer, one head, context 17, identity RoPE table, against fp64 attention on the RMSNorm'ed projection."""
    from chatterbox_amd import ops
    K, H, ctx, maxp = 1024, 1, 17, 32
    N = 3 * H * 64
    nw_, _ = _wb(K, 14)
    w, _, wd, _ = _gemv_w(N, K, 21)
    wp = ops.pack_gemv_weight(w.to(dev))
    pos = torch.full((M,), ctx - 1, dtype=torch.int32)
    kc0, vc0 = torch.randn(M, H, maxp, 64, generator=_gen(22)), torch.randn(M, H, maxp, 64, generator=_gen(23))
    cos, sin = torch.ones(maxp, 64).to(dev), torch.zeros(maxp, 64).to(dev)
    tol = 1e-4 * max(1.0, math.sqrt(K / 256))
    for eps, names in _launches(M, patterns, EPS_GROUPS[:1]):
        x = _rows(names, K, 24)[2]
        parts, ssq = torch.full((2, M, N), SENT).to(dev), torch.zeros(2, 16).to(dev)
        ops.gemv(ops.pack_gemv_weight(x.to(dev)), wp, parts, N=N, M=M, K=K, nw=8, w_packed=True, x_packed=True, norm_w=nw_.to(dev), eps=eps, col_tiles=2, ksplit=2, ssq_out=ssq)
        qkv = _ln_ref(x, names, nw_, None, eps, rms=True) @ wd.t()
        got = (parts[0] + parts[1]).cpu().double() * torch.rsqrt((ssq[0] + ssq[1]).cpu().double()[:M] / K + eps)[:, None]
        _check(got, qkv, "gemv_rms_ct2_ks2", names, f"M {M}: fold of the two K slices", tol)
        kc, vc, out = kc0.clone().to(dev), vc0.clone().to(dev), torch.full((M, H * 64), SENT).to(dev)
        ops.decode_attn_rope(parts, pos.to(dev), cos, sin, kc, vc, out, 0.125, geom=ops.DecodeAttnGeom(dev), qkv_ssq=ssq, rms_dim=K, rms_eps=eps)
        q, k, v = (qkv.view(M, 3, H, 64)[:, i] for i in range(3))
        kk, vv = torch.cat([kc0[:, :, : ctx - 1].double(), k[:, :, None]], 2), torch.cat([vc0[:, :, : ctx - 1].double(), v[:, :, None]], 2)
        att = torch.einsum("mhk,mhkd->mhd", torch.softmax(torch.einsum("mhd,mhkd->mhk", q, kk) * 0.125, -1), vv)
        _check(out, att.reshape(M, H * 64), "gemv_rms_ct2_ks2_attn", names, f"M {M} context {ctx}", tol)


@pytest.mark.parametrize("M", [1, 5, 16, 33])
@pytest.mark.parametrize("N", [70, 6563])
@pytest.mark.parametrize("K", [768, 1024])
def test_gemv_layernorm_fold_stress(dev, K, N, M, patterns=None):
    """cbx_gemv_f32 with the GPT-2 LayerNorm folded in (ln_cw / ln_cb): the one-tile kernel, CBX_GEMV_PRE_EPI, n_xpart = 2 / 4 (large part in x and d in the partial
    images, and the reverse; x_out receives the unshifted sum exactly), col_tiles = 2, half_tile = 12, bf16 weights (reference and fold constants from the rounded
    weights) and the gelu_new epilogue.  PRE_EPI, col_tiles, half_tile and the partial-sum operand are bit-identical to the one-tile kernel on the summed row; bf16
    weights to the fp32 kernel on the rounded weights.  M = 33 (three row tiles, each lane with a pivot per tile): the forms the entry point admits past 16 rows --
    one-tile, PRE_EPI, half_tile, gelu_new."""
    from chatterbox_amd import ops
    lw, lb = _wb(K, 25)
    w, bias, wd, wr = _gemv_w(N, K, 26)
    fold = lambda w64: ((w64 @ lw.double()).float().to(dev), (w64 @ lb.double() + bias.double()).float().to(dev))
    cw, cb = fold(wd)
    cwr, cbr = fold(wr.double())
    wp, wp12, wpr, wpb = (ops.pack_gemv_weight(w.to(dev)), ops.pack_gemv_weight(w.to(dev), half_tile=12), ops.pack_gemv_weight(wr.to(dev)),
                          ops.pack_gemv_weight(w.to(dev), bf16=True))
    tol_ct = 1e-4 * max(1.0, math.sqrt(K / 256))
    for eps, names in _launches(M, patterns):
        big, small, x = _rows(names, K, 27)
        what = f"M {M} N {N} K {K} eps {eps:g}"
        xp = ops.pack_gemv_weight(x.to(dev))
        kw = dict(N=N, M=M, K=K, nw=8, w_packed=True, x_packed=True, norm_w=lw.to(dev), eps=eps)
        ln = _ln_ref(x, names, lw, None, eps)  # (the LayerNorm bias lives in ln_cb)
        ref, ref_r = ln @ wd.t() + cb.cpu().double(), ln @ wr.double().t() + cbr.cpu().double()

        def run(image, xop=xp, cwb=(cw, cb), **extra):
            o = _out((M, N), dev)
            ops.gemv(xop, image, o.v, ln_cw=cwb[0], ln_cb=cwb[1], **kw, **extra)
            o.pads_intact(f"gemv layernorm fold {sorted(extra)}")
            return o.v

        one = run(wp)
        _check(one, ref, "gemv_ln", names, what, 5e-5)
        cr = _const_rows(names)
        assert torch.equal(one[cr].cpu(), cb.cpu().expand(len(cr), N)), "a constant row: ln_cb itself"
        assert torch.equal(run(wp, flags=ops.gemv_flags(pre_epi=1)), one), "CBX_GEMV_PRE_EPI differs from the plain form"
        assert torch.equal(run(wp12, half_tile=12), one), "half_tile = 12 differs from the 16-column form"
        _check(run(wp, act=ops.GELU_TANH), F.gelu(ref, approximate="tanh"), "gemv_ln_gelu", names, what, 5e-5)
        if M > 16:  # col_tiles, bf16 weights and the partial-sum operand serve M <= 16
            continue
        ct = run(wp, col_tiles=2)
        assert torch.equal(ct, one), "col_tiles = 2 (LayerNorm form) differs from the one-tile kernel"
        _check(ct, ref, "gemv_ln_ct2", names, what, tol_ct)
        b16 = run(wpb, cwb=(cwr, cbr))
        assert torch.equal(b16, run(wpr, cwb=(cwr, cbr))), "bf16 weights differ from the fp32 kernel on the rounded weights"
        _check(b16, ref_r, "gemv_ln_bf16", names, what, 5e-5)
        for np_ in (2, 4):
            for where, (x0, rest) in (("offset_in_x", (big, small)), ("offset_in_parts", (small, big))):
                for ctk in (0, 2):
                    pp = torch.stack([ops.pack_gemv_weight(t.contiguous().to(dev)) for t in _channel_parts(rest, np_)])
                    x_out = torch.zeros(16, K).to(dev)
                    got = run(wp, xop=ops.pack_gemv_weight(x0.to(dev)), xpart=pp, x_out=x_out, col_tiles=ctk)
                    assert torch.equal(_unpack(x_out, M, K), x), f"n_xpart {np_} {where}: x_out is the unshifted x + sum of the partial images"
                    assert torch.equal(got, one), f"n_xpart {np_} {where} col_tiles {ctk}: differs from the one-tile kernel on the summed row"
                    _check(got, ref, f"gemv_ln_np{np_}" + ("_ct2" if ctk else ""), names, f"{what} {where}", tol_ct if ctk else 5e-5)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (h) cbx_gemv_row_f32 with the LayerNorm operand, (j) the two LayerNorm paths of the GPT-2 decode step on the same rows
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [256, 768, 1024])
def test_gemv_row_layernorm_stress(dev, K, M, R, N=70, patterns=None):
    """cbx_gemv_row_f32, LayerNorm(x) as the operand (two-pass), strided x and out."""
    from chatterbox_amd import ops
    lw, lb = _wb(K, 28)
    w, bias, wd, _ = _gemv_w(N, K, 29)
    for eps, names in _launches(M, patterns):
        x = _rows(names, K, 30)[2]
        out = _out((M, N), dev)
        ops.gemv_row(_View(x, dev, 4).v, w.to(dev), out.v, bias=bias.to(dev), ln=(lw.to(dev), lb.to(dev)), eps=eps, rows_per_wave=R)
        _check(out.v, _ln_ref(x, names, lw, lb, eps) @ wd.t() + bias.double(), "gemv_row_ln", names, f"M {M} N {N} K {K} rows_per_wave {R} eps {eps:g}", 5e-5)
        out.pads_intact("gemv_row")


@pytest.mark.parametrize("K", [768, 1024])
def test_layernorm_paths_agree_on_offset_rows(dev, K, N=70):
    """The same 3 offset1024 rows through the few-row path (cbx_gemv_row_f32, LayerNorm operand: what the GPT-2 decode step runs for <= 2 rows) and through the
    folded cbx_gemv_f32 (more rows): within the sum of their two tolerances of each other, and each within its own of fp64."""
    from chatterbox_amd import ops
    M, names = 3, ("offset1024",) * 3
    lw, lb = _wb(K, 31)
    w, bias, wd, _ = _gemv_w(N, K, 32)
    x = _rows(names, K, 33)[2]
    ref = _ln_ref(x, names, lw, lb, 1e-5) @ wd.t() + bias.double()
    a, b = torch.full((M, N), SENT).to(dev), torch.full((M, N), SENT).to(dev)
    ops.gemv_row(x.to(dev), w.to(dev), a, bias=bias.to(dev), ln=(lw.to(dev), lb.to(dev)))
    ops.gemv(ops.pack_gemv_weight(x.to(dev)), ops.pack_gemv_weight(w.to(dev)), b, N=N, M=M, K=K, nw=8, w_packed=True, x_packed=True, norm_w=lw.to(dev),
             ln_cw=(wd @ lw.double()).float().to(dev), ln_cb=(wd @ lb.double() + bias.double()).float().to(dev))
    _check(a, ref, "path_gemv_row", names, f"K {K}", 5e-5)
    _check(b, ref, "path_gemv_fold", names, f"K {K}", 5e-5)
    _check(a.cpu().double() - b.cpu().double() + ref, ref, "path_consistency", names, f"K {K}: few-row path against folded path", 1e-4)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (i) cbx_stats_pool_f32: the patterns run along time, one channel per pattern
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 512])
def test_stats_pool_stress(dev, T, patterns=PATTERNS):
    """Mean and unbiased std over time.  T = 1 has no unbiased std: the entry point rejects it (T >= 2), as tests/test_frontend_ops_gpu.py documents."""
    from chatterbox_amd import ops
    C = len(patterns)
    x = _rows(tuple(patterns), T, 34)[2].t().contiguous()  # (T, C)
    xv = _View(x, dev, 7)
    out = torch.full((2 * C + 2,), SENT).to(dev)
    if T == 1:
        with pytest.raises(RuntimeError, match="T >= 2"):
            ops.stats_pool(xv.v, out)
        return
    ops.stats_pool(xv.v, out)
    mean, var, _, _ = _stats(x.t(), tuple(patterns))
    _check(out[:C, None], mean[:, None], "stats_pool_mean", tuple(patterns), f"T {T}", 2e-5)
    _check(out[C:2 * C, None], torch.sqrt(var * T / (T - 1))[:, None], "stats_pool_std", tuple(patterns), f"T {T}", 2e-5)
    assert out[2 * C:].tolist() == [SENT, SENT]
    xv.pads_intact("stats_pool")
