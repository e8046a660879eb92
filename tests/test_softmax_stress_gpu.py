"""Adversarial-score tests (-m gpu) for every kernel that carries its own running (m, l, O) softmax update: the flash attentions (exact fp32, keys
from the KV cache, split precisions 3 / 6 / 16, plane output, rel-pos, plane format in every version), the materialised softmax (rel-pos and plain rows)
and the decode attentions (two-pass, fused RoPE in its plain / pipelined / split-context forms, the part records + their merge in cbx_gemv_row_f32).
The other suites draw q, k from N(0, 1): scores of +-4 and a running maximum that settles in the first key tile, so the data-dependent branches (rescale,
"no key seen yet", merges of partial triples) hardly run.  Here the SCORES are prescribed per key.

Construction (scores exact in every numerics mode, so the tolerances of the neighbouring suites apply unchanged and only the softmax machinery is measured):
  * scale = 0.125; every q / k entry is a multiple of 1/8 with at most 8 significant bits (exact in one bf16 / fp16 plane), |raw score| < 2**11: every
    product and partial sum of q . k is exact in fp32, bf16x3, bf16x6, f16x3 and the plane format, in any summation order;
  * dims 0 .. 15 of a head carry the pattern: q = 1 there and k_j = c_j / 2, i.e. a scaled score of exactly c_j; the other 48 dims hold seeded noise in
    [-1, 1] quantised to 1/8 (scaled contribution of about +-0.5).  Keys that carry a spike, and every key of `flat`, have NO noise: their weights are then
    the stated exact ones (one-hot, 1/2 - 1/2, l = Tk);
  * V is plain N(0, 1);
  * the reference asserts that its fp64 scores equal its fp32 scores: an inexact input fails the test itself, not the kernel;
  * RoPE kernels get the identity table (cos 1, sin 0) or a quarter turn (cos 0, sin 1): rotations that keep the entries exact (the raw q / k rows are
    the inverse rotation of the wanted ones).

Patterns over the valid keys j < n:  asc c_j = j/2 (every tile raises the maximum) | desc c_j = -j/2 | late_spike +48 on key n-1 | first_spike +48 on key 0
| two +40 on keys 3 and n-2 | flat c_j = 3 | neg c_j = -60 | masked_spike: noise only, and a finite +128 on a key the mask must hide (beyond key_lens[z];
above the causal horizon of the compared queries; position pos + 1 of the stale cache) -- the output must equal the run without it bit for bit.

Reference: materialised softmax attention in fp64 on the CPU (masks as -inf, an all-masked row gives zeros; plane kernels: the values the planes hold).
Tolerances, form err <= tol * (1 + |ref|): fp32 kernels, precision 6 / 16 and planes 2e-5, precision 3 1e-4, the materialised softmax 1e-5.
Every comparison prints `STRESS <kernel> <pattern> <max err>` before it asserts (profiles/softmax_stress_tests.log: the figures of the SIMT
emulator, largest 1.9e-5 at precision 3, 1.2e-5 at precision 6 / 16, below 1.4e-6 elsewhere; not yet measured on the MI355X).
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

PATTERNS = ("asc", "desc", "late_spike", "first_spike", "two", "flat", "neg", "masked_spike")
MEASURED = {}  # (kernel, pattern) -> largest |got - ref| seen in this process
TOL = {"p3": 1e-4, "softmax_relpos": 1e-5, "softmax_rows": 1e-5}  # every other kernel: 2e-5
SCALE = 0.125


def _r(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _q8(shape, seed):
    """Seeded noise in [-1, 1], multiples of 1/8."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float() / 8


def _check(got, ref, kernel, pattern, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    e = float(torch.nan_to_num(err, nan=math.inf).max()) if err.numel() else 0.0
    MEASURED[(kernel, pattern)] = max(MEASURED.get((kernel, pattern), 0.0), e)
    tol = TOL.get(kernel, 2e-5)
    print(f"STRESS {kernel} {pattern} {e:.3e} (tol {tol:g}, {what})")
    bad = ~(err <= tol * (1.0 + ref.abs()))
    assert not bad.any(), f"{kernel} {pattern} {what}: max err {e:.3e} (ref max {float(ref.abs().max()):.3e}), {int(bad.sum())} / {bad.numel()} over tol {tol}"


def _pattern(name, n, first=0, late=None, two=None):
    """(c_j, noise-free keys) of a pattern over n valid keys."""
    c, clean = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.bool)
    if n == 0:
        return c, clean
    late = n - 1 if late is None else late
    two = (min(3, n - 1), max(n - 2, 0)) if two is None else two
    j = torch.arange(n, dtype=torch.float64)
    if name == "asc":
        c = j / 2
    elif name == "desc":
        c = -j / 2
    elif name == "late_spike":
        c[late], clean[late] = 48.0, True
    elif name == "first_spike":
        c[first], clean[first] = 48.0, True
    elif name == "two":
        for t in two:
            c[t], clean[t] = 40.0, True
    elif name == "flat":
        c[:], clean[:] = 3.0, True
    elif name == "neg":
        c[:] = -60.0
    else:
        assert name == "masked_spike", name
    return c, clean


def _exact_scores(q, k, eq, bound=2 ** 11):
    """fp64 scaled scores of einsum `eq`, asserted equal to the fp32 evaluation of the same expression (and |raw score| < bound: 2**11 wherever a split format runs)."""
    s = torch.einsum(eq, q.double(), k.double()) * SCALE
    s32 = torch.einsum(eq, q.float(), k.float()) * SCALE
    assert torch.equal(s, s32.double()), "the test's own inputs are not exact in fp32"
    assert float(s.abs().max()) / SCALE < bound
    return s


def _planes_exact(x):
    """What a planes tensor holds for fp32 x: h + l / 2048 in fp64 (tests/test_planes_gpu.py)."""
    h = x.half()
    l = ((x.double() - h.double()) * 2048.0).half()
    return h.double() + l.double() / 2048.0


def _softmax_rows_ref(s):
    return torch.nan_to_num(torch.softmax(s, -1))  # an all-masked row: zeros


# ---------------------------------------------------------------------------------------------------------------------------------------------
# prefill kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
Z, H = 2, 2
PREFILL = ("f32", "kv", "p3", "p6", "p16", "po", "planes1", "planes2", "planes3", "planes4", "planes5", "planes6")
MASKS = (None, "70", "1", "0", "causal")


def _lens(Tk, mask):
    return None if mask in (None, "causal") else [Tk, int(mask)]


def _prefill_cases(kernel):
    """(Tq, Tk, mask): T in {1, 65, 150} (64-key tiles: 150 = two tiles + 22 keys), Tq = 130 (two 128-query blocks), every mask.  `kv`: fewer queries than keys."""
    shapes = ((1, 1), (1, 65), (33, 65), (130, 150)) if kernel == "kv" else ((1, 1), (65, 65), (150, 150), (130, 130))
    out = []
    for Tq, Tk in shapes:
        for mask in MASKS:
            if mask == "70" and Tk <= 70:
                continue
            if mask == "causal" and kernel.startswith("planes") and kernel != "planes1":
                continue  # the causal plane attention is the one-group kernel whatever version is asked for
            if Tq == 130 and mask in ("1", "0"):
                continue
            out.append((Tq, Tk, mask))
    return out


def _spike_key(Tq, Tk, mask):
    """masked_spike: (batch entries, key index, first query that legitimately sees it) or None if the mask hides nothing."""
    if mask is None:
        return None
    if mask == "causal":
        j = (Tk - Tq) + Tq * 7 // 15
        return ((0, 1), j, j - (Tk - Tq)) if j - (Tk - Tq) > 0 else None
    n = int(mask)
    return ((1,), n, Tq) if n < Tk else None


@functools.lru_cache(maxsize=None)
def _prefill_inputs(pattern, Tq, Tk, mask, spike):
    lens = _lens(Tk, mask)
    q, k = torch.zeros(Z, Tq, H, 64), torch.zeros(Z, Tk, H, 64)
    q[..., :16], q[..., 16:] = 1.0, _q8((Z, Tq, H, 48), 11)
    k[..., 16:] = _q8((Z, Tk, H, 48), 12)  # keys past a length stay like this: stale but finite
    v = _r((Z, Tk, H, 64), 13)
    for z in range(Z):
        n = Tk if lens is None else min(Tk, lens[z])
        c, clean = _pattern(pattern, n)
        k[z, :n, :, :16] = (c / 2).float()[:, None, None]
        k[z, :n, :, 16:] *= (~clean).float()[:, None, None]
    if spike and pattern == "masked_spike":
        zs, j, _ = _spike_key(Tq, Tk, mask)
        for z in zs:
            k[z, j, :, :16], k[z, j, :, 16:] = 64.0, 0.0
    return q, k, v


@functools.lru_cache(maxsize=None)
def _prefill_ref(pattern, Tq, Tk, mask, spike, planes):
    q, k, v = _prefill_inputs(pattern, Tq, Tk, mask, spike)
    s = _exact_scores(q, k, "zqhd,zkhd->zhqk")
    j, i = torch.arange(Tk)[None, :], torch.arange(Tq)[:, None]
    if mask == "causal":
        s = s.masked_fill((j > i + (Tk - Tq))[None, None], -math.inf)
    elif mask is not None:
        s = s.masked_fill((j[None] >= torch.tensor(_lens(Tk, mask))[:, None, None])[:, None], -math.inf)
    return torch.einsum("zhqk,zkhd->zqhd", _softmax_rows_ref(s), _planes_exact(v) if planes else v.double())


def _run_prefill(dev, kernel, q, k, v, lens, causal):
    from chatterbox_amd import ops
    from chatterbox_amd._lib import check
    Tq, Tk = q.shape[1], k.shape[1]
    kl = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    out = torch.full((Z, Tq, H, 64), float("nan")).to(dev)
    if kernel == "f32":
        ops.flash_attn(qd, kd, vd, out, SCALE, key_lens=kl, causal=causal)
    elif kernel == "kv":  # views of a [row][head][max_ctx][64] cache with stale rows behind the keys
        ctx = Tk + 11
        kc, vc = _q8((Z, H, ctx, 64), 14).to(dev), _r((Z, H, ctx, 64), 15).to(dev)
        kc[:, :, :Tk], vc[:, :, :Tk] = kd.permute(0, 2, 1, 3), vd.permute(0, 2, 1, 3)
        ops.flash_attn(qd, kc[:, :, :Tk].permute(0, 2, 1, 3), vc[:, :, :Tk].permute(0, 2, 1, 3), out, SCALE, key_lens=kl, causal=causal)
    elif kernel in ("p3", "p6", "p16"):
        with ops.gemm_precision(int(kernel[1:])):
            ops.flash_attn(qd, kd, vd, out, SCALE, key_lens=kl, causal=causal)
    elif kernel == "po":
        outP = ops.Planes(Z * Tq, H * 64, dev, zero=True)
        check(ops.lib.cbx_flash_attn_split_po(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), outP.ptr, None if kl is None else kl.data_ptr(), Z, H, Tq, Tk, qd.stride(0),
                                              qd.stride(1), kd.stride(0), kd.stride(1), vd.stride(0), vd.stride(1), Tq * outP.ld, outP.ld, outP.lo, SCALE, int(causal),
                                              ops._stream()), "cbx_flash_attn_split_po")
        out = outP.float().view(Z, Tq, H, 64)
    else:
        assert kernel.startswith("planes") and Tq == Tk
        T, C, Tp = Tq, H * 64, (Tq + 7) // 8 * 8
        qk = ops.Planes(Z * T, 2 * C, dev, zero=True)
        ops.split_planes(qd.reshape(Z * T, C), qk.cols(0, C))
        ops.split_planes(kd.reshape(Z * T, C), qk.cols(C, C))
        vtt = torch.zeros(Z, C, Tp)
        vtt[:, :, :T] = v.reshape(Z, T, C).transpose(1, 2)
        vt = ops.Planes(Z * C, Tp, dev, zero=True)
        ops.split_planes(vtt.reshape(Z * C, Tp).to(dev), vt)
        outP = ops.Planes(Z * T, C, dev, zero=True)
        ops.flash_attn_planes(qk.cols(0, C), qk.cols(C, C), vt, outP, Z=Z, H=H, T=T, vt_sb=C * vt.ld, scale=SCALE, key_lens=kl, causal=causal, version=int(kernel[6:]))
        out = outP.float().view(Z, T, H, 64)
    return out.cpu()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kernel", PREFILL)
def test_prefill_attention_stress(dev, kernel, pattern, cases=None):
    """cbx_flash_attn_f32 / _kv_f32 / _split_f32 (3, 6, 16) / _split_po / cbx_flash_attn_planes_v (versions 1 .. 6) on prescribed scores, every shape and mask
    of _prefill_cases.  An empty utterance (key_lens 0) gives zeros: the convention all of them document (inv = l > 0 ? 1 / l : 0)."""
    for Tq, Tk, mask in (_prefill_cases(kernel) if cases is None else cases):
        hide = _spike_key(Tq, Tk, mask)
        if pattern == "masked_spike" and hide is None:
            continue
        planes = kernel.startswith("planes")
        q, k, v = _prefill_inputs(pattern, Tq, Tk, mask, True)
        out = _run_prefill(dev, kernel, q, k, v, _lens(Tk, mask), mask == "causal")
        _check(out, _prefill_ref(pattern, Tq, Tk, mask, True, planes), kernel, pattern, f"Tq {Tq} Tk {Tk} mask {mask}")
        if mask == "0":
            assert float(out[1].abs().max()) == 0.0, f"{kernel}: an utterance without keys gives zeros"
        if pattern == "masked_spike":
            q0, k0, v0 = _prefill_inputs(pattern, Tq, Tk, mask, False)
            base = _run_prefill(dev, kernel, q0, k0, v0, _lens(Tk, mask), mask == "causal")
            zs, j, i_vis = hide
            assert torch.equal(out[list(zs), :i_vis], base[list(zs), :i_vis]) and bool(torch.isfinite(base).all()), \
                f"{kernel} Tq {Tq} Tk {Tk} mask {mask}: a +128 score on hidden key {j} changed the output of queries that cannot see it"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# conformer rel-pos attention: flash form and materialised softmax
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _rel_pattern(pattern, T):
    """The pattern over the 2T - 1 relative positions r = T - 1 - i + j: spikes on the diagonals j = i (first), j = i + (T - 1) // 2 (late), j = i - 3 (two)."""
    mid = T - 1
    return _pattern(pattern, 2 * T - 1, first=mid, late=mid + (T - 1) // 2, two=(max(mid - 3, 0), mid + (T - 1) // 2))


@functools.lru_cache(maxsize=None)
def _relpos_case(pattern, T, mask, term, spike):
    """q4 (Z, T, 4, H, 64) = [q + u | q + v | k | v], pp (2T - 1, H * 64) and the fp64 result; `term`: which of the two score terms carries the pattern."""
    lens = _lens(T, mask)
    q4, pp = torch.zeros(Z, T, 4, H, 64), torch.zeros(2 * T - 1, H, 64)
    q4[:, :, 3] = _r((Z, T, H, 64), 23)
    q4[:, :, 0, :, 16:], q4[:, :, 1, :, 16:] = _q8((Z, T, H, 48), 21), _q8((Z, T, H, 48), 22)
    q4[:, :, 2, :, 16:], pp[:, :, 16:] = _q8((Z, T, H, 48), 24), _q8((2 * T - 1, H, 48), 25)
    q4[:, :, 0 if term == "content" else 1, :, :16] = 1.0
    if term == "content":
        for z in range(Z):
            n = T if lens is None else min(T, lens[z])
            c, clean = _pattern(pattern, n)
            q4[z, :n, 2, :, :16] = (c / 2).float()[:, None, None]
            q4[z, :n, 2, :, 16:] *= (~clean).float()[:, None, None]
            if bool(clean.any()):  # a noise-free key has no position noise either
                q4[z, :, 1, :, 16:] = 0.0
    else:
        c, clean = _rel_pattern(pattern, T)
        pp[:, :, :16] = (c / 2).float()[:, None, None]
        pp[:, :, 16:] *= (~clean).float()[:, None, None]
        if bool(clean.any()):
            q4[:, :, 0, :, 16:] = 0.0
    if spike and pattern == "masked_spike":  # on the key behind utterance 1's length, in the content term
        q4[1, lens[1], 2, :, :16], q4[1, :, 0, :, :16] = 64.0, 1.0
    qu, qv, k, v = (q4[:, :, i] for i in range(4))
    ac = _exact_scores(qu, k, "zqhd,zkhd->zhqk")
    bd_full = _exact_scores(qv, pp, "zqhd,rhd->zhqr")
    idx = T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]
    s = ac + torch.gather(bd_full, 3, idx.expand(Z, H, T, T))
    if lens is not None:
        s = s.masked_fill(torch.arange(T)[None, None, None, :] >= torch.tensor(lens)[:, None, None, None], -math.inf)
    return q4, pp.reshape(2 * T - 1, H * 64), torch.einsum("zhqk,zkhd->zqhd", _softmax_rows_ref(s), v.double())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("term", ["content", "position"])
def test_flash_relpos_stress(dev, term, pattern, cases=None):
    """cbx_flash_relpos_f32 with the pattern in the content term (q + u) k or in the position term (q + v) p_{T-1-i+j}; ragged lengths incl. an empty utterance."""
    from chatterbox_amd import ops
    for T, mask in (cases or [(T, m) for T in (1, 65, 150, 130) for m in MASKS[:4] if not (m == "70" and T <= 70)]):
        if pattern == "masked_spike" and (mask is None or int(mask) >= T):
            continue
        outs = []
        for spike in ((True, False) if pattern == "masked_spike" else (True,)):
            q4, pp, ref = _relpos_case(pattern, T, mask, term, spike)
            lens = _lens(T, mask)
            out = torch.full((Z, T, H, 64), float("nan")).to(dev)
            ops.flash_relpos(q4.to(dev), pp.to(dev), out, SCALE, key_lens=None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev))
            _check(out, ref, "relpos", pattern, f"{term} term, T {T} mask {mask}")
            outs.append(out.cpu())
        if mask == "0":
            assert float(outs[0][1].abs().max()) == 0.0, "flash_relpos: an utterance without keys gives zeros"
        if len(outs) == 2:
            assert torch.equal(outs[0][1], outs[1][1]), f"flash_relpos T {T} mask {mask}: a +128 score behind the utterance's length changed its output"


def _softmax_scores(pattern, Tq, Tk, lens, seed, spike=True):
    """Scaled scores C + N (Z, H, Tq, Tk) as their two exact summands: C the pattern per key (per utterance over its own length), N the noise."""
    C, N = torch.zeros(Z, H, Tq, Tk, dtype=torch.float64), _q8((Z, H, Tq, Tk), seed).double()
    where = []
    for z in range(Z):
        n = Tk if lens is None else min(Tk, lens[z])
        c, clean = _pattern(pattern, n)
        C[z, :, :, :n] = c
        N[z, :, :, :n] *= (~clean).double()
        where.append((n, torch.nonzero(clean).flatten().tolist()))
    if spike and pattern == "masked_spike":
        C[1, :, :, lens[1]] = 128.0
    return C, N, where


def _softmax_asserts(p, pattern, where, kernel):
    """The exact rows: one-hot for a single spike, 1/2 - 1/2 for two, and a flat row that sums to 1 within 1e-6."""
    for z, (n, hot) in enumerate(where):
        row = p[z, ..., :n].double()
        if pattern in ("late_spike", "first_spike", "two") and n > 0:
            w = 1.0 / len(set(hot))
            rest = row.clone()
            rest[..., hot] = 0.0
            assert bool((row[..., hot] == w).all()) and float(rest.max()) <= 2.0 ** -50, f"{kernel} {pattern}: exact weights {w} on keys {hot} of {n}"
        if pattern == "flat" and n > 0:
            assert float((row.sum(-1) - 1.0).abs().max()) <= 1e-6, f"{kernel}: a flat row sums to {row.sum(-1).flatten()[0].item()!r}"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("term", ["content", "position"])
def test_softmax_relpos_stress(dev, term, pattern):
    """cbx_softmax_relpos_f32 at T = 75 (ragged [75, 40]; masked_spike: the key behind the 40): the probabilities themselves.  The pattern sits in ac (content)
    or in the shifted bd (position); the entries of bd that no (i, j) reads hold a large finite value."""
    from chatterbox_amd import ops
    T, ld = 75, 76
    for lens in (None, [T, 40]):
        if pattern == "masked_spike" and lens is None:
            continue
        res = []
        for spike in ((True, False) if pattern == "masked_spike" else (True,)):
            C, N, where = _softmax_scores(pattern, T, T, lens, 31, spike)
            A, B = (C, N) if term == "content" else (N, C)
            ac, bd = (A / SCALE).float(), torch.full((Z, H, T, 2 * T - 1), 4096.0)
            idx = (T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]).expand(Z, H, T, T).contiguous()
            bd.scatter_(3, idx, (B / SCALE).float())
            assert torch.equal(ac.double() * SCALE, A) and torch.equal(torch.gather(bd, 3, idx).double() * SCALE, B)
            assert torch.equal(((ac + torch.gather(bd, 3, idx)) * SCALE).double(), C + N), "the test's own inputs are not exact in fp32"
            s = C + N
            if lens is not None:
                s = s.masked_fill(torch.arange(T)[None, None, None, :] >= torch.tensor(lens)[:, None, None, None], -math.inf)
            p = torch.full((Z, H, T, ld), 7.0).to(dev)
            ops.softmax_relpos(ac.to(dev), bd.to(dev), p, SCALE, key_lens=None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev))
            p = p.cpu()
            _check(p[..., :T], _softmax_rows_ref(s), "softmax_relpos", pattern, f"{term} term, lens {lens}")
            assert float(p[..., T:].abs().max()) == 0.0
            _softmax_asserts(p, pattern, where, "softmax_relpos")
            res.append(p)
        if len(res) == 2:
            assert torch.equal(res[0], res[1]), "softmax_relpos: a +128 score behind the utterance's length changed its probabilities"


@pytest.mark.parametrize("pattern", PATTERNS)
def test_softmax_rows_stress(dev, pattern):
    """The bd == NULL, Tk != Tq path of cbx_softmax_relpos_f32 (perceiver attention): 32 queries, 150 keys (three strides of a wave), ragged [150, 61]."""
    from chatterbox_amd import ops
    Tq, Tk, ld = 32, 150, 152
    for lens in (None, [Tk, 61]):
        if pattern == "masked_spike" and lens is None:
            continue
        res = []
        for spike in ((True, False) if pattern == "masked_spike" else (True,)):
            C, N, where = _softmax_scores(pattern, Tq, Tk, lens, 32, spike)
            s32 = ((C + N) / SCALE).float()
            assert torch.equal(s32.double() * SCALE, C + N), "the test's own inputs are not exact in fp32"
            s = C + N
            if lens is not None:
                s = s.masked_fill(torch.arange(Tk)[None, None, None, :] >= torch.tensor(lens)[:, None, None, None], -math.inf)
            p = torch.full((Z, H, Tq, ld), 7.0).to(dev)
            ops.softmax_rows(s32.to(dev), p, SCALE, Tk, None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev))
            p = p.cpu()
            _check(p[..., :Tk], _softmax_rows_ref(s), "softmax_rows", pattern, f"lens {lens}")
            assert float(p[..., Tk:].abs().max()) == 0.0
            _softmax_asserts(p, pattern, where, "softmax_rows")
            res.append(p)
        if len(res) == 2:
            assert torch.equal(res[0], res[1]), "softmax_rows: a +128 score behind the utterance's length changed its probabilities"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# decode kernels: one query per (row, head) over a [row][head][max_ctx][64] cache; row r has context CONTEXTS[r]
# ---------------------------------------------------------------------------------------------------------------------------------------------
CONTEXTS = (1, 17, 64, 65, 129, 513)  # around the 16 U step (64 / 128 positions), the chunk boundaries and the split threshold (512)


def _rot_inv(y):
    """x with rotate_half(x) == y: the raw row a quarter-turn RoPE table (cos 0, sin 1) turns into y."""
    return torch.cat([y[..., 32:], -y[..., :32]], -1)


@functools.lru_cache(maxsize=None)
def _decode_case(pattern, Hd, contexts, spike):
    """Caches whose rows 0 .. pos - 1 carry the pattern, the new token's q / k / v (key pos = the LAST valid key: late_spike sits on it), stale noise from pos
    on (masked_spike: +128 at pos + 1) and the fp64 result (rows, Hd, 64)."""
    rows, maxp = len(contexts), max(contexts) + 15
    kc, vc = torch.zeros(rows, Hd, maxp, 64), _r((rows, Hd, maxp, 64), 42)
    kc[..., 16:] = _q8((rows, Hd, maxp, 48), 41)
    kc[..., :16] = -2.0  # stale rows: a score of -4 + noise, finite
    q = torch.zeros(rows, Hd, 64)
    q[..., :16], q[..., 16:] = 1.0, _q8((rows, Hd, 48), 43)
    kn, vn = torch.zeros(rows, Hd, 64), _r((rows, Hd, 64), 44)
    ref = torch.zeros(rows, Hd, 64, dtype=torch.float64)
    for r, n in enumerate(contexts):
        c, clean = _pattern(pattern, n)
        K = kc[r, :, :n].clone()
        K[:, :, :16] = (c / 2).float()[None, :, None]
        K[:, :, 16:] *= (~clean).float()[None, :, None]
        kn[r], V = K[:, n - 1], torch.cat([vc[r, :, : n - 1], vn[r][:, None]], 1)
        kc[r, :, : n - 1] = K[:, : n - 1]  # position n - 1 itself keeps its stale row: the new token's key is not in the cache yet
        if spike and pattern == "masked_spike":
            kc[r, :, n, :16], kc[r, :, n, 16:] = 64.0, 0.0
        s = _exact_scores(q[r], K, "hd,hkd->hk", 2 ** 12)  # fp32 kernels only: asc reaches 256 at context 513
        ref[r] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), V.double())
    return kc, vc, q, kn, vn, ref


def _rope_tables(rope, maxp, dev):
    if rope == "none":
        return None, None
    one, zero = torch.ones(maxp, 64), torch.zeros(maxp, 64)
    return (one.to(dev), zero.to(dev)) if rope == "identity" else (zero.to(dev), one.to(dev))


def _qkv_rows(q, kn, vn, rope):
    raw = _rot_inv if rope == "quarter" else (lambda t: t)
    return torch.cat([raw(q).flatten(1), raw(kn).flatten(1), vn.flatten(1)], 1).contiguous()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Hd", [12, 16])
def test_decode_attn_stress(dev, Hd, pattern, contexts=CONTEXTS):
    """cbx_decode_attn_f32 (two-pass softmax through LDS): every key from the cache, ctx_lens = the context; masked_spike at index ctx."""
    from chatterbox_amd import ops
    outs = []
    for spike in ((True, False) if pattern == "masked_spike" else (True,)):
        kc, vc, q, kn, vn, ref = _decode_case(pattern, Hd, contexts, spike)
        kc, vc = kc.clone(), vc.clone()
        for r, n in enumerate(contexts):
            kc[r, :, n - 1], vc[r, :, n - 1] = kn[r], vn[r]
        out = torch.full((len(contexts), Hd * 64), float("nan")).to(dev)
        ops.decode_attn(q.flatten(1).to(dev), kc.to(dev), vc.to(dev), out, torch.tensor(contexts, dtype=torch.int32).to(dev), SCALE)
        _check(out.view(-1, Hd, 64), ref, "decode_attn", pattern, f"H {Hd} contexts {contexts}")
        outs.append(out.cpu())
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), "decode_attn: a +128 score at cache index ctx changed the output"


DA_VARIANTS = ((1, 4), (1, 8), (3, 4), (7, 4))  # (pipeline, unroll) against (0, unroll)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Hd,rope", [(12, "none"), (16, "identity"), (16, "quarter"), (12, "quarter")])
def test_decode_attn_rope_stress(dev, Hd, rope, pattern, contexts=CONTEXTS, variants=DA_VARIANTS, split_mins=(1, 512)):
    """cbx_decode_attn_rope: the plain form (unroll 4 / 8), the pipelined / non-temporal / speculative forms and the split-context grid with its ticket merge
    (rows * heads < 128: split_min 1 splits every row, 512 only the longest).  Against fp64; every variant equal to the plain form of the same unroll and split
    threshold bit for bit; the new token's k / v appended exactly (its cache slot held a stale row before); masked_spike at pos + 1 against the run without it."""
    from chatterbox_amd import ops
    rows = len(contexts)
    pos = torch.tensor([n - 1 for n in contexts], dtype=torch.int32)
    cases = {spike: _decode_case(pattern, Hd, contexts, spike) for spike in ((True, False) if pattern == "masked_spike" else (True,))}
    maxp = cases[True][0].shape[2]
    cos, sin = _rope_tables(rope, maxp, dev)

    def run(geom, spike):
        kc0, vc0, q, kn, vn, ref = cases[spike]
        kc, vc, out = kc0.clone().to(dev), vc0.clone().to(dev), torch.full((rows, Hd * 64), float("nan")).to(dev)
        ops.decode_attn_rope(_qkv_rows(q, kn, vn, rope).to(dev), pos.to(dev), cos, sin, kc, vc, out, SCALE, geom=geom)
        kc, vc = kc.cpu(), vc.cpu()
        for r, n in enumerate(contexts):
            assert torch.equal(kc[r, :, n - 1], kn[r]) and torch.equal(vc[r, :, n - 1], vn[r]), f"row {r}: the new token's k / v in the cache"
            kc[r, :, n - 1], vc[r, :, n - 1] = kc0[r, :, n - 1], vc0[r, :, n - 1]
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0), "exactly one cache row written per (row, head)"
        return out.cpu()

    for split_min in split_mins:
        plain = {}
        for u in sorted({u for _, u in variants} | {4}):
            plain[u] = run(ops.DecodeAttnGeom(dev, unroll=u, pipeline=0, split_min=split_min), True)
            _check(plain[u].view(rows, Hd, 64), cases[True][5], "decode_rope" if split_min > 1 else "decode_rope_split", pattern,
                   f"plain, unroll {u}, split_min {split_min}, H {Hd}, rope {rope}")
            if pattern == "masked_spike":
                assert torch.equal(plain[u], run(ops.DecodeAttnGeom(dev, unroll=u, pipeline=0, split_min=split_min), False)), \
                    f"plain, unroll {u}, split_min {split_min}: a +128 score at pos + 1 of the stale cache changed the output"
        for pipe, u in variants:
            got = run(ops.DecodeAttnGeom(dev, unroll=u, pipeline=pipe, split_min=split_min), True)
            assert torch.equal(got, plain[u]), f"pipeline {pipe}, unroll {u}, split_min {split_min}: differs from the plain form by {float((got - plain[u]).abs().max()):.3e}"
            if pattern == "masked_spike":
                assert torch.equal(got, run(ops.DecodeAttnGeom(dev, unroll=u, pipeline=pipe, split_min=split_min), False)), \
                    f"pipeline {pipe}, unroll {u}, split_min {split_min}: a +128 score at pos + 1 of the stale cache changed the output"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Hd,rope,chunks,S", [(12, "none", 2, 3), (16, "quarter", 4, 8), (16, "identity", 8, 2), (12, "quarter", 4, 16)])
def test_decode_attn_parts_stress(dev, Hd, rope, chunks, S, pattern, contexts=CONTEXTS):
    """cbx_decode_attn_parts (S slices x `chunks` chunks of 16 positions in flight; contexts that need a second batch of chunks, slices that stay empty) followed
    by the attention-merge prologue of cbx_gemv_row_f32 on an identity weight, which returns the merged attention row exactly (<= 4 rows per launch)."""
    from chatterbox_amd import ops
    rows, Kd = len(contexts), Hd * 64
    pos = torch.tensor([n - 1 for n in contexts], dtype=torch.int32)
    eye = torch.eye(Kd).to(dev)
    outs = []
    for spike in ((True, False) if pattern == "masked_spike" else (True,)):
        kc0, vc0, q, kn, vn, ref = _decode_case(pattern, Hd, contexts, spike)
        cos, sin = _rope_tables(rope, kc0.shape[2], dev)
        kc, vc = kc0.clone().to(dev), vc0.clone().to(dev)
        parts = torch.full((rows, Hd, S, ops.ATTN_PART_REC), float("nan")).to(dev)
        ops.decode_attn_parts(_qkv_rows(q, kn, vn, rope).to(dev), pos.to(dev), kc, vc, parts, SCALE, cos_t=cos, sin_t=sin, chunks=chunks)
        out = torch.full((rows, Kd), float("nan")).to(dev)
        for r0 in range(0, rows, 4):
            ops.gemv_row(None, eye, out[r0:r0 + 4], parts=parts[r0:r0 + 4])
        _check(out.view(rows, Hd, 64), ref, "decode_parts", pattern, f"H {Hd} rope {rope} chunks {chunks} slices {S}")
        kc, vc = kc.cpu(), vc.cpu()
        for r, n in enumerate(contexts):
            assert torch.equal(kc[r, :, n - 1], kn[r]) and torch.equal(vc[r, :, n - 1], vn[r]), f"row {r}: the new token's k / v in the cache"
        outs.append(out.cpu())
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), "decode_attn_parts + merge: a +128 score at pos + 1 of the stale cache changed the output"
