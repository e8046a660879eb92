"""Thin Python wrappers that hand raw device pointers of torch tensors + the current HIP stream to the C ABI.

torch is used only as the allocator / stream provider; every function below launches hand-written gfx950 kernels
from libcbx_hip.so and raises if the library is unavailable (no eager fallback).
"""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import (ATTN_PART_REC, ATTN_PL_CORESIDENT, GEMV_DEEP, GEMV_PRE_EPI, GEMV_SHALLOW, PL_TILE_CORESIDENT, AttnPartsParams, DecodeAttnParams, GemmParams,
                   GemmPlParams, GemvParams, GemvRowParams, PrefillEmbed, SamplerParams, check, lib)

NONE, SILU, GELU_ERF, GELU_TANH, MISH, LRELU, ELU, TANH, SNAKE, ABS = range(10)


class KernelTimer:
    """HIP-event timing of individual launches of selected kernel classes, on the stream they are launched on.
    Used by bench.py for the roofline line (average launch duration + algorithmic FLOPs/bytes per launch)."""

    def __init__(self, kinds):
        self.kinds = set(kinds)
        self.rec = []  # (kind, start_event, end_event, flops, bytes)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, e0, e1, fl, by in self.rec:
            d = out.setdefault(kind, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


TIMER = None  # set to a KernelTimer to time launches (never during hipGraph capture)


def _timed(kind, flops, nbytes, fn):
    if TIMER is None or kind not in TIMER.kinds:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    TIMER.rec.append((kind, e0, e1, float(flops), float(nbytes)))
    return r


def on_device(fn):
    """Method decorator for the engines: run the body with `self.dev` as the current HIP device, so that every launch (which goes
    to torch's CURRENT stream of the CURRENT device, see _stream()) lands on the GPU the engine's tensors live on -- the drop-in
    API accepts any device string (e.g. 'cuda:1' in a process whose current device is 0)."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        dev = getattr(self, "dev", None)
        if dev is None:  # decorating __init__(self, state_dict, device="cuda", ...): the device is the 2nd argument
            dev = k.get("device", a[1] if len(a) > 1 else "cuda")
        dev = dev if isinstance(dev, torch.device) else torch.device(dev)
        if dev.type != "cuda" or dev.index is None or dev.index == torch.cuda.current_device():
            return fn(self, *a, **k)
        with torch.cuda.device(dev):
            return fn(self, *a, **k)
    return wrapper


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t, name):
    assert t.dtype == torch.float32 and t.is_cuda, f"{name}: expected a CUDA fp32 tensor, got {t.dtype} on {t.device}"
    return t


# cbx_gemm_t.precision of every gemm()/linear()/conv1d() issued inside `with gemm_precision(p)`: 0 default, 1 exact, 3 / 6 split-bf16, 16 split-fp16.
# PER HOST THREAD (round 5): synthesize_pipelined enqueues T3 (exact) on one thread while the flow + vocoder (16) are enqueued on another; a module
# global would let the flow's scope leak into T3's conditioning / head GEMMs.  `ops.GEMM_PRECISION` reads the calling thread's value (module __getattr__).
import threading as _threading

_TLS = _threading.local()


def _prec():
    return getattr(_TLS, "prec", 0)


def __getattr__(name):
    if name == "GEMM_PRECISION":
        return _prec()
    raise AttributeError(name)


GEMM_DIAG = 0  # cbx_gemm_t.reserved0: only read by a -DCBX_DIAG build of gemm_split.hip (scripts/diag_gemm.sh)


class gemm_precision:
    """`with ops.gemm_precision(6): ...` -- the engines scope their numerics policy this way (T3 stays exact: sampled
    tokens must match the reference bit for bit; the CFM / vocoder run the fp32-accurate split-bf16 kernels)."""

    def __init__(self, precision):
        self.precision = int(precision)

    def __enter__(self):
        self._prev, _TLS.prec = _prec(), self.precision

    def __exit__(self, *exc):
        _TLS.prec = self._prev


LN_FUSION = os.environ.get("CBX_LN_FUSION", "1") != "0"  # CFM transformer blocks: LayerNorm folded into the consuming Linear
_RANGE_FLAGS = {}  # device index -> int32 device word (one per GPU: an engine per GPU may live in one process, see on_device())


def _dev_index(device=None):
    d = torch.device("cuda" if device is None else device)
    return torch.cuda.current_device() if d.index is None else d.index


def enable_range_flag(device=None):
    """Allocate (once per GPU) the device words the f16x3 kernels (precision 16) raise when an operand exceeds the fp16 range.  The library
    keeps one pointer per device ordinal (cbx_set_range_flag registers it for the CURRENT device; a launch looks its own device's word up),
    so engines on different GPUs of one process never OR into a foreign-device pointer.  Two words per GPU: select_range_flag() switches the
    registered one between batches whose launches are in flight at once (the launch carries the pointer that was registered when it was ENQUEUED)."""
    idx = _dev_index(device)
    if idx not in _RANGE_FLAGS:
        with torch.cuda.device(idx):
            _RANGE_FLAGS[idx] = [torch.zeros(2, dtype=torch.int32, device=torch.device("cuda", idx)), 0]
            check(lib.cbx_set_range_flag(_p(_RANGE_FLAGS[idx][0])), "cbx_set_range_flag")
    words, which = _RANGE_FLAGS[idx]
    return words[which: which + 1]


def select_range_flag(device, which):
    """Every precision-16 launch ENQUEUED from now on reports into word `which` (0 / 1) of this GPU: engine.synthesize_pipelined gives consecutive batches
    alternating words, so a trip is attributed to the batch that raised it although the vocoder of one batch runs beside the flow of the next."""
    enable_range_flag(device)
    idx = _dev_index(device)
    words = _RANGE_FLAGS[idx][0]
    _RANGE_FLAGS[idx][1] = int(which)
    if words.is_cuda:
        with torch.cuda.device(idx):  # (the registration is for the CURRENT device)
            check(lib.cbx_set_range_flag(words.data_ptr() + 4 * int(which)), "cbx_set_range_flag")
    else:  # the SIMT emulator's host words (tests/simt/harness.py)
        check(lib.cbx_set_range_flag(words.data_ptr() + 4 * int(which)), "cbx_set_range_flag")


def range_flag_tripped(device=None, which=None):
    """True when a precision-16 launch on this GPU since the last call saw an operand outside the fp16 range (synchronises; clears the flag).
    `which`: the word to look at (default: the one currently registered)."""
    ent = _RANGE_FLAGS.get(_dev_index(device))
    if ent is None:
        return False
    words, cur = ent
    w = cur if which is None else int(which)
    flag = words[w: w + 1]
    hit = bool(flag.item())
    if hit:
        flag.zero_()
    return hit


def gemm(A, W, C, *, M, N, K, lda, ldw, ldc, bias=None, R=None, ldr=0, C2=None, ldc2=0, act1=NONE, act2=NONE,
         act1_param=None, act2_param=None, act1_slope=0.0, act2_slope=0.0, alpha=1.0, beta=0.0, lens=None, Cin=0, taps=1,
         dil=1, stride=1, pad_left=0, up=1, Tin=0, nz1=1, nz2=1, a_s=(0, 0), w_s=(0, 0), c_s=(0, 0), r_s=(0, 0),
         c2_s=(0, 0), w_kn=False, swiglu=False, ln=None):
    """Raw access to cbx_gemm_f32 (see include/cbx.h).  A/W/C... are tensors (their data_ptr() is the base)."""
    p = GemmParams()
    p.A, p.W, p.C = _p(_f32(A, "A")), _p(_f32(W, "W")), _p(_f32(C, "C"))
    p.bias, p.R, p.C2 = _p(bias), _p(R), _p(C2)
    p.act1_param, p.act2_param, p.lens = _p(act1_param), _p(act2_param), _p(lens)
    if lens is not None:
        assert lens.dtype == torch.int32
    p.M, p.N, p.K = M, N, K
    p.Cin, p.taps, p.dil, p.stride, p.pad_left, p.up, p.Tin = Cin or (K // taps), taps, dil, stride, pad_left, up, Tin
    p.nz1, p.nz2, p.w_kn, p.swiglu = nz1, nz2, int(w_kn), int(swiglu)
    p.act1, p.act2, p.act1_slope, p.act2_slope, p.alpha, p.beta = act1, act2, act1_slope, act2_slope, alpha, beta
    p.lda, p.a_s1, p.a_s2 = lda, a_s[0], a_s[1]
    p.ldw, p.w_s1, p.w_s2 = ldw, w_s[0], w_s[1]
    p.ldc, p.c_s1, p.c_s2 = ldc, c_s[0], c_s[1]
    p.ldr, p.r_s1, p.r_s2 = ldr, r_s[0], r_s[1]
    p.ldc2, p.c2_s1, p.c2_s2 = ldc2, c2_s[0], c2_s[1]
    p.precision = _prec()
    p.reserved0 = GEMM_DIAG
    if ln is not None:  # (stats (M, 2), ln_w (K,), ln_b (K,)): LayerNorm folded into the A operand (ln_fusable())
        p.ln_stats, p.ln_w, p.ln_b = _p(_f32(ln[0], "ln stats")), _p(_f32(ln[1], "ln_w")), _p(_f32(ln[2], "ln_b"))
    nz = nz1 * nz2
    split = _prec() in (3, 6, 16) and M > 32 and not w_kn and not swiglu and (taps == 1 or (Cin or K // taps) % 32 == 0)
    kind = "gemm_f32_skinny" if M <= 32 else ("gemm_split" if split else "gemm_f32")  # mirrors the dispatch in gemm_f32.hip
    _timed(kind, 2.0 * M * N * K * nz, 4.0 * nz * (M * K / max(1, taps) + N * K + M * N),
           lambda: check(lib.cbx_gemm_f32(ctypes.byref(p), _stream()), "cbx_gemm_f32"))
    return C


def ln_fusable(M, K, lda=None):
    """Can `linear(..., ln=...)` fold a LayerNorm over K into its A operand here?  (the f16x3 split kernel on its Linear loader, C = 256
    statistics kernel: the CFM transformer blocks).  The library is asked (cbx_gemm_ln_fusable mirrors the dispatcher's own conditions:
    no forced tile / generic-loader knob, 31-bit byte offsets), so a tuning knob or a > 2 GiB activation falls back to layernorm + linear
    instead of raising."""
    if not (_prec() == 16 and K == 256 and M > 32 and LN_FUSION):
        return False
    return bool(lib.cbx_gemm_ln_fusable(int(M), int(K), int(K if lda is None else lda)))


def row_stats(x, stats, eps=1e-5):
    """stats[r] = (mean, rstd) of row r of x (rows, 256), as layernorm() computes them."""
    rows, C = x.shape
    assert x.stride(1) == 1 and stats.is_contiguous() and stats.shape == (rows, 2)
    check(lib.cbx_row_stats_f32(_p(_f32(x, "x")), _p(_f32(stats, "stats")), rows, C, x.stride(0), eps, _stream()), "cbx_row_stats_f32")
    return stats


def linear(x, w, out, bias=None, act=NONE, residual=None, out2=None, act2=NONE, act_param=None, act2_param=None,
           act_slope=0.0, act2_slope=0.0, alpha=1.0, beta=0.0, swiglu=False, ln=None):
    """out[M,N] = epilogue(x[M,K] @ w[N,K]^T).  x/out/residual are 2-D views with unit inner stride.
    ln = (stats, ln_w, ln_b): x is LayerNorm'ed on the way in (row_stats() + ln_fusable())."""
    M, K = x.shape
    N = w.shape[0]
    assert x.stride(1) == 1 and out.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K
    return gemm(x, w, out, M=M, N=N, K=K, lda=x.stride(0), ldw=w.stride(0), ldc=out.stride(0), bias=bias, R=residual,
                ldr=0 if residual is None else residual.stride(0), C2=out2, ldc2=0 if out2 is None else out2.stride(0),
                act1=act, act2=act2, act1_param=act_param, act2_param=act2_param, act1_slope=act_slope,
                act2_slope=act2_slope, alpha=alpha, beta=beta, swiglu=swiglu, ln=ln)


def conv1d(x, w, out, *, taps, cin, bias=None, dil=1, stride=1, pad_left=0, up=1, lens=None, act=NONE, residual=None,
           out2=None, act2=NONE, act_param=None, act2_param=None, act_slope=0.0, act2_slope=0.0, alpha=1.0, beta=0.0,
           t_in=None):
    """Channel-last conv1d as implicit GEMM.  x (B,Tin,>=cin), w packed (N, taps*cin), out (B,Tout,N)."""
    B, Tin = x.shape[0], (t_in if t_in is not None else x.shape[1])
    Tout, N = out.shape[1], w.shape[0]
    assert x.stride(2) == 1 and out.stride(2) == 1 and w.shape[1] == taps * cin
    return gemm(x, w, out, M=Tout, N=N, K=taps * cin, Cin=cin, taps=taps, dil=dil, stride=stride, pad_left=pad_left, up=up,
                Tin=Tin, lens=lens, lda=x.stride(1), ldw=w.stride(0), ldc=out.stride(1), nz1=B, a_s=(x.stride(0), 0),
                c_s=(out.stride(0), 0), bias=bias, R=residual, ldr=0 if residual is None else residual.stride(1),
                r_s=(0 if residual is None else residual.stride(0), 0), C2=out2,
                ldc2=0 if out2 is None else out2.stride(1), c2_s=(0 if out2 is None else out2.stride(0), 0), act1=act,
                act2=act2, act1_param=act_param, act2_param=act2_param, act1_slope=act_slope, act2_slope=act2_slope,
                alpha=alpha, beta=beta)


# ----------------------------------------------------------------------------- plane-format operands (ABI v7, gemm_planes.hip)

class Planes:
    """An fp32 tensor (rows, C) stored as two fp16 planes x = h + l / 2048, row by row: `t` (rows, 2 * C) fp16 = [h | l].  `cols(c0, n)`
    is the operand made of n columns from c0 on (a pointer offset: row stride and plane offset stay those of the whole tensor)."""

    def __init__(self, rows, C, device, zero=False, t=None, c0=0, width=None):
        self.t = t if t is not None else (torch.zeros if zero else torch.empty)(rows, 2 * C, dtype=torch.float16, device=device)
        assert self.t.dtype == torch.float16 and self.t.is_cuda and self.t.stride(1) == 1
        self.rows, self.Call, self.c0 = self.t.shape[0], self.t.shape[1] // 2, c0
        self.C = self.Call - c0 if width is None else width

    def cols(self, c0, n):
        assert 0 <= c0 and c0 + n <= self.C
        return Planes(0, 0, None, t=self.t, c0=self.c0 + c0, width=n)

    def rows_view(self, r0, n):
        return Planes(0, 0, None, t=self.t[r0:r0 + n], c0=self.c0, width=self.C)

    @property
    def ptr(self):
        return self.t.data_ptr() + 2 * self.c0

    @property
    def ld(self):
        return self.t.stride(0)

    @property
    def lo(self):
        return self.Call

    def float(self):
        """Back to fp32 (tests): h + l / 2048."""
        h = self.t[:, self.c0:self.c0 + self.C].float()
        return h + self.t[:, self.Call + self.c0:self.Call + self.c0 + self.C].float() / 2048.0


def split_planes(x, out=None):
    """x (rows, C) fp32 (unit inner stride, C % 4 == 0) -> Planes; `out` may be a column range of a wider Planes."""
    rows, C = x.shape
    assert x.stride(1) == 1
    out = out if out is not None else Planes(rows, C, x.device)
    assert out.C == C
    check(lib.cbx_split_planes_f32(_p(_f32(x, "x")), out.ptr, rows, C, x.stride(0), out.ld, out.lo, _stream()), "cbx_split_planes_f32")
    return out


def layernorm_planes(x, w, b, out, eps=1e-5, act=NONE, post_add=None, scale=1.0):
    """LayerNorm (C = 256) (+ activation + per-channel post_add) of fp32 rows, written in plane format."""
    rows, C = x.shape
    assert x.stride(1) == 1 and out.C == C
    check(lib.cbx_layernorm_planes_f32(_p(_f32(x, "x")), out.ptr, _p(w), _p(b), _p(post_add), rows, C, x.stride(0), out.ld, out.lo, eps, act,
                                       scale, _stream()), "cbx_layernorm_planes_f32")
    return out


# launch geometry of the plane-format kernels issued inside `with planes_geometry(tile, attn_version)` (cbx_gemm_pl_t.tile / the version argument of
# cbx_flash_attn_planes_v: per-call descriptor fields since ABI v13, nothing process-wide); (0, 0) = the library's measured defaults
def _planes_geom():
    """(tile form, attention version) of the calling HOST THREAD's planes_geometry scope -- thread-local like the GEMM precision (a plane
    GEMM issued by another thread while the flow thread sits inside a scope must not pick the scope's forms up)."""
    return getattr(_TLS, "planes_geom", (0, 0))



class planes_geometry:
    def __init__(self, tile=0, attn_version=0):
        self.new = [int(tile), int(attn_version)]

    def __enter__(self):
        self.old = _planes_geom()
        _TLS.planes_geom = tuple(self.new)

    def __exit__(self, *a):
        _TLS.planes_geom = self.old


def gemm_planes(A, W, *, M, N, K, C=None, P=None, bias=None, R=None, act=NONE, act_slope=0.0, alpha=1.0, lens=None, Cin=0, taps=1, dil=1,
                stride=1, pad_left=0, Tin=0, nz1=1, a_s1=0, w_s1=0, ldc=0, c_s1=0, ldr=0, r_s1=0, p_s1=0, PT=None, pt_n0=0, pt_T=0, pt_zs=0, tile=None,
                ln=None, lnp=None, lnp_s1=0, ln_eps=1e-5):
    """Raw access to cbx_gemm_planes (include/cbx.h): A, W, P are Planes operands, C / R fp32 tensors (their data_ptr() is the base).
    PT (Planes over (groups * (N - pt_n0), >= pt_T) rows): output columns n >= pt_n0 are written TRANSPOSED per group of pt_T rows.
    ln = (w, b) + lnp (Planes, N == 256): the epilogue also writes LayerNorm(C row) * w + b to lnp (ABI v13: replaces a layernorm_planes launch)."""
    p = GemmPlParams()
    p.A, p.W, p.C, p.P = A.ptr, W.ptr, _p(C), None if P is None else P.ptr
    p.bias, p.R, p.lens = _p(bias), _p(R), _p(lens)
    if lens is not None:
        assert lens.dtype == torch.int32
    p.M, p.N, p.K = M, N, K
    p.Cin, p.taps, p.dil, p.stride, p.pad_left, p.Tin, p.nz1 = Cin or (K // taps), taps, dil, stride, pad_left, Tin, nz1
    p.act, p.act_slope, p.alpha = act, act_slope, alpha
    p.lda, p.a_lo, p.a_s1 = A.ld, A.lo, a_s1
    p.ldw, p.w_lo, p.w_s1 = W.ld, W.lo, w_s1
    p.ldc, p.c_s1, p.ldr, p.r_s1 = ldc, c_s1, ldr, r_s1
    if P is not None:
        p.ldp, p.p_lo, p.p_s1 = P.ld, P.lo, p_s1
    p.reserved0 = GEMM_DIAG
    p.tile = _planes_geom()[0] if tile is None else int(tile)
    if ln is not None:
        assert lnp is not None and N == 256
        p.ln_w, p.ln_b, p.LNP, p.ld_lnp, p.lnp_lo, p.lnp_s1, p.ln_eps = _p(_f32(ln[0], "ln_w")), _p(ln[1]), lnp.ptr, lnp.ld, lnp.lo, lnp_s1, ln_eps
    if PT is not None:
        p.PT, p.pt_n0, p.pt_T, p.pt_ld, p.pt_lo, p.pt_zs = PT.ptr, pt_n0, pt_T, PT.ld, PT.lo, pt_zs
    _timed("gemm_planes", 2.0 * M * N * K * nz1, 4.0 * nz1 * (M * K / max(1, taps) + N * K + M * N),
           lambda: check(lib.cbx_gemm_planes(ctypes.byref(p), _stream()), "cbx_gemm_planes"))


def linear_planes(x, w, *, out=None, outp=None, bias=None, act=NONE, residual=None, act_slope=0.0, ln=None, lnp=None):
    """epilogue(x @ w^T) for Planes x (M, K), w (N, K): fp32 `out` (M, N) and / or Planes `outp`; residual fp32 (may alias out).
    ln = (w, b), lnp (Planes (M, 256)): LayerNorm of the finished row to lnp as well (N == 256)."""
    M, K, N = x.rows, x.C, w.rows
    assert w.C == K and (out is not None or outp is not None)
    gemm_planes(x, w, M=M, N=N, K=K, C=out, P=outp, bias=bias, R=residual, act=act, act_slope=act_slope,
                ldc=0 if out is None else out.stride(0), ldr=0 if residual is None else residual.stride(0), ln=ln, lnp=lnp)


def conv1d_planes(x, w, *, B, T, taps, cin, out=None, outp=None, bias=None, pad_left=0, lens=None, act=NONE, residual=None):
    """Channel-last causal Conv1d as implicit GEMM on plane operands: x Planes over (B * T, cin) rows, w Planes (N, taps * cin);
    fp32 out (B, T, N) and / or Planes outp over (B * T, N)."""
    N = w.rows
    assert w.C == taps * cin and x.C >= cin
    gemm_planes(x, w, M=T, N=N, K=taps * cin, Cin=cin, taps=taps, pad_left=pad_left, Tin=T, lens=lens, nz1=B, a_s1=T * x.ld,
                C=out, P=outp, bias=bias, R=residual, act=act, ldc=0 if out is None else out.stride(1), c_s1=0 if out is None else out.stride(0),
                ldr=0 if residual is None else residual.stride(1), r_s1=0 if residual is None else residual.stride(0),
                p_s1=0 if outp is None else T * outp.ld)


def flash_attn_planes(q, k, vt, out, *, Z, H, T, vt_sb, scale, key_lens=None, causal=False, version=None):
    """q, k: Planes column ranges (Z * T rows, H * 64 columns); vt: Planes over (Z * H * 64 rows, >= T rounded up to 8 columns) = V^T
    (batch stride vt_sb halves); out: Planes (Z * T rows, H * 64)."""
    args = (q.ptr, k.ptr, vt.ptr, out.ptr, _p(key_lens), Z, H, T, T, T * q.ld, q.ld, q.lo, T * k.ld, k.ld, k.lo, vt_sb, vt.ld, vt.lo,
            T * out.ld, out.ld, out.lo, scale, int(causal))
    _timed("flash_attn_planes", 4.0 * Z * H * T * T * 64 * (0.5 if causal else 1.0), 4.0 * Z * H * 64 * 4 * T,
           lambda: check(lib.cbx_flash_attn_planes_v(*args, _planes_geom()[1] if version is None else int(version), _stream()), "cbx_flash_attn_planes_v"))
    return out


def bmm(a, b, out, *, nn=False, alpha=1.0):
    """Two-level batched matmul on 4-D strided views (Z1, Z2, M, K):  out = a @ b^T (b: Z1,Z2,N,K) or, with nn=True,
    out = a @ b (b: Z1,Z2,K,N)."""
    Z1, Z2, M, K = a.shape
    N = b.shape[3] if nn else b.shape[2]
    assert a.stride(3) == 1 and b.stride(3) == 1 and out.stride(3) == 1
    return gemm(a, b, out, M=M, N=N, K=K, lda=a.stride(2), ldw=b.stride(2), ldc=out.stride(2), nz1=Z1, nz2=Z2,
                a_s=(a.stride(0), a.stride(1)), w_s=(b.stride(0), b.stride(1)), c_s=(out.stride(0), out.stride(1)),
                w_kn=nn, alpha=alpha)


def _tile_rows(half_tile):
    """gemv / pack_gemv_weight `half_tile`: False -> 16-column tiles, True -> 8, or the tile width itself (8, 12, 4)."""
    tr = 0 if not half_tile else (8 if half_tile is True or half_tile == 1 else int(half_tile))
    assert tr in (0, 4, 8, 12), f"narrow gemv tiles are 4, 8 or 12 columns wide, got {half_tile!r}"
    return tr


def pack_gemv_weight(w, swiglu=False, half_tile=False, bf16=False):
    """(N, K) fp32 weight [swiglu: (2F, K) = gate rows then up rows] -> lane-ordered packed image of cbx_gemv_f32 (w_packed = 1):
    (ceil(N/16)*16, K) floats [swiglu: (2*ceil(F/16)*16, K)].  half_tile (True = 8, or 12 / 4): the narrow-tile image of the same weight.
    Done once at load (weights are constants)."""
    w = _f32(w, "w").contiguous()
    R, K = w.shape
    N = R // 2 if swiglu else R
    tr = _tile_rows(half_tile)
    assert not (tr and swiglu)
    rows = (N + tr - 1) // tr * tr if tr else (N + 15) // 16 * 16 * (2 if swiglu else 1)
    if bf16:  # opt-in decode numerics: weights rounded to bf16 (cbx_gemv_t.w_bf16), half the streamed bytes
        out = torch.empty(rows, K, dtype=torch.bfloat16, device=w.device)
        check(lib.cbx_pack_gemv_weight_bf16(_p(w), _p(out), N, K, w.stride(0), tr or int(swiglu), _stream()), "cbx_pack_gemv_weight_bf16")
        return out
    out = torch.empty(rows, K, device=w.device)
    check(lib.cbx_pack_gemv_weight_f32(_p(w), _p(out), N, K, w.stride(0), tr or int(swiglu), _stream()), "cbx_pack_gemv_weight_f32")
    return out


def gemv(x, w, out, *, N=None, bias=None, ksplit=1, nw=4, swiglu=False, act=NONE, w_packed=False, x_packed=False, M=None, K=None,
         norm_w=None, eps=1e-5, res=None, out_packed=False, xpart=None, x_out=None, ln_cw=None, ln_cb=None, half_tile=False, flags=0,
         col_tiles=0, ssq_out=None):
    """Decode GEMM: x (M<=64, K), w (N, K) [swiglu: packed (2N, K)], out (M, N) or, for ksplit > 1, (ksplit, M, N) partials.
    w_packed: w is a pack_gemv_weight() image (pass N); x_packed: x is in the same lane-ordered layout (pass M, K);
    norm_w: RMSNorm(x) folded in (packed operands only); res: residual added in the epilogue (same layout as out, may alias it);
    out_packed: out is written in the packed operand layout of the next gemv (ksplit > 1: out (ksplit, rows16, N) partial images);
    half_tile (True = 8, or 12 / 4): output columns per workgroup, w being the pack_gemv_weight image of that tile width;
    xpart (2 or 4, rows16, K): split-K partial images summed into the x operand on the fly, x_out receives x + sum(xpart);
    flags: cbx_gemv_t.flags (GEMV_PRE_EPI | GEMV_DEEP: per-launch geometry bits, results unchanged);
    col_tiles (1 .. 4, RMSNorm-folded packed fp32 form): a workgroup owns that many 16-column tiles sharing every x register and 1 / ksplit of K;
    ksplit > 1 then leaves UN-normalised partial sums out (ksplit, M, N) + ssq_out (ksplit, 16) for the consumer (decode_attn_rope(qkv_parts=...))."""
    p, M, N, K = _gemv_params(x, w, out, N=N, bias=bias, ksplit=ksplit, nw=nw, swiglu=swiglu, act=act, w_packed=w_packed, x_packed=x_packed, M=M, K=K,
                              norm_w=norm_w, eps=eps, res=res, out_packed=out_packed, xpart=xpart, x_out=x_out, ln_cw=ln_cw, ln_cb=ln_cb,
                              half_tile=half_tile, flags=flags, col_tiles=col_tiles, ssq_out=ssq_out)
    _timed("gemv_f32", 2.0 * M * N * K * (2 if swiglu else 1), 4.0 * N * K * (2 if swiglu else 1),
           lambda: check(lib.cbx_gemv_f32(ctypes.byref(p), _stream()), "cbx_gemv_f32"))
    return out


def _gemv_params(x, w, out, *, N=None, bias=None, ksplit=1, nw=4, swiglu=False, act=NONE, w_packed=False, x_packed=False, M=None, K=None,
                 norm_w=None, eps=1e-5, res=None, out_packed=False, xpart=None, x_out=None, ln_cw=None, ln_cb=None, half_tile=False, flags=0,
                 col_tiles=0, ssq_out=None):
    """The cbx_gemv_t descriptor of a gemv() call: (descriptor, M, N, K)."""
    if x_packed:
        assert w_packed and M is not None and K is not None
    else:
        M, K = x.shape
    N = N or (w.shape[0] // 2 if swiglu else w.shape[0])
    p = GemvParams()
    w_bf16 = w.dtype == torch.bfloat16
    assert not w_bf16 or (w_packed and x_packed), "bf16 weights are a packed-operand feature"
    p.x, p.W, p.bias, p.out = _p(_f32(x, "x")), _p(w if w_bf16 else _f32(w, "w")), _p(bias), _p(_f32(out, "out"))
    p.M, p.N, p.K, p.ksplit, p.nw, p.swiglu, p.act = M, N, K, ksplit, nw, int(swiglu), act
    p.ldx, p.ldw = x.stride(0), w.stride(0)
    p.w_packed, p.x_packed, p.half_tile, p.w_bf16 = int(w_packed), int(x_packed), _tile_rows(half_tile), int(w_bf16)
    p.out_packed, p.norm_w, p.res, p.eps = int(out_packed), _p(norm_w), _p(res), eps
    p.ln_cw, p.ln_cb = _p(ln_cw), _p(ln_cb)  # LayerNorm form (GPT-2): see cbx_gemv_t
    p.flags = int(flags)
    p.col_tiles, p.ssq_out = int(col_tiles), _p(ssq_out)
    if xpart is not None:
        p.n_xpart, p.xpart, p.xpart_stride, p.x_out = xpart.shape[0], _p(_f32(xpart, "xpart")), xpart.stride(0), _p(x_out)
    if ksplit > 1:
        assert out.dim() == 3 and out.shape[0] == ksplit
        p.ldo, p.part_stride = out.stride(1), out.stride(0)
    else:
        p.ldo, p.part_stride = out.stride(0), 0
    return p, M, N, K


def add_rmsnorm(x, part, w, h, eps=1e-5, bias=None, rms=True):
    """x += sum_k part[k]; h = rmsnorm(x) * w  (rms=False: LayerNorm with bias).   part (ksplit, rows, C) or None."""
    rows, C = x.shape
    ks = 0 if part is None else part.shape[0]
    check(lib.cbx_add_norm_f32(_p(x), _p(part), ks, 0 if part is None else part.stride(0), 0 if part is None else part.stride(1),
                               _p(w), _p(bias), _p(h), rows, C, x.stride(0), h.stride(0), eps, int(rms), _stream()), "cbx_add_norm_f32")
    return h


def layernorm(x, w, b, out, eps=1e-5, rms=False, act=NONE, post_add=None, scale=1.0):
    rows, C = x.shape
    assert x.stride(1) == 1 and out.stride(1) == 1
    check(lib.cbx_layernorm_f32(_p(x), _p(out), _p(w), _p(b), _p(post_add), rows, C, x.stride(0), out.stride(0), eps,
                                int(rms), act, scale, _stream()), "cbx_layernorm_f32")
    return out


def flash_attn(q, k, v, out, scale, key_lens=None, causal=False):
    """q (Z,Tq,H,64), k/v (Z,Tk,H,64), out (Z,Tq,H,64): strided views with head stride 64, unit inner stride.  k / v may carry another head stride (ABI v15:
    views of the KV cache, exact fp32 only)."""
    Z, Tq, H, D = q.shape
    Tk = k.shape[1]
    assert D == 64
    for t in (q, out):
        assert t.stride(3) == 1 and t.stride(2) == 64
    assert k.stride(3) == 1 and v.stride(3) == 1
    if k.stride(2) != 64 or v.stride(2) != 64:
        assert _prec() not in (3, 6, 16), "K / V head strides: the exact fp32 attention only"
        kv_args = (_p(q), _p(k), _p(v), _p(out), _p(key_lens), Z, H, Tq, Tk, q.stride(0), q.stride(1), k.stride(0), k.stride(1), k.stride(2),
                   v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1), scale, int(causal))
        _timed("flash_attn_f32", 4.0 * Z * H * Tq * Tk * 64 * (0.5 if causal else 1.0), 4.0 * Z * H * 64 * (2 * Tq + 2 * Tk),
               lambda: check(lib.cbx_flash_attn_kv_f32(*kv_args, _stream()), "cbx_flash_attn_kv_f32"))
        return out
    args = (_p(q), _p(k), _p(v), _p(out), _p(key_lens), Z, H, Tq, Tk, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
            v.stride(0), v.stride(1), out.stride(0), out.stride(1), scale, int(causal))
    if _prec() in (3, 6, 16):  # same numerics policy as the GEMMs issued in this scope
        prec = _prec()
        fn = lambda: check(lib.cbx_flash_attn_split_f32(*args, prec, _stream()), "cbx_flash_attn_split_f32")
    else:
        fn = lambda: check(lib.cbx_flash_attn_f32(*args, _stream()), "cbx_flash_attn_f32")
    _timed("flash_attn_f32", 4.0 * Z * H * Tq * Tk * 64 * (0.5 if causal else 1.0), 4.0 * Z * H * 64 * (2 * Tq + 2 * Tk), fn)
    return out


def attn_text_mass(q, k, mass, heads, q_len, ctx0, t0, t_len, scale, weight=1.0, accumulate=False, q0=None):
    """cbx_attn_text_mass_f32 on the current stream: mass[z, i, t] (+)= weight * sum over `heads` (in list order; ints of THIS layer, 1 .. 16 of them) of the
    attention probability query i of row z puts on key t0[z] + t, the softmax taken over every visible key j <= ctx0[z] + i.  q (Z, Tq, H, 64) and k (Z, Tk, H,
    64): strided views with unit inner stride, q's head stride 64, k's free (a view of the KV cache); mass (Z, >= max q_len, >= max t_len) fp32 with unit inner
    stride.  q_len, ctx0, t0, t_len: Z Python ints each; q0 (None: zeros): query i of row z is q[z, q0[z] + i].  Elements outside [q_len) x [t_len) keep what they hold.  No host synchronisation."""
    Z, Tq, H, D = q.shape
    heads, q_len, ctx0, t0, t_len, q0 = ([int(v) for v in a] for a in (heads, q_len, ctx0, t0, t_len, [0] * Z if q0 is None else q0))
    assert D == 64 and k.shape[0] == Z and k.shape[2] == H and k.shape[3] == 64 and q.stride(3) == 1 and q.stride(2) == 64 and k.stride(3) == 1
    assert mass.dim() == 3 and mass.shape[0] == Z and mass.stride(2) == 1 and all(len(a) == Z for a in (q_len, ctx0, t0, t_len, q0))
    assert all(0 <= n <= mass.shape[1] and 0 <= a and a + n <= Tq for n, a in zip(q_len, q0)) and all(n <= mass.shape[2] for n in t_len), "attn_text_mass: a row outside q / mass"
    assert all(n == 0 or c + n <= k.shape[1] for n, c in zip(q_len, ctx0)), "attn_text_mass: a context beyond k"
    ia = lambda a: (ctypes.c_int * len(a))(*a)
    hs, ql, c0, ts, tn, qs = ia(heads), ia(q_len), ia(ctx0), ia(t0), ia(t_len), ia(q0)
    args = (_p(_f32(q, "q")), _p(_f32(k, "k")), _p(_f32(mass, "mass")), ctypes.addressof(hs), len(heads), H, ctypes.addressof(qs), ctypes.addressof(ql), ctypes.addressof(c0),
            ctypes.addressof(ts), ctypes.addressof(tn), Z, q.stride(0), q.stride(1), k.stride(0), k.stride(1), k.stride(2), mass.stride(0), mass.stride(1),
            float(scale), float(weight), int(bool(accumulate)))
    _timed("attn_text_mass", 2.0 * len(heads) * 64 * sum(n * (c + n) for n, c in zip(q_len, ctx0)), 4.0 * len(heads) * 64 * sum(c + n for n, c in zip(q_len, ctx0)),
           lambda: check(lib.cbx_attn_text_mass_f32(*args, _stream()), "cbx_attn_text_mass_f32"))
    return mass


def align_path(score, n, m):
    """cbx_align_path_f32 on the current stream: the best monotonic path through score[z, :n[z], :m[z]] (Z, N, M) fp32 with unit inner stride -- include/cbx.h
    states the recurrence.  n, m: Z Python ints each.  Returns (spans (Z, M, 2) int32: first frame and last frame + 1 of every text token, frame_tok (Z, N) int32)
    on the device; entries beyond m[z] / n[z] are zero.  Allocates the move-bit workspace.  No host synchronisation."""
    Z, N, M = score.shape
    n, m = [int(v) for v in n], [int(v) for v in m]
    assert score.stride(2) == 1 and len(n) == Z and len(m) == Z and all(1 <= v <= N for v in n) and all(1 <= v <= M for v in m), "align_path: a row outside score"
    dev = score.device
    spans = torch.zeros(Z, M, 2, dtype=torch.int32, device=dev)
    frame_tok = torch.zeros(Z, N, dtype=torch.int32, device=dev)
    ws = torch.empty(Z * max(n) * (-(-max(m) // 64)), dtype=torch.int64, device=dev)
    na, ma = (ctypes.c_int * Z)(*n), (ctypes.c_int * Z)(*m)
    _timed("align_path", 2.0 * sum(a * b for a, b in zip(n, m)), 4.0 * sum(a * b for a, b in zip(n, m)),
           lambda: check(lib.cbx_align_path_f32(_p(_f32(score, "score")), score.stride(0), score.stride(1), ctypes.addressof(na), ctypes.addressof(ma), Z, _p(spans),
                                                spans.stride(0), _p(frame_tok), frame_tok.stride(0), _p(ws), 8 * ws.numel(), _stream()), "cbx_align_path_f32"))
    return spans, frame_tok


def guard_text_mass(qkv, positions, cos_t, sin_t, kc, heads, done, t_len, t0, scale, p, qkv_ssq=None, rms_dim=0, rms_eps=1e-5, max_ctx=None):
    """cbx_guard_text_mass_f32 on the current stream, right after decode_attn_rope of the same layer and with its operands: p[s, b, t] = the attention probability
    the CURRENT query of conditional row b (head heads[s] of this layer; ints, 1 .. 16 of them) puts on key t0 + t, t < t_len[b], the softmax over every key
    j <= positions[b].  qkv (rows, 3*H*64) or (nparts, rows, 3*H*64) with qkv_ssq (nparts, 16) and rms_dim; kc (rows, H, max, 64) one layer of the cache;
    positions (rows,), done (B,), t_len (B,) int32 on the device; p (>= len(heads), B, t_cap) fp32 with unit inner stride (a view at the layer's first slot).
    Rows that are done, and columns beyond t_len, keep what they hold.  No host array changes from step to step: the launch can be captured."""
    H, B = kc.shape[1], p.shape[1]
    heads = [int(h) for h in heads]
    nparts = qkv.shape[0] if qkv.dim() == 3 else 0
    assert kc.dim() == 4 and kc.shape[3] == 64 and kc.stride(3) == 1 and kc.stride(2) == 64 and kc.shape[0] >= B and qkv.shape[-2] >= B and qkv.stride(-1) == 1
    assert p.dim() == 3 and p.stride(2) == 1 and p.shape[0] >= len(heads) and done.numel() >= B and t_len.numel() >= B and positions.numel() >= B
    assert all(t.dtype == torch.int32 for t in (positions, done, t_len)), "guard_text_mass: positions, done and t_len are int32"
    assert nparts == 0 or (qkv_ssq is not None and tuple(qkv_ssq.shape) == (nparts, 16) and rms_dim > 0)
    hs = (ctypes.c_int * len(heads))(*heads)
    args = (_p(_f32(qkv, "qkv")), qkv.stride(-2), nparts, qkv.stride(0) if nparts else 0, _p(qkv_ssq), int(rms_dim), float(rms_eps), _p(positions), _p(cos_t), _p(sin_t),
            _p(_f32(kc, "kc")), kc.stride(0), kc.stride(1), int(kc.shape[2] if max_ctx is None else max_ctx), ctypes.addressof(hs), len(heads), H, B, _p(done), _p(t_len),
            int(t0), p.shape[2], float(scale), _p(_f32(p, "p")), p.stride(0), p.stride(1))
    _timed("guard_text_mass", 2.0 * len(heads) * B * 64 * kc.shape[2], 4.0 * len(heads) * B * 64 * kc.shape[2],
           lambda: check(lib.cbx_guard_text_mass_f32(*args, _stream()), "cbx_guard_text_mass_f32"))
    return p


GUARD_NTHR = 8  # thresholds per utterance of cbx_guard_update_f32: back, ahead, end_tokens, tail, repeat, repeat_skip, token_run, hold_min


def guard_update(p, t_len, step, done, thresholds, out_tokens, mass, state, sums, trace, logits, V, eos, dev_params, n_sel=None):
    """cbx_guard_update_f32 on the current stream, between the head GEMV and t3_sample (include/cbx.h states the eight steps).  p (n_sel, B, t_cap) the slots
    guard_text_mass filled in this step; thresholds (B, 8) fp32; out_tokens (B, max_steps) int64; mass (B, max_steps, ld) the history; state (B, 8) int32, sums
    (B, 4) fp32, trace (B, max_steps) int32; logits (>= 2 B, >= V); dev_params (B, 8) the sampler's per-utterance parameters: column 6 is written.  All on the device."""
    n_sel = p.shape[0] if n_sel is None else int(n_sel)
    B, max_steps = out_tokens.shape
    assert p.dim() == 3 and p.stride(2) == 1 and p.shape[0] >= n_sel and p.shape[1] == B and mass.shape[:2] == (B, max_steps) and mass.stride(2) == 1
    assert out_tokens.dtype == torch.int64 and out_tokens.is_contiguous() and trace.dtype == torch.int32 and trace.shape == (B, max_steps) and trace.is_contiguous()
    assert state.dtype == torch.int32 and state.shape == (B, 8) and state.is_contiguous() and sums.shape == (B, 4) and sums.is_contiguous()
    assert thresholds.shape == (B, GUARD_NTHR) and thresholds.is_contiguous() and dev_params.shape == (B, 8) and dev_params.is_contiguous()
    assert all(t.dtype == torch.int32 and t.numel() >= B for t in (t_len, step, done)) and logits.shape[0] >= 2 * B and logits.stride(1) == 1 and logits.shape[1] >= V
    assert mass.stride(1) <= p.shape[2], "guard_update: a text the history row holds must fit a slot of p (the kernel follows t_len <= the history's row stride)"
    args = (_p(_f32(p, "p")), p.stride(0), p.stride(1), n_sel, _p(t_len), _p(step), _p(done), _p(_f32(thresholds, "thresholds")), _p(out_tokens), max_steps,
            _p(_f32(mass, "mass")), mass.stride(0), mass.stride(1), _p(state), _p(_f32(sums, "sums")), _p(trace), _p(_f32(logits, "logits")), logits.stride(0), int(V), B,
            int(eos), _p(_f32(dev_params, "dev_params")))
    check(lib.cbx_guard_update_f32(*args, _stream()), "cbx_guard_update_f32")


def flash_relpos(q4, pp, out, scale, key_lens=None):
    """Conformer rel-pos attention without materialised scores.  q4 (Z,T,4,H,64): the fused [q + u | q + v | k | v] projection (any batch /
    token strides, unit inner strides); pp (2T-1, H*64) = linear_pos(pos_emb); out (Z,T,H,64) view."""
    Z, T, four, H, D = q4.shape
    assert four == 4 and D == 64 and q4.stride(4) == 1 and q4.stride(3) == 64 and q4.stride(2) == H * 64
    assert pp.shape[0] == 2 * T - 1 and pp.stride(1) == 1 and out.stride(3) == 1 and out.stride(2) == 64
    args = (_p(q4[:, :, 0]), _p(q4[:, :, 1]), _p(q4[:, :, 2]), _p(q4[:, :, 3]), _p(pp), _p(out), _p(key_lens), Z, H, T,
            q4.stride(0), q4.stride(1), pp.stride(0), out.stride(0), out.stride(1), scale)
    _timed("flash_relpos_f32", 6.0 * Z * H * T * T * 64, 4.0 * Z * H * 64 * 5 * T + 4.0 * H * 64 * (2 * T - 1),
           lambda: check(lib.cbx_flash_relpos_f32(*args, _stream()), "cbx_flash_relpos_f32"))
    return out


def decode_attn(q, kc, vc, out, ctx_lens, scale):
    """q/out (rows, H*64) views; kc/vc (rows, H, max_pos, 64) contiguous caches; ctx_lens int32 (rows,)."""
    rows, H = kc.shape[0], kc.shape[1]
    check(lib.cbx_decode_attn_f32(_p(q), _p(kc), _p(vc), _p(out), _p(ctx_lens), rows, H, q.stride(0), out.stride(0),
                                  kc.stride(0), kc.stride(1), scale, _stream()), "cbx_decode_attn_f32")
    return out


_DA_WS = {}  # device index -> (partials, arrival counters) of the split-context decode attention: the TEST-HOOK workspace of the positional entry


def ensure_decode_attn_workspace(device):
    """TEST HOOK: register, once per device, the process-wide workspace the POSITIONAL cbx_decode_attn_rope_f32 splits a context through when
    rows * heads < 128 (op-level tests; single-stream use).  The engines own a DecodeAttnGeom each instead."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx in _DA_WS:
        return
    with torch.cuda.device(idx):
        ws = torch.empty(128 * 8 * 66, dtype=torch.float32, device=f"cuda:{idx}")
        cnt = torch.zeros(128, dtype=torch.int32, device=f"cuda:{idx}")
        torch.cuda.current_stream().synchronize()
        check(lib.cbx_set_decode_attn_workspace(_p(ws), _p(cnt), 128), "cbx_set_decode_attn_workspace")
    _DA_WS[idx] = (ws, cnt)


class DecodeAttnGeom:
    """Geometry + CALLER-OWNED split-context workspace of cbx_decode_attn_rope (cbx_decode_attn_t, ABI v10).  One per engine state (i.e. per
    stream of launches that may be in flight together): nothing of it is process-wide, so two engines in one process -- or a hipGraph captured
    before another engine changed its geometry -- keep their own.  Allocate outside stream captures (the engines do it at construction)."""

    def __init__(self, device, unroll=0, pipeline=0, split_min=None, max_pairs=128, split=True):
        dev = torch.device(device)
        if split_min is None:  # 0 = the library's 512
            split_min = 0
        self.unroll, self.pipeline, self.split_min, self.max_pairs = int(unroll), int(pipeline), int(split_min), int(max_pairs)
        self.ws = torch.empty(max_pairs * 8 * 66, dtype=torch.float32, device=dev) if split else None
        self.cnt = torch.zeros(max_pairs, dtype=torch.int32, device=dev) if split else None

    def fill(self, p):
        p.unroll, p.pipeline, p.split_min = self.unroll, self.pipeline, self.split_min
        p.split_ws, p.split_cnt, p.split_pairs = _p(self.ws), _p(self.cnt), (self.max_pairs if self.ws is not None else 0)


def decode_attn_rope(qkv, positions, cos_t, sin_t, kc, vc, out, scale, out_packed=False, geom=None, qkv_ssq=None, rms_dim=0, rms_eps=1e-5):
    """Fused RoPE + KV append + decode attention: qkv (rows, 3*H*64), caches (rows,H,max,64), out (rows, H*64)
    [out_packed: the packed operand image of the o-projection gemv, (ceil(rows/16)*16, H*64)].
    geom: a DecodeAttnGeom (the engines: geometry and workspace per call); None = the positional entry point on the process-wide test hooks.
    qkv (nparts, rows, 3*H*64) + qkv_ssq (nparts, rows padded to 16; rows <= 32) + rms_dim: split-K partial sums of the RMSNorm-folded projection (gemv(col_tiles=..., ksplit > 1))."""
    rows, H = kc.shape[0], kc.shape[1]
    nparts = 0
    if qkv.dim() == 3:
        assert geom is not None and qkv_ssq is not None and rms_dim > 0 and qkv.shape[0] <= 4 and qkv_ssq.shape == (qkv.shape[0], max(16, (rows + 15) // 16 * 16))
        nparts = qkv.shape[0]
    if geom is None:
        check(lib.cbx_decode_attn_rope_f32(_p(qkv), _p(positions), _p(cos_t), _p(sin_t), _p(kc), _p(vc), _p(out), rows, H,
                                           qkv.stride(0), out.stride(0), int(out_packed), kc.stride(0), kc.stride(1), scale, _stream()),
              "cbx_decode_attn_rope_f32")
        return out
    p = DecodeAttnParams()
    p.qkv, p.positions, p.cos_t, p.sin_t, p.kc, p.vc, p.o = _p(qkv), _p(positions), _p(cos_t), _p(sin_t), _p(kc), _p(vc), _p(out)
    p.rows, p.n_heads, p.ld_qkv, p.o_ld, p.o_packed = rows, H, qkv.stride(-2), out.stride(0), int(out_packed)
    p.cache_row_stride, p.cache_head_stride, p.scale = kc.stride(0), kc.stride(1), scale
    if nparts:
        p.qkv_nparts, p.qkv_part_stride, p.qkv_ssq, p.rms_dim, p.rms_eps = nparts, qkv.stride(0), _p(qkv_ssq), int(rms_dim), float(rms_eps)
    geom.fill(p)
    check(lib.cbx_decode_attn_rope(ctypes.byref(p), _stream()), "cbx_decode_attn_rope")
    return out


def gemv_row(x, w, out, *, bias=None, res=None, ln=None, eps=1e-5, parts=None, act=NONE, rows_per_wave=0):
    """Few-row decode GEMV (cbx_gemv_row_f32): out (M, N) [or (N,) for one row] = act(x' . w[n] + bias) + res, M <= 4, with x' = x (M, K) / (K,),
    LayerNorm(x) (ln = (weight, bias)) or the merge of the split-context attention records `parts` (M, n_heads, n_splits, ATTN_PART_REC) [or 3-D for one
    row] that decode_attn_parts left (x is then None).  w (N, K) row-major fp32 -- the checkpoint layout, no packed image."""
    N, K = w.shape
    o2 = out if out.dim() == 2 else out.view(1, -1)
    M = o2.shape[0]
    assert o2.shape[1] == N and M <= 4
    p = GemvRowParams()
    p.W, p.bias, p.out = _p(_f32(w, "w")), _p(bias), _p(_f32(out, "out"))
    p.M, p.ldo = M, o2.stride(0)
    if x is not None:
        x2 = x if x.dim() == 2 else x.view(1, -1)
        assert x2.shape == (M, K) and x2.stride(1) == 1
        p.x, p.ldx = _p(_f32(x, "x")), x2.stride(0)
    if res is not None:
        r2 = res if res.dim() == 2 else res.view(1, -1)
        assert r2.shape == (M, N)
        p.res, p.ldr = _p(res), r2.stride(0)
    if ln is not None:
        p.ln_w, p.ln_b, p.eps = _p(ln[0]), _p(ln[1]), eps
    if parts is not None:
        p4 = parts if parts.dim() == 4 else parts.unsqueeze(0)
        assert p4.shape[0] == M and p4.shape[3] == ATTN_PART_REC and p4[0].is_contiguous()
        p.parts, p.n_parts, p.n_heads, p.parts_row_stride = _p(parts), p4.shape[2], p4.shape[1], p4.stride(0)
    p.N, p.K, p.ldw, p.act, p.rows_per_wave = N, K, w.stride(0), act, int(rows_per_wave)
    _timed("gemv_f32", 2.0 * M * N * K, 4.0 * N * K, lambda: check(lib.cbx_gemv_row_f32(ctypes.byref(p), _stream()), "cbx_gemv_row_f32"))
    return out


def decode_attn_parts(qkv, positions, kc, vc, parts, scale, cos_t=None, sin_t=None, chunks=0):
    """Split-context decode attention that leaves its partial results (cbx_decode_attn_parts): qkv (rows, 3*H*64), caches (rows, H, max_ctx, 64),
    parts (rows, H, n_splits, ATTN_PART_REC) -- merged by the consuming gemv_row(parts=parts[row])."""
    rows, H, max_ctx = kc.shape[0], kc.shape[1], kc.shape[2]
    assert parts.shape[:2] == (rows, H) and parts.shape[3] == ATTN_PART_REC and parts.is_contiguous()
    p = AttnPartsParams()
    p.qkv, p.positions, p.cos_t, p.sin_t, p.kc, p.vc, p.parts = _p(qkv), _p(positions), _p(cos_t), _p(sin_t), _p(kc), _p(vc), _p(parts)
    p.rows, p.n_heads, p.n_splits, p.chunks, p.max_ctx = rows, H, parts.shape[2], int(chunks), max_ctx
    p.ld_qkv, p.cache_row_stride, p.cache_head_stride, p.scale = qkv.stride(0), kc.stride(0), kc.stride(1), scale
    check(lib.cbx_decode_attn_parts(ctypes.byref(p), _stream()), "cbx_decode_attn_parts")
    return parts


def gemv_flags(pre_epi=0, deep=0, shallow=0):
    return (GEMV_PRE_EPI if pre_epi else 0) | (GEMV_DEEP if deep else 0) | (GEMV_SHALLOW if shallow else 0)


def softmax_relpos(ac, bd, p, scale, key_lens=None):
    """ac (Z1,Z2,Tq,>=Tk), bd (Z1,Z2,Tq,>=2Tk-1) or None, p (Z1,Z2,Tq,ld_p) (pad columns written as 0)."""
    Z1, Z2, Tq = ac.shape[:3]
    Tk = Tq
    assert ac.is_contiguous() or ac.stride(3) == 1
    check(lib.cbx_softmax_relpos_f32(_p(ac), _p(bd), _p(p), _p(key_lens), Z1, Z2, Tq, Tk, ac.stride(2),
                                     0 if bd is None else bd.stride(2), p.stride(2), ac.stride(1),
                                     0 if bd is None else bd.stride(1), p.stride(1), scale, _stream()),
          "cbx_softmax_relpos_f32")
    return p


def softmax_rows(s, p, scale, n_keys, key_lens=None):
    """Plain row softmax of s (Z1,Z2,Tq,>=n_keys) into p (pad columns zeroed): perceiver attention."""
    Z1, Z2, Tq = s.shape[:3]
    check(lib.cbx_softmax_relpos_f32(_p(s), None, _p(p), _p(key_lens), Z1, Z2, Tq, n_keys, s.stride(2), 0, p.stride(2),
                                     s.stride(1), 0, p.stride(1), scale, _stream()), "cbx_softmax_relpos_f32")
    return p


def act(x, out, kind, param=None, slope=0.0):
    rows, C = x.shape
    check(lib.cbx_act_f32(_p(x), _p(out), _p(param), rows, C, x.stride(0), out.stride(0), kind, slope, _stream()), "cbx_act_f32")
    return out


def axpby(x, y, a=1.0, b=0.0):
    """y = a*x + b*y on 2-D strided views."""
    rows, C = x.shape
    assert x.stride(1) == 1 and y.stride(1) == 1
    check(lib.cbx_axpby_f32(_p(x), _p(y), rows, C, x.stride(0), y.stride(0), a, b, _stream()), "cbx_axpby_f32")
    return y


def embed(ids, table, out, table2=None, ids2=None, scale=1.0, out_packed=False):
    """out_packed: out is the packed operand image (ceil(rows/16)*16, C) of a decode gemv; rows = len(ids)."""
    rows, C = (ids.numel(), out.shape[1]) if out_packed else out.shape
    assert ids.dtype == torch.int64 and (ids2 is None or ids2.dtype == torch.int32)
    check(lib.cbx_embed_f32(_p(ids), _p(table), _p(table2), _p(ids2), _p(out), rows, C, out.stride(0), scale, 3 if out_packed else 1, _stream()),
          "cbx_embed_f32")
    return out


def prefill_embed(text_tokens, *, text_emb, text_pos, speech_emb, speech_pos, bos_id, n_bos, cfg, abs_pos, cond_lens, cond=None, cond_slots=None, pos0=0):
    """The prefill input of a ragged batch in ONE launch (cbx_prefill_embed): text_tokens a list of B 1-D id tensors; cond_lens[b] the conditioning positions
    in front of utterance b's text; cond (slots, Pmax, D) conditioning embeddings with cond_slots[b] the slot of utterance b -- or None when those positions
    are already in the KV cache (then pos0 = the common prefix length and x starts at the text).  Returns (x (rows, S - pos0, D), positions, cache_rows
    (rows * (S - pos0),) int32, last (rows,) int64) with rows = B * (1 + cfg).  One host buffer {meta | ids} and one host-to-device copy per batch."""
    B, dev, D = len(text_tokens), text_emb.device, text_emb.shape[1]
    ids = torch.cat([t.detach().reshape(-1).to("cpu", torch.int32) for t in text_tokens]) if B else torch.zeros(0, dtype=torch.int32)
    tl = [int(t.numel()) for t in text_tokens]
    cond_lens = [int(c) for c in cond_lens]
    slots = [-1] * B if cond is None else [int(c) for c in cond_slots]
    assert B >= 1 and len(cond_lens) == B and len(slots) == B
    assert not ids.numel() or (0 <= int(ids.min()) and int(ids.max()) < text_emb.shape[0]), "prefill_embed: a text id outside the embedding table"
    S = max(c + n + n_bos for c, n in zip(cond_lens, tl))
    if cond is None:
        assert all(c == pos0 for c in cond_lens), "prefill_embed: without conditioning embeddings every row starts behind the same cached prefix"
    else:
        _f32(cond, "cond")
        assert pos0 == 0 and cond.dim() == 3 and cond.shape[2] == D and cond.is_contiguous() and all(0 <= s_ < cond.shape[0] for s_ in slots) \
            and max(cond_lens) <= cond.shape[1], "prefill_embed: conditioning slots / lengths outside `cond`"
    assert (S <= min(text_pos.shape[0], speech_pos.shape[0])) if abs_pos else (max(tl) <= text_pos.shape[0]), "prefill_embed: position outside the position table"
    assert 0 <= int(bos_id) < speech_emb.shape[0] and all(t.shape[1] == D and t.is_contiguous() for t in (text_emb, text_pos, speech_emb, speech_pos))
    offs, o = [], 0
    for n in tl:
        offs.append(o)
        o += n
    meta = torch.tensor([v for b in range(B) for v in (offs[b], tl[b], slots[b], cond_lens[b])], dtype=torch.int32)
    buf = torch.cat([meta, ids]).to(dev, non_blocking=True)
    rows, Sx = B * (2 if cfg else 1), S - pos0
    x = torch.empty(rows, Sx, D, device=dev)
    positions = torch.empty(rows * Sx, dtype=torch.int32, device=dev)
    cache_rows = torch.empty(rows * Sx, dtype=torch.int32, device=dev)
    last = torch.empty(rows, dtype=torch.int64, device=dev)
    d = PrefillEmbed()
    d.B, d.cfg, d.n_bos, d.abs_pos, d.S, d.pos0, d.dim, d.bos_id = B, int(bool(cfg)), int(n_bos), int(bool(abs_pos)), S, int(pos0), D, int(bos_id)
    d.meta, d.ids = buf.data_ptr(), buf.data_ptr() + 16 * B
    d.cond, d.cond_stride = _p(cond), (0 if cond is None else cond.stride(0))
    d.text_emb, d.text_pos, d.speech_emb, d.speech_pos = _p(_f32(text_emb, "text_emb")), _p(_f32(text_pos, "text_pos")), _p(_f32(speech_emb, "speech_emb")), _p(_f32(speech_pos, "speech_pos"))
    d.x, d.positions, d.cache_rows, d.last = _p(x), _p(positions), _p(cache_rows), _p(last)
    check(lib.cbx_prefill_embed(ctypes.byref(d), _stream()), "cbx_prefill_embed")
    return x, positions, cache_rows, last


def kv_prefix_paste(prefixes, voice_of_row, kc, vc):
    """kc / vc[l, r, h, :P] = prefixes[voice_of_row[r]][0 / 1][l, h, :P] for every layer, row r < len(voice_of_row) and head in one launch
    (cbx_kv_prefix_paste_f32).  prefixes: list of (k, v) pairs of contiguous (L, H, P, 64) tensors; kc / vc: KV caches (L, rows, H, max_ctx, 64)."""
    L, R, H, ctx, hd = kc.shape
    nv, rows = len(prefixes), len(voice_of_row)
    P = prefixes[0][0].shape[2]
    assert hd == 64 and vc.shape == kc.shape and kc.stride() == vc.stride() and kc.stride(3) == 64 and 1 <= rows <= R and 1 <= P <= ctx
    assert all(0 <= int(v) < nv for v in voice_of_row), "kv_prefix_paste: voice index outside the prefix table"
    for k, v in prefixes:
        assert k.shape == (L, H, P, 64) and v.shape == (L, H, P, 64) and k.is_contiguous() and v.is_contiguous(), "kv_prefix_paste: prefix shape"
        _f32(k, "prefix k"), _f32(v, "prefix v")
    table = torch.tensor([k.data_ptr() for k, _ in prefixes] + [v.data_ptr() for _, v in prefixes] + [int(v) for v in voice_of_row],
                         dtype=torch.int64).to(kc.device, non_blocking=True)
    check(lib.cbx_kv_prefix_paste_f32(_p(table), nv, _p(_f32(kc, "kc")), _p(vc), L, rows, H, P, kc.stride(0), kc.stride(1), kc.stride(2), _stream()),
          "cbx_kv_prefix_paste_f32")


def rope_kv(qkv, positions, cos_t, sin_t, kc, vc, n_heads, cache_rows=None):
    """In-place RoPE on the q,k parts of qkv (rows, 3*H*64) + append k,v at `positions` into caches (rows,H,max,64)."""
    n_rows = qkv.shape[0]
    check(lib.cbx_rope_kv_f32(_p(qkv), _p(positions), _p(cos_t), _p(sin_t), _p(kc), _p(vc), _p(cache_rows), n_rows, n_heads,
                              qkv.stride(0), 0 if kc is None else kc.stride(0), 0 if kc is None else kc.stride(1),
                              _stream()), "cbx_rope_kv_f32")


def cfm_euler(xin, v, B, T, C, dt, w, cfg=True):
    """xin (rows,T,ld) packed estimator input whose first C columns are x; v (rows,T,C)."""
    check(lib.cbx_cfm_euler_f32(_p(xin), _p(v), B, T, C, xin.stride(1), v.stride(1), xin.stride(0), v.stride(0), dt, w,
                                int(cfg), _stream()), "cbx_cfm_euler_f32")


def t3_sample(**kw):
    p = SamplerParams()
    for k, val in kw.items():
        setattr(p, k, _p(val) if torch.is_tensor(val) else val)
    check(lib.cbx_t3_sample(ctypes.byref(p), _stream()), "cbx_t3_sample")


def hift_source(f0, phase, noise, lin_w, lin_b, s, frame_cum, up=480, sr=24000.0, cum_in=None):
    """cum_in (B, 9) float64 or None: the cumulative cycles the frame scan starts from (a window of a longer signal: frame_cum[:, :, w0] of that signal)."""
    B, T = f0.shape
    if cum_in is None:
        check(lib.cbx_hift_source_f32(_p(f0), _p(phase), _p(noise), _p(lin_w), float(lin_b), _p(s), _p(frame_cum), B, T, up, sr,
                                      _stream()), "cbx_hift_source_f32")
    else:
        assert cum_in.dtype == torch.float64 and cum_in.shape == (B, 9) and cum_in.is_contiguous() and cum_in.device == f0.device, "cum_in: (B, 9) float64"
        check(lib.cbx_hift_source_carry_f32(_p(f0), _p(phase), _p(noise), _p(lin_w), float(lin_b), _p(s), _p(frame_cum), _p(cum_in), B, T, up, sr,
                                            _stream()), "cbx_hift_source_carry_f32")
    return s


def stream_emit(wav, origin, meta, tail_in, ramp, out, tail_out):
    """cbx_stream_emit_f32.  wav (B, L) of the round, wav[b, q] = absolute sample origin + q; meta (4, B) int32 = emitted, end, avail, tail length (absolute
    samples); tail_in / tail_out (B, fade), ramp (fade,) -- or None when fade is 0; out (B, max_new).  Fills out[b, : end - emitted] and tail_out."""
    B, L = wav.shape
    assert wav.is_contiguous() and meta.dtype == torch.int32 and meta.shape == (4, B) and meta.is_contiguous() and meta.device == wav.device
    fade = 0 if ramp is None else int(ramp.numel())
    assert out.shape[0] == B and out.is_contiguous() and (fade == 0 or (tail_in.shape == tail_out.shape == (B, fade) and tail_in.is_contiguous()
                                                                        and tail_out.is_contiguous() and ramp.is_contiguous()))
    m = meta.data_ptr()
    check(lib.cbx_stream_emit_f32(_p(_f32(wav, "wav")), wav.stride(0), int(origin), m, m + 4 * B, m + 8 * B, _p(tail_in), m + 12 * B, _p(ramp), fade,
                                  _p(_f32(out, "out")), out.shape[1], _p(tail_out), B, _stream()), "cbx_stream_emit_f32")
    return out


# ----------------------------------------------------------------------------- per-request seeds: the counter-based RNG (cbx_rng_fill_f32)

RNG_T3_UNIFORMS, RNG_CFM_Z, RNG_VOC_PHASE, RNG_VOC_NOISE = _lib.RNG_T3_UNIFORMS, _lib.RNG_CFM_Z, _lib.RNG_VOC_PHASE, _lib.RNG_VOC_NOISE


def check_seeds(seeds, B, name="seeds"):
    """Per-request seeds as a list of B Python ints in [0, 2^64) (None stays None).  An int serves every request; anything else must be a list or tuple of
    exactly B ints.  TypeError / ValueError, before anything is launched."""
    if seeds is None:
        return None
    one = lambda s: isinstance(s, int) and not isinstance(s, bool)
    if one(seeds):
        seeds = [seeds] * B
    elif not isinstance(seeds, (list, tuple)):
        raise TypeError(f"{name}: expected an int or a list of {B} ints, got {type(seeds).__name__}")
    if len(seeds) != B:
        raise ValueError(f"{name}: {len(seeds)} entries for {B} requests")
    for k, s in enumerate(seeds):
        if not one(s):
            raise TypeError(f"{name}[{k}]: expected an int, got {type(s).__name__}")
        if not 0 <= s < 1 << 64:
            raise ValueError(f"{name}[{k}] = {s}: a seed is an int in [0, 2^64)")
    return list(seeds)


def request_seeds(seeds, B, generator=None):
    """An engine entry's `seeds` as a list of B ints or None (check_seeds).  Seeds and a torch.Generator exclude each other: ValueError."""
    seeds = check_seeds(seeds, B)
    if seeds is not None and generator is not None:
        raise ValueError("give seeds or generator, not both")
    return seeds


def rng_keys(seeds, stream, substreams=(0,), device="cpu"):
    """The (len(seeds) * len(substreams), 4) int32 key tensor of cbx_rng_fill_f32: row b * len(substreams) + h = (seed_b & 0xffffffff, seed_b >> 32,
    substreams[h], stream), the 32-bit words stored as their two's-complement int32."""
    import numpy as np
    k = np.array([[s & 0xFFFFFFFF, s >> 32, int(h), int(stream)] for s in seeds for h in substreams], dtype=np.uint32).reshape(-1, 4)
    return torch.from_numpy(k.view(np.int32)).to(device)


def rng_fill(out, keys, n=None, col0=0, normal=False):
    """cbx_rng_fill_f32: out[r, :n] = the draws of key row r at absolute columns [col0, col0 + n) -- uniform in [0, 1), or standard normal.  out (rows, >= n)
    fp32 with unit column stride (a view is fine; columns from n on are left alone), keys (rows, 4) int32 on out's device (rng_keys)."""
    assert out.dim() == 2 and (out.shape[1] <= 1 or out.stride(1) == 1), "rng_fill: out is (rows, columns) with unit column stride"
    rows = out.shape[0]
    n = out.shape[1] if n is None else int(n)
    assert 0 <= n <= out.shape[1] and (rows <= 1 or out.stride(0) >= n), "rng_fill: n exceeds the row"
    assert keys.dtype == torch.int32 and keys.shape == (rows, 4) and keys.is_contiguous() and keys.device == out.device, "rng_fill: keys is (rows, 4) int32 on out's device"
    assert 0 <= int(col0) and int(col0) + n <= 1 << 64, "rng_fill: columns are 64-bit"
    check(lib.cbx_rng_fill_f32(_p(_f32(out, "out")), out.stride(0) if rows > 1 else max(out.stride(0), n), _p(keys), rows, n, int(col0), _lib.RNG_NORMAL if normal else _lib.RNG_UNIFORM,
                               _stream()), "cbx_rng_fill_f32")
    return out


def seeded_z(seeds, frames, device, frame0=0):
    """The CFM noise of B seeded requests, (B, frames, 80) channel-last: frames [frame0, frame0 + frames) of each request's RNG_CFM_Z stream (one row per
    request, column = frame * 80 + channel, the request's own frame index -- whatever the batch's padded length)."""
    z = torch.empty(len(seeds), frames, 80, device=device)
    rng_fill(z.view(len(seeds), frames * 80), rng_keys(seeds, RNG_CFM_Z, device=device), col0=80 * int(frame0), normal=True)
    return z


def seeded_phase(seeds, device):
    """The vocoder's initial phases of B seeded requests, (B, 9): the RNG_VOC_PHASE uniforms scaled to [-pi, pi), harmonic 0 zeroed, as the unseeded draw is."""
    u = torch.empty(len(seeds), 9, device=device)
    rng_fill(u, rng_keys(seeds, RNG_VOC_PHASE, device=device))
    phase = (u * 2 - 1) * 3.141592653589793
    phase[:, 0] = 0
    return phase


def seeded_noise(seeds, n, device, col0=0):
    """The vocoder's source noise of B seeded requests, (B, 9, n): samples [col0, col0 + n) of each request's RNG_VOC_NOISE stream, substream = harmonic."""
    noise = torch.empty(len(seeds), 9, n, device=device)
    rng_fill(noise.view(len(seeds) * 9, n), rng_keys(seeds, RNG_VOC_NOISE, substreams=range(9), device=device), col0=col0, normal=True)
    return noise


# ----------------------------------------------------------------------------- speed control: the mel stretched along time (cbx_mel_time_scale_f32)

SPEED_MIN, SPEED_MAX = 0.5, 2.0


def scaled_len(n, rate):
    """Frames (or any other unit of time) that `n` of them become at speaking rate `rate`: max(1, floor(n / rate)) in Python floats.  THE definition: the
    kernel's out_lens, the vocoder's lens and the trim of the waveform all come from here."""
    import math
    return max(1, int(math.floor(int(n) / float(rate))))


def _per_request_numbers(value, B, name, lo, hi, what, *, scalar="None, a number", entry="None or a number", plural="numbers", none_as=None, finish=None):
    """The one shape of the per-request number arguments (speed, pitch, loudness, true_peak, duration): None, a number that serves every request, or a list / tuple
    of exactly B numbers / Nones, every number finite and in [lo, hi] -> B entries, a None as `none_as` and a number through `finish`, or None when every entry is
    `none_as`.  A bool or a non-number is a TypeError, a non-finite or out-of-range value and a wrong length are ValueErrors; `what`, `scalar`, `entry` and
    `plural` are the words in which the messages of the five arguments differ."""
    import math
    import numbers
    one = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)
    if value is None:
        return None
    if one(value):
        value = [value] * B
    elif not isinstance(value, (list, tuple)):
        raise TypeError(f"{name}: expected {scalar} or a list of {B} {plural}, got {type(value).__name__}")
    if len(value) != B:
        raise ValueError(f"{name}: {len(value)} entries for {B} requests")
    out = []
    for k, v in enumerate(value):
        if v is None:
            out.append(none_as)
            continue
        if not one(v):
            raise TypeError(f"{name}[{k}]: expected {entry}, got {type(v).__name__}")
        v = float(v)
        if not math.isfinite(v) or not lo <= v <= hi:
            raise ValueError(f"{name}[{k}] = {v}: {what} in [{lo}, {hi}]")
        out.append(finish(v) if finish else v)
    return None if all(v == none_as for v in out) else out


def check_speed(value, B, name="speed"):
    """A `speed` argument as a list of B floats, or None when no request is scaled (None, or every entry 1.0 or None).  A number serves every request; anything
    else must be a list or tuple of exactly B numbers (or None: 1.0) in [0.5, 2.0].  A bool or a non-number is a TypeError; a non-finite or out-of-range value and
    a wrong length are ValueErrors -- raised before anything is launched."""
    return _per_request_numbers(value, B, name, SPEED_MIN, SPEED_MAX, "a speed is a finite number", scalar="a number", entry="a number", none_as=1.0)


def mel_time_scale(mel, rates, in_lens=None, out=None):
    """cbx_mel_time_scale_f32: mel (B, T_in, C) fp32 channel-last (any batch / row stride, unit channel stride) stretched along time, row b at rates[b] (B Python
    floats) over its in_lens[b] valid frames (B ints on the host; None: T_in) -> (out, out_lens): out (B, T_out, C), frames from scaled_len(in_lens[b], rates[b])
    on zero, and out_lens the (B,) int32 device tensor of those lengths (what the vocoder takes as `lens`).  out: None (a fresh contiguous tensor, T_out = the
    longest row) or a (B, T_out, C) fp32 view with unit channel stride that holds the longest row; its columns beyond C are not touched."""
    assert mel.dim() == 3 and mel.shape[2] >= 1 and (mel.shape[2] == 1 or mel.stride(2) == 1), "mel_time_scale: mel is (B, T_in, C) with unit channel stride"
    B, T_in, C = mel.shape
    rates = [float(r) for r in rates]
    M = [T_in] * B if in_lens is None else [int(v) for v in in_lens]
    if len(rates) != B or len(M) != B:
        raise ValueError(f"mel_time_scale: {len(rates)} rates and {len(M)} lengths for {B} rows")
    if not all(0 <= m <= T_in for m in M):
        raise ValueError(f"mel_time_scale: in_lens {M} outside [0, {T_in}]")
    O = [scaled_len(m, r) for m, r in zip(M, rates)]
    if out is None:
        out = torch.empty(B, max(O), C, device=mel.device)
    assert out.dim() == 3 and out.shape[0] == B and out.shape[2] == C and (C == 1 or out.stride(2) == 1) and out.device == mel.device, "mel_time_scale: out is (B, T_out, C)"
    T_out = out.shape[1]
    if max(O) > T_out:
        raise ValueError(f"mel_time_scale: out holds {T_out} frames, the longest row needs {max(O)}")
    # rates (B doubles), in_lens and out_lens (B ints each) travel as ONE pinned buffer and one asynchronous copy: a pageable copy would hold the host until the
    # flow in front of it on this stream has finished, which is what the throughput schedule (sync=False) must not do
    dev = mel.device
    host = torch.empty(4 * B, dtype=torch.int32, pin_memory=dev.type == "cuda")
    host[: 2 * B].view(torch.float64).copy_(torch.tensor(rates, dtype=torch.float64))
    host[2 * B:].copy_(torch.tensor(M + O, dtype=torch.int32))
    args = host.to(dev, non_blocking=True)
    sb = lambda t, T: t.stride(0) if B > 1 else max(t.stride(0), T * t.stride(1), C)  # (the stride of a dimension of size 1 is arbitrary)
    check(lib.cbx_mel_time_scale_f32(_p(_f32(mel, "mel")), sb(mel, T_in), mel.stride(1) if T_in > 1 else max(mel.stride(1), C), T_in,
                                     None if in_lens is None else args.data_ptr() + 8 * B, args.data_ptr(), _p(_f32(out, "out")), sb(out, T_out),
                                     out.stride(1) if T_out > 1 else max(out.stride(1), C), T_out, args.data_ptr() + 12 * B, B, C, _stream()), "cbx_mel_time_scale_f32")
    return out, args[3 * B:]


def mel_time_scale_window(mel, rate, j0, i_org, in_lens, out_lens, out=None):
    """cbx_mel_time_scale_win_f32: a WINDOW of mel_time_scale's map for the rounds of a stream.  mel (B, T_in, C) holds absolute input frames [i_org, i_org + T_in),
    row b in_lens[b] of them; out[b, jj] for jj < out_lens[b] is absolute output frame j0 + jj at `rate` (one Python float for every row), frames from out_lens[b] on
    zero.  in_lens / out_lens: B host ints each, relative to the window; the caller decides which frames are ready (engine.stream_ready_frames).  The kernel clamps
    every tap into the row's window, so no argument can make it read outside mel.  out: None (fresh, T_out = max(out_lens)) or a (B, T_out, C) view as in
    mel_time_scale.  -> (out, the (B,) int32 device tensor of out_lens: the vocoder's `lens`)."""
    assert mel.dim() == 3 and mel.shape[2] >= 1 and (mel.shape[2] == 1 or mel.stride(2) == 1), "mel_time_scale_window: mel is (B, T_in, C) with unit channel stride"
    B, T_in, C = mel.shape
    rate, j0, i_org = float(rate), int(j0), int(i_org)
    M, O = [int(v) for v in in_lens], [int(v) for v in out_lens]
    if len(M) != B or len(O) != B:
        raise ValueError(f"mel_time_scale_window: {len(M)} input and {len(O)} output lengths for {B} rows")
    if not all(0 <= m <= T_in for m in M) or min(O, default=0) < 0:
        raise ValueError(f"mel_time_scale_window: in_lens {M} outside [0, {T_in}] or a negative out_lens {O}")
    if not (SPEED_MIN <= rate <= SPEED_MAX) or j0 < 0 or i_org < 0:
        raise ValueError(f"mel_time_scale_window: rate {rate} outside [{SPEED_MIN}, {SPEED_MAX}], or a negative origin (j0 {j0}, i_org {i_org})")
    if out is None:
        out = torch.empty(B, max(O, default=0), C, device=mel.device)
    assert out.dim() == 3 and out.shape[0] == B and out.shape[2] == C and (C == 1 or out.stride(2) == 1) and out.device == mel.device, "mel_time_scale_window: out is (B, T_out, C)"
    T_out = out.shape[1]
    if max(O, default=0) > T_out:
        raise ValueError(f"mel_time_scale_window: out holds {T_out} frames, the longest row needs {max(O)}")
    dev = mel.device
    host = torch.empty(2 * B, dtype=torch.int32, pin_memory=dev.type == "cuda")  # one pinned buffer, one asynchronous copy (mel_time_scale)
    host.copy_(torch.tensor(M + O, dtype=torch.int32))
    args = host.to(dev, non_blocking=True)
    sb = lambda t, T: t.stride(0) if B > 1 else max(t.stride(0), T * t.stride(1), C)
    check(lib.cbx_mel_time_scale_win_f32(_p(_f32(mel, "mel")), sb(mel, T_in), mel.stride(1) if T_in > 1 else max(mel.stride(1), C), T_in, args.data_ptr(), rate, j0, i_org,
                                         _p(_f32(out, "out")), sb(out, T_out), out.stride(1) if T_out > 1 else max(out.stride(1), C), T_out, args.data_ptr() + 4 * B, B, C,
                                         _stream()), "cbx_mel_time_scale_win_f32")
    return out, args[B:]


# ----------------------------------------------------------------------------- timing control: a piecewise-linear time map of the mel (cbx_mel_time_warp_f32)
MEL_WARP_MAX_ROWS = 64            # seg_off travels to the kernel by value
DURATION_MIN, DURATION_MAX = 0.02, 80.0   # seconds: one 20 ms frame .. twice the 40 s budget (1000 tokens) at rate 0.5
MEL_FRAMES_PER_S = 50


def seconds_to_frames(t):
    """Seconds -> 20 ms mel frames, floor(50 t + 0.5): half-way cases go up (Python's round sends them to the even neighbour)"""
    import math
    return int(math.floor(MEL_FRAMES_PER_S * float(t) + 0.5))


def warp_plan(K, anchors, end=None, lo=SPEED_MIN, hi=SPEED_MAX):
    """THE definition of the timing control, pure host arithmetic: the piecewise-linear map that takes the K mel frames the unwarped call returns for a row to a
    chosen number of output frames, through `anchors` = [(x, t), ...]: input frame x (a number in [0, K], nondecreasing) should land on output frame t (an int).
    The plan starts at (x, o) = (0, 0).  Anchor k with L = x_k - x_{k-1} > 0 gets n_k = min(max(t_k - o_{k-1}, ceil(L / hi), 1), floor(L / lo)) output frames,
    o_k = o_{k-1} + n_k, and the segment's rate is L / n_k -- in [lo, hi] by construction; a later anchor still aims at its absolute target, so a clamp does not
    accumulate.  An anchor whose x is 0 or equals an earlier anchor's x has no input to stretch: it is dropped (`dropped`), achieved[k] is the output frame its x
    already has, and it counts as clamped when that is not its target.  The last segment runs to x = K with target `end` (None: o_last + (K - x_last), rate 1); an
    anchor at x = K closes the plan itself, and `end` is then not honoured unless it agrees.
    -> dict(table=[(o, a, s), ...] (segment starts at output frame o, where input position a lies, and runs at rate s: mel_time_warp's row), frames = the output
    length, achieved = [o_k per anchor], clamped = [k with o_k != t_k] plus "end" when `end` was given and frames != end, dropped = [k])."""
    import math
    K = int(K)
    if K < 1:
        raise ValueError(f"warp_plan: K = {K}: a row has at least one frame")
    table, achieved, clamped, dropped = [], [], [], []
    x0, o0 = 0, 0

    def fit(L, want):
        return int(min(max(int(want), int(math.ceil(L / hi)), 1), int(math.floor(L / lo))))
    for k, (x, t) in enumerate(anchors):
        if not x0 <= x <= K:
            raise ValueError(f"warp_plan: anchor {k} at x = {x}: positions are nondecreasing in [0, {K}]")
        L = x - x0
        if L > 0:
            n = fit(L, int(t) - o0)
            table.append((o0, float(x0), L / n))
            x0, o0 = x, o0 + n
        else:
            dropped.append(k)
        achieved.append(o0)
        if o0 != int(t):
            clamped.append(k)
    L = K - x0
    if L > 0:
        n = fit(L, L if end is None else int(end) - o0)
        table.append((o0, float(x0), L / n))
        o0 += n
    if end is not None and o0 != int(end):
        clamped.append("end")
    return dict(table=table, frames=o0, achieved=achieved, clamped=clamped, dropped=dropped)


def warp_place(table, x):
    """The inverse of a row's map: input frame position x -> its output position o_k + (x - a_k) / s_k in frames, k the last segment with a_k <= x (the first
    when there is none).  At an anchor -- x = a_k -- that is exactly o_k.  The word boundaries of word_times= go through here."""
    k = 0
    for i, (_, a, _) in enumerate(table):
        if a <= x:
            k = i
    o, a, s = table[k]
    return o + (x - a) / s


def check_duration(value, B, name="duration"):
    """A `duration` argument as a list of B target lengths in FRAMES (seconds_to_frames) / Nones, or None when no request has one.  A number serves every
    request; anything else is a list or tuple of exactly B numbers / Nones in [0.02, 80] seconds.  A bool or a non-number is a TypeError; a non-finite or
    out-of-range value and a wrong length are ValueErrors -- raised before anything is launched."""
    return _per_request_numbers(value, B, name, DURATION_MIN, DURATION_MAX, "a duration is a finite number of seconds", scalar="a number of seconds",
                                entry="a number of seconds or None", plural="numbers / Nones", finish=seconds_to_frames)


def check_timing(value, B, name="timing"):
    """A `timing` argument as a list of B entries, each None or the list of its request's word starts in FRAMES (seconds_to_frames) / Nones, or None when no
    request has one.  value: None, or a list / tuple of exactly B entries, each None or a list / tuple with one entry per word: None (the word falls where it
    falls) or its start in seconds, in [0, 80] and nondecreasing over the words that have one.  A bool or a non-number is a TypeError; a non-finite, negative,
    too large or decreasing value and a wrong length are ValueErrors.  (The number of words is checked by the caller, who knows the text; a list without a
    single time is kept for that check.)"""
    import math
    import numbers
    if value is None:
        return None
    if not isinstance(value, (list, tuple)):
        raise TypeError(f"{name}: expected a list of {B} lists of word starts / Nones, got {type(value).__name__}")
    if len(value) != B:
        raise ValueError(f"{name}: {len(value)} entries for {B} requests")
    out = []
    for b, row in enumerate(value):
        if row is None:
            out.append(None)
            continue
        if not isinstance(row, (list, tuple)):
            raise TypeError(f"{name}[{b}]: expected a list with one start in seconds / None per word, got {type(row).__name__}")
        frames, last = [], None
        for k, v in enumerate(row):
            if v is None:
                frames.append(None)
                continue
            if not isinstance(v, numbers.Real) or isinstance(v, bool):
                raise TypeError(f"{name}[{b}][{k}]: expected a number of seconds or None, got {type(v).__name__}")
            v = float(v)
            if not math.isfinite(v) or not 0.0 <= v <= DURATION_MAX:
                raise ValueError(f"{name}[{b}][{k}] = {v}: a word start is a finite number of seconds in [0, {DURATION_MAX}]")
            if last is not None and v < last:
                raise ValueError(f"{name}[{b}][{k}] = {v} after {last}: word starts are nondecreasing")
            last = v
            frames.append(seconds_to_frames(v))
        out.append(frames)  # (kept even when no word has a time: the caller still checks the number of entries against the text)
    return None if all(r is None for r in out) else out


def mel_time_warp(mel, tables, in_lens=None, out=None, out_lens=None):
    """cbx_mel_time_warp_f32: mel (B, T_in, C) fp32 channel-last (any batch / row stride, unit channel stride; B <= 64) warped along time, row b by tables[b] =
    [(o, a, s), ...] (warp_plan's `table`: the segment starts at output frame o, where input position a lies, and runs at rate s) over its in_lens[b] valid frames
    (B ints on the host; None: T_in) -> (out, out_lens) as mel_time_scale returns them.  out_lens: B host ints, or None: the last segment runs to the row's end,
    o + max(1, floor((in_lens[b] - a) / s + 0.5)) -- what warp_plan's `frames` is for a plan over K = in_lens[b].  A one-segment table (0, 0.0, s) gives
    mel_time_scale's bits at rate s.  out: as in mel_time_scale."""
    import ctypes
    import math
    assert mel.dim() == 3 and mel.shape[2] >= 1 and (mel.shape[2] == 1 or mel.stride(2) == 1), "mel_time_warp: mel is (B, T_in, C) with unit channel stride"
    B, T_in, C = mel.shape
    M = [T_in] * B if in_lens is None else [int(v) for v in in_lens]
    tables = [[(int(o), float(a), float(s)) for o, a, s in tb] for tb in tables]
    if len(tables) != B or len(M) != B or not 1 <= B <= MEL_WARP_MAX_ROWS:
        raise ValueError(f"mel_time_warp: {len(tables)} tables and {len(M)} lengths for {B} rows (at most {MEL_WARP_MAX_ROWS})")
    if not all(0 <= m <= T_in for m in M):
        raise ValueError(f"mel_time_warp: in_lens {M} outside [0, {T_in}]")
    if not all(len(tb) >= 1 for tb in tables):
        raise ValueError("mel_time_warp: every row needs at least one segment")
    if out_lens is None:
        O = []
        for m, tb in zip(M, tables):
            o, a, s = tb[-1]
            n = (m - a) / s if s > 0 and math.isfinite(s) and math.isfinite(a) else 0.0
            O.append(o + max(1, int(math.floor(n + 0.5))))
    else:
        O = [int(v) for v in out_lens]
    if len(O) != B or min(O) < 0:
        raise ValueError(f"mel_time_warp: out_lens {O} for {B} rows")
    if out is None:
        out = torch.empty(B, max(O), C, device=mel.device)
    assert out.dim() == 3 and out.shape[0] == B and out.shape[2] == C and (C == 1 or out.stride(2) == 1) and out.device == mel.device, "mel_time_warp: out is (B, T_out, C)"
    T_out = out.shape[1]
    if max(O) > T_out:
        raise ValueError(f"mel_time_warp: out holds {T_out} frames, the longest row needs {max(O)}")
    # the table (S doubles seg_a, S doubles seg_s, S ints seg_o), in_lens and out_lens travel as ONE pinned buffer and one asynchronous copy (mel_time_scale);
    # seg_off stays on the host: the entry checks it and passes it by value
    S = sum(len(tb) for tb in tables)
    off = [0]
    for tb in tables:
        off.append(off[-1] + len(tb))
    dev = mel.device
    host = torch.empty(5 * S + 2 * B, dtype=torch.int32, pin_memory=dev.type == "cuda")
    host[: 4 * S].view(torch.float64).copy_(torch.tensor([a for tb in tables for _, a, _ in tb] + [s for tb in tables for _, _, s in tb], dtype=torch.float64))
    host[4 * S:].copy_(torch.tensor([o for tb in tables for o, _, _ in tb] + M + O, dtype=torch.int32))
    args = host.to(dev, non_blocking=True)
    p = args.data_ptr()
    seg_off = (ctypes.c_int * (B + 1))(*off)
    sb = lambda t, T: t.stride(0) if B > 1 else max(t.stride(0), T * t.stride(1), C)  # (the stride of a dimension of size 1 is arbitrary)
    check(lib.cbx_mel_time_warp_f32(_p(_f32(mel, "mel")), sb(mel, T_in), mel.stride(1) if T_in > 1 else max(mel.stride(1), C), T_in,
                                    None if in_lens is None else p + 4 * (5 * S), ctypes.addressof(seg_off), S, p + 4 * (4 * S), p, p + 8 * S,
                                    _p(_f32(out, "out")), sb(out, T_out), out.stride(1) if T_out > 1 else max(out.stride(1), C), T_out, p + 4 * (5 * S + B), B, C,
                                    _stream()), "cbx_mel_time_warp_f32")
    return out, args[5 * S + B:]


# ----------------------------------------------------------------------------- long-form synthesis: trim + join the waveforms of a sub-batch (wave_join.hip)
WAVE_FRAME, WAVE_JOIN_MAX_ROWS = 480, 64
JOIN_KEYS = ("gaps", "trim_db", "pad_frames", "fade", "first", "last")
_DEVICE_TABLES = {}


def _on_device(key, device, make):
    """make() -- a NumPy array or a tensor, one of the delivery kernels' tables -- on `device`: built and uploaded once per (key, device)"""
    key = (key, str(device))
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.as_tensor(make()).to(device)
    return _DEVICE_TABLES[key]


def _all_empty(rows):
    """every row is an empty tensor: such rows may have no allocation to point at, and there is nothing to launch"""
    return bool(rows) and all(torch.is_tensor(w) and w.numel() == 0 for w in rows)


def check_join(join, R, name="join"):
    """A `join` argument of the engines as a dict with every key of JOIN_KEYS, or None: gaps (R ints >= 0, samples behind each row), trim_db (None: no trimming, or
    a finite number >= 0), pad_frames (int >= 0), fade (int >= 0, samples), first / last (bools: the piece begins / ends the whole text).  Defaults: pad_frames 2,
    fade 240, first = last = True, trim_db None.  TypeError / ValueError before anything is launched."""
    import math
    import numbers
    if join is None:
        return None
    if not isinstance(join, dict):
        raise TypeError(f"{name}: expected a dict with {JOIN_KEYS}, got {type(join).__name__}")
    extra = set(join) - set(JOIN_KEYS)
    if extra or "gaps" not in join:
        raise ValueError(f"{name}: keys {sorted(join)}: `gaps` is required, the others are {JOIN_KEYS[1:]}")
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    gaps = join["gaps"]
    if not isinstance(gaps, (list, tuple)) or not all(is_int(g) for g in gaps):
        raise TypeError(f"{name}['gaps']: expected a list of {R} ints")
    if len(gaps) != R or not 1 <= R <= WAVE_JOIN_MAX_ROWS or any(g < 0 for g in gaps):
        raise ValueError(f"{name}['gaps']: {len(gaps)} entries for {R} rows (1 .. {WAVE_JOIN_MAX_ROWS} rows, every gap >= 0)")
    trim_db = join.get("trim_db")
    if trim_db is not None:
        if not isinstance(trim_db, numbers.Real) or isinstance(trim_db, bool):
            raise TypeError(f"{name}['trim_db']: expected None or a number, got {type(trim_db).__name__}")
        trim_db = float(trim_db)
        if not math.isfinite(trim_db) or trim_db < 0.0:
            raise ValueError(f"{name}['trim_db'] = {trim_db}: a finite number >= 0 (decibels below the loudest frame)")
    out = dict(gaps=[int(g) for g in gaps], trim_db=trim_db)
    for key, default in (("pad_frames", 2), ("fade", 240)):
        v = join.get(key, default)
        if not is_int(v):
            raise TypeError(f"{name}['{key}']: expected an int, got {type(v).__name__}")
        if not 0 <= v <= 1 << 20:
            raise ValueError(f"{name}['{key}'] = {v}: expected an int in [0, 2^20]")
        out[key] = v
    for key in ("first", "last"):
        v = join.get(key, True)
        if not isinstance(v, bool):
            raise TypeError(f"{name}['{key}']: expected a bool, got {type(v).__name__}")
        out[key] = v
    return out


def join_ramp(fade, device):
    """The fade ramp of cbx_wave_join_f32 on `device`: ramp[i] = (2 i + 1) / (2 fade), evaluated in fp64 and rounded to fp32 (None for fade 0); built once per
    (fade, device)."""
    fade = int(fade)
    if fade == 0:
        return None
    return _on_device(("join_ramp", fade), device, lambda: ((2.0 * torch.arange(fade, dtype=torch.float64) + 1.0) / (2.0 * fade)).float())


def _wave_rows(rows, who):
    """rows: 1 .. 64 1-D fp32 tensors with unit stride, all views of ONE allocation (what vocode cuts out of its padded (B, L) waveform) -> (pointer of the
    allocation, ctypes arrays of the per-row element offsets and lengths).  Rows of different allocations are refused."""
    rows = list(rows)
    if not 1 <= len(rows) <= WAVE_JOIN_MAX_ROWS:
        raise ValueError(f"{who}: {len(rows)} rows (1 .. {WAVE_JOIN_MAX_ROWS})")
    dev = rows[0].device
    for r, w in enumerate(rows):
        _f32(w, f"{who}: row {r}")
        if w.dim() != 1 or (w.numel() > 1 and w.stride(0) != 1) or w.device != dev:
            raise ValueError(f"{who}: row {r} is not a 1-D tensor with unit stride on {dev}")
    base = rows[0].untyped_storage().data_ptr()
    if any(w.untyped_storage().data_ptr() != base for w in rows):
        raise ValueError(f"{who}: the rows are views of different allocations; pass views of one (B, L) tensor")
    R = len(rows)
    offs = (ctypes.c_long * R)(*[(w.data_ptr() - base) // 4 if w.numel() else 0 for w in rows])
    lens = (ctypes.c_int * R)(*[int(w.numel()) for w in rows])
    return base, offs, lens


def wave_edges(rows, trim_db, pad_frames=2, edges=None):
    """cbx_wave_edges_f32: the kept part {start, stop} of every row as an (R, 2) int32 device tensor -- from the first to the last 480-sample frame whose mean
    square is above the loudest frame's times 10^(-trim_db / 10), `pad_frames` frames more on either side.  No host synchronisation."""
    base, offs, lens = _wave_rows(rows, "wave_edges")
    R, dev = len(lens), rows[0].device
    if edges is None:
        edges = torch.empty(R, 2, dtype=torch.int32, device=dev)
    assert edges.dtype == torch.int32 and edges.numel() == 2 * R and edges.is_contiguous() and edges.device == dev, "wave_edges: edges is (R, 2) int32 on the rows' device"
    n_frames = -(-max(lens) // WAVE_FRAME)
    ws = torch.empty(max(1, R * n_frames), dtype=torch.float64, device=dev)
    check(lib.cbx_wave_edges_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), R, 10.0 ** (-float(trim_db) / 10.0), int(pad_frames), _p(edges), _p(ws),
                                 ws.numel(), _stream()), "cbx_wave_edges_f32")
    return edges


def wave_join(rows, gaps, trim_db=None, pad_frames=2, fade=240, first=True, last=True, out=None, squeeze=None):
    """cbx_wave_edges_f32 (unless trim_db is None) + cbx_wave_join_f32 on the current stream: the rows' kept parts laid out in ONE buffer with their gaps and
    fades (include/cbx.h states the layout).  rows: _wave_rows; gaps: R ints.  Returns the piece, everything on the device and nothing synchronised:
    dict(out=(capacity,) fp32 of which [0, total) is the piece -- capacity = sum of the lengths and gaps; the rest is NOT written --, rec=(3 R + 1,) int32 = the
    layout record off_0 .. off_(R-1), total followed by the edge table, layout / edges = views of rec, n = the R row lengths).
    squeeze (None: this call, launch for launch; else check_pauses' dict): the pause control between the two -- edges on the ORIGINAL rows, then wave_squeeze,
    which shortens the rows and maps the table, then the join over the shortened rows with the host-side lengths n_r and the mapped table (a caller-written
    {0, n_r} has become {0, n'_r}: the zero tail never reaches the piece).  The piece gains `pauses`, wave_squeeze's stats."""
    base, offs, lens = _wave_rows(rows, "wave_join")
    R, dev = len(lens), rows[0].device
    n = [int(v) for v in lens]
    gaps = [int(g) for g in gaps]
    if len(gaps) != R:
        raise ValueError(f"wave_join: {len(gaps)} gaps for {R} rows")
    cap = sum(n) + sum(gaps)
    if out is None:
        out = torch.empty(max(1, cap), device=dev)
    assert out.dim() == 1 and out.is_contiguous() and out.device == dev, "wave_join: out is a contiguous 1-D fp32 tensor on the rows' device"
    rec = torch.empty(3 * R + 1, dtype=torch.int32, device=dev)
    layout, edges = rec[: R + 1], rec[R + 1:].view(R, 2)
    if trim_db is None:  # (0, n_r) written by the host: one small pinned copy, no synchronisation
        host = torch.tensor([v for k in n for v in (0, k)], dtype=torch.int32)
        edges.view(-1).copy_(host.pin_memory() if dev.type == "cuda" else host, non_blocking=True)
    else:
        wave_edges(rows, trim_db, pad_frames, edges=edges)
    pauses = None
    if squeeze is not None:
        sq = wave_squeeze(rows, squeeze["keep"], squeeze["db"], squeeze["fade"], edges=edges)
        pauses = sq["stats"]
        base, offs, lens = _wave_rows(sq["rows"], "wave_join")
    g = (ctypes.c_int * R)(*gaps)
    check(lib.cbx_wave_join_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), ctypes.addressof(g), R, _p(edges), _p(join_ramp(fade, dev)), int(fade),
                                int(bool(first)), int(bool(last)), _p(_f32(out, "out")), out.numel(), _p(layout), _stream()), "cbx_wave_join_f32")
    piece = dict(out=out, rec=rec, layout=layout, edges=edges, n=n)
    return piece if pauses is None else dict(piece, pauses=pauses)


# ----------------------------------------------------------------------------- pause control: shorten long silences inside the rows (wave_squeeze.hip)
WAVE_SQUEEZE_TILE = 256          # frames per step of the plan kernel's scans (WS_TILE): a pause may start in one tile and end in a later one
WAVE_SQUEEZE_MAX_KEEP = 3000     # 60 s of 480-sample frames
PAUSES_KEYS = ("keep", "db", "fade")


def check_pauses(value, B, name="pauses"):
    """A `pauses` argument of the engines as dict(keep=[B ints], db=float, fade=int), or None.  value: None; a dict(keep=, db=, fade=) whose keep is an int (every
    row) or a list of B ints / Nones; or a per-request list of B ints / Nones (the keeps, db and fade at their defaults).  keep[b]: 0 or None -- row b is left as it
    is --, else the frames (of 480 samples) that remain of every longer pause, an int in [2, 3000].  db: a finite number >= 0, decibels below the row's loudest
    frame at or under which a frame is silent (default 40).  fade: the seam's cross-fade in samples, an int in [0, 480] (default 240).  A value with no keep on
    any row is None: the call is then the call without the argument.  TypeError / ValueError before anything is launched."""
    import math
    import numbers
    if value is None:
        return None
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if isinstance(value, dict):
        extra = set(value) - set(PAUSES_KEYS)
        if extra or "keep" not in value:
            raise ValueError(f"{name}: keys {sorted(value)}: `keep` is required, the others are {PAUSES_KEYS[1:]}")
        keep, db, fade = value["keep"], value.get("db", 40.0), value.get("fade", 240)
    elif isinstance(value, (list, tuple)):
        keep, db, fade = value, 40.0, 240
    else:
        raise TypeError(f"{name}: expected None, a dict with {PAUSES_KEYS} or a list of {B} ints / Nones, got {type(value).__name__}")
    if is_int(keep):
        keep = [keep] * B
    if not isinstance(keep, (list, tuple)) or not all(k is None or is_int(k) for k in keep):
        raise TypeError(f"{name}['keep']: expected an int or a list of {B} ints / Nones")
    if len(keep) != B or not 1 <= B <= WAVE_JOIN_MAX_ROWS:
        raise ValueError(f"{name}['keep']: {len(keep)} entries for {B} rows (1 .. {WAVE_JOIN_MAX_ROWS} rows)")
    keep = [0 if k is None else int(k) for k in keep]
    if any(k != 0 and not 2 <= k <= WAVE_SQUEEZE_MAX_KEEP for k in keep):
        raise ValueError(f"{name}['keep'] = {keep}: 0 / None (the row is left alone) or an int in [2, {WAVE_SQUEEZE_MAX_KEEP}] frames")
    if not isinstance(db, numbers.Real) or isinstance(db, bool):
        raise TypeError(f"{name}['db']: expected a number, got {type(db).__name__}")
    db = float(db)
    if not math.isfinite(db) or db < 0.0:
        raise ValueError(f"{name}['db'] = {db}: a finite number >= 0 (decibels below the loudest frame)")
    if not is_int(fade):
        raise TypeError(f"{name}['fade']: expected an int, got {type(fade).__name__}")
    if not 0 <= fade <= WAVE_FRAME:
        raise ValueError(f"{name}['fade'] = {fade}: expected an int in [0, {WAVE_FRAME}]")
    return dict(keep=keep, db=db, fade=fade) if any(keep) else None


def wave_squeeze(rows, keep, db=40.0, fade=240, edges=None, out=None):
    """cbx_wave_squeeze_f32 on the current stream: of every pause (a run of silent 480-sample frames between two non-silent ones; silent = mean square at or under
    the row's loudest frame's times 10^(-db / 10)) longer than keep[r] frames only keep[r] remain, the cut cross-faded over `fade` samples (include/cbx.h states
    the definition).  rows: _wave_rows; keep: R ints, 0 = the row is copied.  edges: None, or an (R, 2) int32 device table {start, stop} on the ORIGINAL rows, which
    is rewritten in place for the shortened ones.  out: None, or the buffer to write into (row r at the offset it has in its own allocation; not that allocation).
    Returns dict(rows = views of a NEW buffer with the rows' layout, each still n_r long: [0, n'_r) the shortened
    row, [n'_r, n_r) zeros; stats = (R, 4) int32 device tensor {n', pauses cut, frames removed, n}; edges = the table or None; n = the R lengths).  Everything
    stays on the device and nothing is synchronised: n' is known to the host once `stats` has been copied."""
    base, offs, lens = _wave_rows(rows, "wave_squeeze")
    R, dev = len(lens), rows[0].device
    keep = [int(k) for k in keep]
    if len(keep) != R:
        raise ValueError(f"wave_squeeze: {len(keep)} keeps for {R} rows")
    n = [int(v) for v in lens]
    span = max(int(o) + k for o, k in zip(offs, n))
    if out is None:
        out = torch.empty(max(1, span), device=dev)
    assert out.dim() == 1 and out.is_contiguous() and out.device == dev, "wave_squeeze: out is a contiguous 1-D fp32 tensor on the rows' device"
    stats = torch.empty(R, 4, dtype=torch.int32, device=dev)
    if edges is not None:
        assert edges.dtype == torch.int32 and edges.numel() == 2 * R and edges.is_contiguous() and edges.device == dev, "wave_squeeze: edges is (R, 2) int32 on the rows' device"
    ws = torch.empty(max(1, 2 * R * -(-max(n) // WAVE_FRAME)), dtype=torch.float64, device=dev)  # 16 bytes per frame
    kp = (ctypes.c_int * R)(*keep)
    check(lib.cbx_wave_squeeze_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), ctypes.addressof(kp), R, 10.0 ** (-float(db) / 10.0), _p(join_ramp(fade, dev)),
                                   int(fade), _p(_f32(out, "out")), out.numel(), _p(edges), _p(stats), _p(ws), 8 * ws.numel(), _stream()), "cbx_wave_squeeze_f32")
    return dict(rows=[out[int(o): int(o) + k] for o, k in zip(offs, n)], stats=stats, edges=edges, n=n)


def cut_pauses(rows, stats, fmt=None):
    """The rows of wave_squeeze (or their conversion by wave_format to `fmt`) cut to their new lengths once `stats` is readable on the host: row r keeps n'_r
    samples, a converted row formatted_len(n'_r, rate) -- the conversion of a zero-tailed row is, in that range, bit for bit the conversion of the exact-length
    row: an output past it would be the first to read no sample of the row at all."""
    new = [int(s[0]) for s in stats.tolist()]
    return [w[: k if fmt is None else formatted_len(k, fmt["sample_rate"])] for w, k in zip(rows, new)]


def piece_on_host(out, rec, n, fmt=None):
    """The host's reading of a joined piece once `out` and `rec` (wave_join) are readable: dict(wav = out[:total], offsets, total, edges = [(start, stop)], n).
    fmt (a format dict; `out` is then the converted buffer of vocode(join=, format=)): wav = out[:formatted_len(total)] and the dict names the `format`; offsets,
    total and edges stay in 24 kHz samples."""
    R = len(n)
    rec = [int(v) for v in rec.tolist()]
    piece = dict(wav=out[: rec[R]], offsets=rec[:R], total=rec[R], edges=[(rec[R + 1 + 2 * r], rec[R + 2 + 2 * r]) for r in range(R)], n=list(n))
    return piece if fmt is None else dict(piece, wav=out[: formatted_len(rec[R], fmt["sample_rate"])], format=fmt)


# ----------------------------------------------------------------------------- dialogue: sum rows into one waveform, each at its own position (wave_mix.hip)
WAVE_MIX_TILE = 4096             # output samples of one workgroup of cbx_wave_mix_f32 (WM_TILE)


def mix_layout(lengths, after):
    """Where the rows of a conversation start: (starts, total) as host ints.  after[r]: the signed count of samples between the front of the conversation (the
    furthest end of any row so far) and the next non-empty row; negative: the next row comes in that many samples before the front.  The walk, with front = 0 and
    pending = 0: an empty row gets start = front and changes nothing (the join drops an empty row's gap); otherwise start_r = max(0, front + pending),
    front = max(front, start_r + n_r), pending = after[r].  total = front.  With every after >= 0 this is cbx_wave_join_f32's layout with last=True."""
    lengths, after = [int(n) for n in lengths], [int(g) for g in after]
    if len(lengths) != len(after):
        raise ValueError(f"mix_layout: {len(after)} entries of `after` for {len(lengths)} rows")
    if any(n < 0 for n in lengths):
        raise ValueError(f"mix_layout: negative length in {lengths}")
    starts, front, pending = [], 0, 0
    for n, g in zip(lengths, after):
        if n == 0:
            starts.append(front)
            continue
        start = max(0, front + pending)
        starts.append(start)
        front, pending = max(front, start + n), g
    return starts, front


def _wave_mix(who, rows, starts, flags, pan, out, gain, gain_idx, fade, accumulate):
    """The one body of wave_mix (pan None: out is 1-D) and wave_pan_mix (pan: R (left, right) pairs, out is (2, n)): the counts, `out`, the shortcut for rows that
    are all empty, _wave_rows, the gain vector and the ctypes arrays, then ONE call of cbx_<who>_f32, the C entry of the public function `who`.  Returns out."""
    rows = list(rows)
    R = len(rows)
    starts, flags = [int(s) for s in starts], [int(f) for f in flags]
    if pan is None:
        counts, shape, planes_ok = f"{len(starts)} starts and {len(flags)} flags", "1-D", out.dim() == 1
    else:
        counts, shape, planes_ok = f"{len(starts)} starts, {len(flags)} flags and {len(pan)} pan pairs", "(2, n)", out.dim() == 2 and out.shape[0] == 2
    if len(starts) != R or len(flags) != R or (pan is not None and len(pan) != R):
        raise ValueError(f"{who}: {counts} for {R} rows")
    if pan is not None and any(len(g) != 2 for g in pan):
        raise ValueError(f"{who}: pan holds one (left, right) pair per row")
    if gain_idx is not None and len(gain_idx) != R:
        raise ValueError(f"{who}: {len(gain_idx)} gain indices for {R} rows")
    assert planes_ok and out.is_contiguous(), f"{who}: out is a contiguous {shape} fp32 tensor on the rows' device"
    _f32(out, "out")
    n = int(out.shape[-1])
    if _all_empty(rows):  # (such rows may have no allocation to point at)
        if not 1 <= R <= WAVE_JOIN_MAX_ROWS or any(not 0 <= s <= n for s in starts):
            raise ValueError(f"{who}: {R} empty rows at {starts} of an output of {n}")
        return out if accumulate else out.zero_()
    base, offs, lens = _wave_rows(rows, who)
    dev = rows[0].device
    assert out.device == dev, f"{who}: out is a contiguous {shape} fp32 tensor on the rows' device"
    G = 0
    if gain is not None:
        assert gain.dtype == torch.float32 and gain.dim() == 1 and gain.is_contiguous() and gain.device == dev, f"{who}: gain is (G,) fp32 on the rows' device"
        G = int(gain.numel())
    st, fl = (ctypes.c_long * R)(*starts), (ctypes.c_int * R)(*flags)
    entry = f"cbx_{who}_f32"
    pg = None if pan is None else (ctypes.c_float * (2 * R))(*[float(v) for g in pan for v in g])
    gi = None if gain_idx is None else (ctypes.c_int * R)(*[int(g) for g in gain_idx])
    check(getattr(lib, entry)(base, ctypes.addressof(offs), ctypes.addressof(lens), ctypes.addressof(st), ctypes.addressof(fl), *(() if pg is None else (ctypes.addressof(pg),)),
                              R, _p(gain), G, None if gi is None else ctypes.addressof(gi), _p(join_ramp(fade, dev)), int(fade), _p(out),
                              *(() if pg is None else (n,)), n, int(bool(accumulate)), _stream()), entry)  # (the plane stride of a contiguous (2, n) is n)
    return out


def wave_mix(rows, starts, flags, out, gain=None, gain_idx=None, fade=240, accumulate=False):
    """cbx_wave_mix_f32 on the current stream: row r (_wave_rows: 1 .. 64 1-D fp32 views of ONE allocation) times its gain, with the join's fades, ADDED into
    out[starts[r], starts[r] + n_r) -- rows that cover the same sample are summed in ascending r (include/cbx.h states the definition).  starts: R ints >= 0;
    flags: R ints, bit 0 the row fades in, bit 1 it fades out, over min(fade, n_r / 2) samples of join_ramp(fade).  out: a contiguous 1-D fp32 tensor on the rows'
    device, not the rows' allocation; every sample of it is written (+0.0 where no row is) unless accumulate, which adds to what it holds and leaves uncovered
    samples alone.  gain: None (every row at 1, no multiply) or a (G,) fp32 device tensor; gain_idx: None (row r uses gain[r]) or R ints in [0, G).  One launch,
    nothing is synchronised.  Returns out."""
    return _wave_mix("wave_mix", rows, starts, flags, None, out, gain, gain_idx, fade, accumulate)


# ----------------------------------------------------------------------------- pitch control: the waveform read back at a real step (wave_pitch.hip)
PITCH_MIN, PITCH_MAX = -12.0, 12.0               # semitones a caller may ask for
PITCH_Z, PITCH_L, PITCH_BETA = 16, 256, 9.0      # zero crossings per side, table steps per crossing, Kaiser beta: UNMEASURED choices
_PITCH_FILTER = {}


def pitch_ratio(p):
    """The frequency ratio of `p` semitones: 2.0 ** (p / 12.0) in Python floats.  THE definition: the mel's stretch and the kernel's step come from here."""
    return 2.0 ** (float(p) / 12.0)


def check_pitch(value, B, name="pitch"):
    """A `pitch` argument as a list of B floats (semitones; a None entry is 0.0), or None when no request is transposed (None, or every entry None or 0).  A
    number serves every request; anything else must be a list or tuple of exactly B numbers / Nones in [-12, 12].  A bool or a non-number is a TypeError; a
    non-finite or out-of-range value and a wrong length are ValueErrors -- raised before anything is launched."""
    return _per_request_numbers(value, B, name, PITCH_MIN, PITCH_MAX, "a pitch is a finite number of semitones", none_as=0.0)


def check_speed_pitch(speed, pitch, B):
    """The rates at which the mel is stretched when `speed` and `pitch` (as check_speed / check_pitch take them) meet: None without a pitch -- the call is then
    the one with `speed` alone --, else B floats s_eff[b] = speed[b] / pitch_ratio(pitch[b]), a request without a pitch at exactly its speed.  The vocoder's
    source is 480 scaled_len(K, s_eff) samples, read at a step of pitch_ratio into 480 scaled_len(K, speed).  Every s_eff must lie in [0.5, 2.0], where the mel's
    stretch is defined: otherwise a ValueError that names both arguments, before anything is launched."""
    speed, pitch = check_speed(speed, B), check_pitch(pitch, B)
    if pitch is None:
        return None
    speed = [1.0] * B if speed is None else speed
    eff = [s if p == 0.0 else s / pitch_ratio(p) for s, p in zip(speed, pitch)]
    for k, (s, p, e) in enumerate(zip(speed, pitch, eff)):
        if not SPEED_MIN <= e <= SPEED_MAX:
            raise ValueError(f"speed[{k}] = {s} with pitch[{k}] = {p}: the mel would be stretched at speed / 2^(pitch / 12) = {e:.4f}, outside [{SPEED_MIN}, {SPEED_MAX}]")
    return eff


def pitch_filter():
    """The interpolation filter of the pitch step, built once in NumPy fp64: h(t) = sinc(t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta) for |t| < Z, else 0 -- a
    Kaiser-windowed sinc of Z = 16 zero crossings per side, beta = 9.0 -- as the fp32 table tab[k] = h(k / L), k = 0 .. Z L + 1, L = 256 steps per crossing (4098
    floats, 16 KiB).  tab[0] = 1; tab[k] = 0 exactly at every other multiple of L and for k >= Z L: a step of 1 then returns the input's bits."""
    import numpy as np
    if not _PITCH_FILTER:
        Z, L, beta = PITCH_Z, PITCH_L, PITCH_BETA
        t = np.arange(Z * L + 2, dtype=np.float64) / L
        h = np.sinc(t) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / Z) ** 2))) / np.i0(beta)
        h[0] = 1.0
        h[L::L] = 0.0
        h[Z * L:] = 0.0
        _PITCH_FILTER.update(Z=Z, L=L, beta=beta, h=h, tab=np.ascontiguousarray(h.astype(np.float32)))
    return _PITCH_FILTER


def _pitch_table(device):
    """pitch_filter's table on `device`, uploaded once per device"""
    return _on_device("pitch", device, lambda: pitch_filter()["tab"])


def wave_pitch(rows, steps, out_lens):
    """cbx_wave_pitch_f32 on the current stream: row r (_wave_rows: 1 .. 64 1-D fp32 views of ONE allocation) read at a step of steps[r] source samples per output
    sample (R Python floats in [0.5, 2.0]) into out_lens[r] samples, through pitch_filter's windowed sinc with its cutoff at min(1, 1 / step) of the source's Nyquist
    rate, in ONE launch (include/cbx.h states the definition).  Samples outside a row read as zeros; a step of 1 copies the row.  Returns R 1-D fp32 tensors that
    are views of one packed device buffer, each beginning on a 16-byte boundary of it.  No host synchronisation."""
    rows = list(rows)
    steps, out_lens = [float(s) for s in steps], [int(n) for n in out_lens]
    if len(steps) != len(rows) or len(out_lens) != len(rows):
        raise ValueError(f"wave_pitch: {len(steps)} steps and {len(out_lens)} lengths for {len(rows)} rows")
    if any(n < 0 for n in out_lens):
        raise ValueError(f"wave_pitch: out_lens {out_lens}")
    if _all_empty(rows):  # (every tap reads outside its row)
        return [torch.zeros(n, device=w.device) for w, n in zip(rows, out_lens)]
    base, offs, lens = _wave_rows(rows, "wave_pitch")
    R, dev, f = len(lens), rows[0].device, pitch_filter()
    starts, pos = [], 0
    for n in out_lens:
        starts.append(pos)
        pos += -(-n // 4) * 4
    packed = torch.empty(max(1, pos), device=dev)
    st, ol, o = (ctypes.c_double * R)(*steps), (ctypes.c_int * R)(*out_lens), (ctypes.c_long * R)(*starts)
    check(lib.cbx_wave_pitch_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), ctypes.addressof(st), ctypes.addressof(ol), R, _p(_pitch_table(dev)), f["Z"], f["L"],
                                 _p(packed), ctypes.addressof(o), packed.numel(), _stream()), "cbx_wave_pitch_f32")
    return [packed[a: a + n] for a, n in zip(starts, out_lens)]


# ----------------------------------------------------------------------------- output formats: resample + encode ahead of the copy to the host (wave_format.hip)
WAVE_IN_RATE = 24000
WAVE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
WAVE_ENCODINGS = ("f32", "s16", "mulaw", "alaw")   # cbx_wave_format_f32's encoding 0 .. 3
_WAVE_DTYPES = (torch.float32, torch.int16, torch.uint8, torch.uint8)
_WAVE_FILTERS = {}


def check_format(sample_rate=None, encoding=None, name="format"):
    """The output format of a call: None for the default (sample_rate None / 24000 and encoding None / "f32": the call is then exactly the one without the
    arguments), else dict(sample_rate=int, encoding=str).  sample_rate: an int of WAVE_RATES (a bool or a non-int is a TypeError); encoding: a str of
    WAVE_ENCODINGS.  TypeError / ValueError before anything is launched."""
    if sample_rate is None:
        sample_rate = WAVE_IN_RATE
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int):
        raise TypeError(f"{name}: sample_rate: expected None or an int, got {type(sample_rate).__name__}")
    if sample_rate not in WAVE_RATES:
        raise ValueError(f"{name}: sample_rate = {sample_rate}: expected one of {WAVE_RATES}")
    if encoding is None:
        encoding = "f32"
    if not isinstance(encoding, str):
        raise TypeError(f"{name}: encoding: expected None or a str, got {type(encoding).__name__}")
    if encoding not in WAVE_ENCODINGS:
        raise ValueError(f"{name}: encoding = {encoding!r}: expected one of {WAVE_ENCODINGS}")
    return None if (sample_rate, encoding) == (WAVE_IN_RATE, "f32") else dict(sample_rate=sample_rate, encoding=encoding)


def check_format_arg(fmt, name="format"):
    """A `format` argument of the engines -- None, or a dict with the keys sample_rate and / or encoding -- as check_format returns it."""
    if fmt is None:
        return None
    if not isinstance(fmt, dict):
        raise TypeError(f"{name}: expected None or a dict(sample_rate=, encoding=), got {type(fmt).__name__}")
    if set(fmt) - {"sample_rate", "encoding"}:
        raise ValueError(f"{name}: keys {sorted(fmt)}: expected sample_rate and / or encoding")
    return check_format(fmt.get("sample_rate"), fmt.get("encoding"), name)


def _wave_fmt(fmt):
    """(rate, encoding index) of a format dict; None is 24 kHz fp32 (the identity, still one launch)"""
    fmt = check_format_arg(fmt) or dict(sample_rate=WAVE_IN_RATE, encoding="f32")
    return fmt["sample_rate"], WAVE_ENCODINGS.index(fmt["encoding"])


def _poly_filter(U, D):
    """THE resampler design of the delivery kernels, scipy.signal.resample_poly's for the reduced ratio U / D restated in NumPy fp64 (no SciPy in the product
    path): hl = 10 max(U, D), h = U firwin(2 hl + 1, 1 / max(U, D), window=("kaiser", 5.0)) -- the windowed sinc cutoff sinc(cutoff (i - hl)) times np.kaiser,
    scaled to unit gain at 0 --, tab (U, T) fp32 = h[p + j U] (zero past 2 hl), T = ceil((2 hl + 1) / U) taps per output, H = ceil(2 hl / U) samples of history.
    U == D: no filter (U = D = T = 1, hl = H = 0, tab = [[1]]).  -> a new dict(U, D, hl, T, H, h, tab)."""
    import numpy as np
    if U == D:
        return dict(U=1, D=1, hl=0, T=1, H=0, h=np.ones(1), tab=np.ones((1, 1), np.float32))
    hl, cutoff = 10 * max(U, D), 1.0 / max(U, D)
    i = np.arange(2 * hl + 1, dtype=np.float64) - hl
    h = cutoff * np.sinc(cutoff * i) * np.kaiser(2 * hl + 1, 5.0)
    h = U * (h / h.sum())
    T = -(-(2 * hl + 1) // U)
    pad = np.zeros(U * T)
    pad[: 2 * hl + 1] = h
    return dict(U=U, D=D, hl=hl, T=T, H=-(-2 * hl // U), h=h, tab=np.ascontiguousarray(pad.reshape(T, U).T.astype(np.float32)))


def wave_filter(sample_rate):
    """The resampler 24000 -> sample_rate as scipy.signal.resample_poly designs it (_poly_filter states the design): U / D the reduced ratio, hl = 10 max(U, D),
    h the fp64 taps, tab (U, T) fp32 = h[p + j U], T = ceil((2 hl + 1) / U) taps per output, H = ceil(2 hl / U) samples of history.
    24000: no filter (hl = H = 0, T = 1, tab = [[1]]).  Built once per rate."""
    import math
    if sample_rate not in _WAVE_FILTERS:
        if sample_rate not in WAVE_RATES:
            raise ValueError(f"sample_rate = {sample_rate}: expected one of {WAVE_RATES}")
        g = math.gcd(sample_rate, WAVE_IN_RATE)
        _WAVE_FILTERS[sample_rate] = _poly_filter(sample_rate // g, WAVE_IN_RATE // g)
    return _WAVE_FILTERS[sample_rate]


def _wave_table(sample_rate, device):
    """wave_filter's phase table on `device`, uploaded once per (device, rate)"""
    return _on_device(("wave", sample_rate), device, lambda: wave_filter(sample_rate)["tab"])


def formatted_len(n, sample_rate):
    """Samples at `sample_rate` of n samples at 24 kHz: ceil(n U / D)"""
    f = wave_filter(WAVE_IN_RATE if sample_rate is None else sample_rate)
    return -(-int(n) * f["U"] // f["D"])


def _wave_counts(f, n0, m0, lens, final):
    """outputs of one cbx_wave_format_f32 launch per row (include/cbx.h states the rule)"""
    out = []
    for a, b, L, fin in zip(n0, m0, lens, final):
        N = a + L
        m1 = -(-N * f["U"] // f["D"]) if fin else max(0, ((N - 1) * f["U"] - f["hl"]) // f["D"] + 1)
        out.append(max(0, m1 - b))
    return out


def _wave_format_launch(rows, rate, enc, n0=None, m0=None, final=None, hist_in=None, hist_out=None):
    """One cbx_wave_format_f32 launch on the current stream -> (packed output buffer, [(offset, count)] per row).  No host synchronisation."""
    base, offs, lens = _wave_rows(rows, "wave_format")
    R, dev, f = len(lens), rows[0].device, wave_filter(rate)
    one_shot = n0 is None
    cnt = _wave_counts(f, [0] * R if one_shot else n0, [0] * R if one_shot else m0, [int(v) for v in lens], [True] * R if one_shot else final)
    starts = [sum(cnt[:r]) for r in range(R)]
    packed = torch.empty(max(1, sum(cnt)), dtype=_WAVE_DTYPES[enc], device=dev)
    o = (ctypes.c_long * R)(*starts)
    cont = [None] * 3 if one_shot else [(ctypes.c_long * R)(*n0), (ctypes.c_long * R)(*m0), (ctypes.c_int * R)(*[int(bool(v)) for v in final])]
    check(lib.cbx_wave_format_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), R, rate, enc, _p(_wave_table(rate, dev)) if f["hl"] else None, f["U"], f["T"],
                                  *[None if c is None else ctypes.addressof(c) for c in cont], _p(hist_in), _p(hist_out), _p(packed), ctypes.addressof(o),
                                  packed.numel(), _stream()), "cbx_wave_format_f32")
    return packed, list(zip(starts, cnt))


def wave_format(rows, fmt):
    """cbx_wave_format_f32 on the current stream: rows (_wave_rows: 1 .. 64 1-D fp32 views of ONE allocation, 24 kHz) resampled to fmt["sample_rate"] and stored
    as fmt["encoding"] (check_format's dict; None: 24 kHz fp32) in ONE launch.  Returns R 1-D tensors (float32, int16 or uint8; row r has
    formatted_len(n_r, sample_rate) elements) that are views of one packed device buffer: `rows[0]._base` of the result is what a single copy takes to the host.
    No host synchronisation."""
    rate, enc = _wave_fmt(fmt)
    rows = list(rows)
    if _all_empty(rows):
        return [torch.empty(0, dtype=_WAVE_DTYPES[enc], device=w.device) for w in rows]
    packed, spans = _wave_format_launch(rows, rate, enc)
    return [packed[a: a + c] for a, c in spans]


class WaveFormatStream:
    """cbx_wave_format_f32 over the pieces of B signals that arrive round by round: per row the samples consumed (n0), the outputs produced (m0) and the last H
    samples (two (B, H) device buffers, ping-pong).  push(rows, final) converts the rows' new pieces in ONE launch; the concatenated results of a row are bit for
    bit wave_format of the concatenated pieces.  A row is flushed by the push that carries final[b] = True; later pushes give it nothing."""

    def __init__(self, B, fmt, device):
        self.rate, self.enc = _wave_fmt(fmt)
        self.B, self.dev, self.f = int(B), torch.device(device), wave_filter(self.rate)
        self.n0, self.m0, self.closed = [0] * self.B, [0] * self.B, [False] * self.B
        self.hist = [torch.zeros(self.B, max(1, self.f["H"]), device=self.dev) for _ in range(2)]
        self.cur, self.packed, self.spans = 0, None, None

    def push(self, rows, final):
        """rows: B 1-D fp32 tensors on the device, views of ONE allocation (None or an empty tensor: nothing new for that row); final: B bools.  Returns B 1-D
        tensors, views of self.packed (one buffer: a single copy takes the round to the host; self.spans = [(offset, count)])."""
        rows, final = list(rows), [bool(v) for v in final]
        if len(rows) != self.B or len(final) != self.B:
            raise ValueError(f"WaveFormatStream.push: {len(rows)} rows and {len(final)} flags for {self.B} signals")
        anchor = next((w for w in rows if w is not None and w.numel()), self.hist[0].view(-1))  # (an empty tensor may have no allocation at all)
        rows = [anchor[:0] if (w is None or not w.numel() or self.closed[b]) else w for b, w in enumerate(rows)]
        final = [fin or self.closed[b] for b, fin in enumerate(final)]
        lens = [int(w.numel()) for w in rows]
        self.packed, self.spans = _wave_format_launch(rows, self.rate, self.enc, self.n0, self.m0, final, self.hist[self.cur], self.hist[1 - self.cur])
        self.cur = 1 - self.cur
        for b in range(self.B):
            self.n0[b] += lens[b]
            self.m0[b] += self.spans[b][1]
            self.closed[b] = final[b]
        return [self.packed[a: a + c] for a, c in self.spans]


# ----------------------------------------------------------------------------- loudness: BS.1770 meter, gain to a LUFS target (wave_loudness.hip)
LOUDNESS_MIN, LOUDNESS_MAX = -50.0, -5.0   # LUFS targets a caller may ask for
_LOUDNESS_FILTERS = {}


def loudness_filter(fs=WAVE_IN_RATE):
    """The K-weighting of ITU-R BS.1770-4 at sample rate fs as pyloudnorm.Meter builds it (RBJ biquads, fp64 NumPy, normalised by a0): a high shelf of +4 dB,
    Q = 1 / sqrt 2 at 1500 Hz, then a high pass of Q = 0.5 at 38 Hz.  -> dict(fs, hop = fs / 10 samples, coef = 10 doubles b0 b1 b2 a1 a2 of the shelf, then of
    the high pass: cbx_wave_loudness_f32's `coef`).  fs must be a multiple of 10.  Built once per rate."""
    import numpy as np
    fs = int(fs)
    if fs not in _LOUDNESS_FILTERS:
        if fs < 10 or fs % 10:
            raise ValueError(f"loudness_filter: fs = {fs}: a tenth of a second must be a whole number of samples")
        A = 10.0 ** (4.0 / 40.0)
        w0 = 2.0 * np.pi * (1500.0 / fs)
        al, cs = np.sin(w0) / (2.0 * (1.0 / np.sqrt(2.0))), np.cos(w0)
        shelf = np.array([A * ((A + 1) + (A - 1) * cs + 2 * np.sqrt(A) * al), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - 2 * np.sqrt(A) * al),
                          (A + 1) - (A - 1) * cs + 2 * np.sqrt(A) * al, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - 2 * np.sqrt(A) * al], dtype=np.float64)
        w0 = 2.0 * np.pi * (38.0 / fs)
        al, cs = np.sin(w0) / (2.0 * 0.5), np.cos(w0)
        hp = np.array([(1 + cs) / 2, -(1 + cs), (1 + cs) / 2, 1 + al, -2 * cs, 1 - al], dtype=np.float64)
        coef = np.concatenate([np.delete(q / q[3], 3) for q in (shelf, hp)])
        _LOUDNESS_FILTERS[fs] = dict(fs=fs, hop=fs // 10, coef=coef)
    return _LOUDNESS_FILTERS[fs]


def check_loudness(value, B, name="loudness"):
    """A `loudness` argument as a list of B entries -- a float (the LUFS target of that request) or None (that request is left alone) --, or None when no request
    is normalised.  A number serves every request; anything else must be a list or tuple of exactly B numbers or Nones, each number finite and in [-50, -5].  A
    bool or a non-number is a TypeError; a non-finite or out-of-range value and a wrong length are ValueErrors -- raised before anything is launched."""
    return _per_request_numbers(value, B, name, LOUDNESS_MIN, LOUDNESS_MAX, "a loudness target is a finite number of LUFS")


def _loudness_blocks(who, target, S, unit, f, dev):
    """What every call of the meter builds for its S signals (`unit`: what `who` calls them): the targets as S doubles (one number serves all; None: NaN, gain 1),
    the filter's ten coefficients, the (S, 4) float64 stats and the (S,) float32 gain on `dev`."""
    if target is None or not isinstance(target, (list, tuple)):
        target = [target] * S
    if len(target) != S:
        raise ValueError(f"{who}: {len(target)} targets for {S} {unit}")
    tg = (ctypes.c_double * S)(*[float("nan") if t is None else float(t) for t in target])
    return tg, (ctypes.c_double * 10)(*f["coef"].tolist()), torch.empty(S, 4, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float32, device=dev)


def _wave_loudness(who, rows, C, target, ceiling, fs):
    """The one body of wave_loudness (C None: cbx_wave_loudness_f32, a signal per row) and wave_loudness_ch (cbx_wave_loudness_ch_f32: signals of C rows)"""
    base, offs, lens = _wave_rows(rows, who)
    R, dev, f = len(lens), rows[0].device, loudness_filter(fs)
    tg, coef, stats, gain = _loudness_blocks(who, target, R // (C or 1), "rows" if C is None else "signals", f, dev)
    ws = torch.empty(max(1, 6 * R * -(-max(lens) // f["hop"])), dtype=torch.float64, device=dev)
    entry = f"cbx_{who}_f32"
    check(getattr(lib, entry)(base, ctypes.addressof(offs), ctypes.addressof(lens), R, *(() if C is None else (C,)), ctypes.addressof(coef), f["hop"], ctypes.addressof(tg),
                              0.0 if ceiling is None else float(ceiling), _p(stats), _p(gain), _p(ws), ws.numel(), _stream()), entry)
    return stats, gain


def wave_loudness(rows, target=None, ceiling=1.0, fs=WAVE_IN_RATE):
    """cbx_wave_loudness_f32 on the current stream: the BS.1770-4 integrated loudness and the sample peak of every row (_wave_rows: 1 .. 64 1-D fp32 views of ONE
    allocation, sampled at fs), and the gain that brings it to its target.  target: None (measure only), a number, or R numbers / Nones (None: gain 1); no range is
    imposed here (check_loudness is the public arguments' check).  ceiling: the sample peak the gain may not exceed (None or 0: no limit).  Returns (stats, gain):
    stats (R, 4) float64 {L in LUFS (-inf: silence or shorter than 0.4 s), peak, gain in fp64, blocks used} and gain (R,) float32, both on the device; nothing is
    synchronised (include/cbx.h states the definition)."""
    return _wave_loudness("wave_loudness", rows, None, target, ceiling, fs)


def wave_loudness_push(meter, rows, target=None, ceiling=1.0):
    """cbx_wave_loudness_push_f32 on the current stream: the rows' new pieces (_wave_rows: R 1-D fp32 views of ONE allocation; an empty row: nothing new) enter
    `meter` (a WaveLoudnessStream of R rows, which owns the records, the two tails, n0 and the workspace and is advanced here).  target, ceiling: wave_loudness's.
    Returns (stats, gain) on the device as wave_loudness does -- bit for bit what wave_loudness gives for each row's pieces so far, concatenated.  Nothing is
    synchronised.  A push that would pass the meter's seg_cap is refused by the entry (-22): WaveLoudnessStream.push grows the record first."""
    base, offs, lens = _wave_rows(rows, "wave_loudness_push")
    R, dev, f = len(lens), rows[0].device, meter.f
    if R != meter.R:
        raise ValueError(f"wave_loudness_push: {R} rows for a meter of {meter.R}")
    tg, coef, stats, gain = _loudness_blocks("wave_loudness_push", target, R, "rows", f, dev)
    n0 = (ctypes.c_long * R)(*meter.n0)
    k_max = max((a % f["hop"] + int(n)) // f["hop"] for a, n in zip(meter.n0, lens))
    if meter.ws.numel() < 4 * R * k_max:
        meter.ws = torch.empty(4 * R * k_max, dtype=torch.float64, device=dev)
    check(lib.cbx_wave_loudness_push_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), ctypes.addressof(n0), R, ctypes.addressof(coef), f["hop"],
                                         ctypes.addressof(tg), 0.0 if ceiling is None else float(ceiling), _p(meter.rec), meter.seg_cap, _p(meter.tail[meter.cur]),
                                         _p(meter.tail[1 - meter.cur]), _p(stats), _p(gain), _p(meter.ws), meter.ws.numel(), _stream()), "cbx_wave_loudness_push_f32")
    meter.cur = 1 - meter.cur
    meter.n0 = [a + int(n) for a, n in zip(meter.n0, lens)]
    return stats, gain


class WaveLoudnessStream:
    """cbx_wave_loudness_push_f32 over the pieces of R signals that arrive one after the other: a running BS.1770-4 meter.  Per row a device record of 8 + seg_cap
    doubles (the K-weighting's state on entry to the unfinished 100 ms segment, the running peak, the table of segment energies), two (R, hop) tail buffers
    (ping-pong) with the unfinished segment's samples, the samples consumed (n0, on the host) and the workspace.  push(rows, target, ceiling) measures in at most
    four launches; after ANY sequence of pushes its (stats, gain) are bit for bit wave_loudness of each row's concatenated pieces -- the "integrated so far"
    reading of a live meter.  The record grows by a device copy when a push would pass seg_cap (4096 segments are 6.8 minutes; one hour is 36 000)."""

    def __init__(self, R, device, fs=WAVE_IN_RATE, seg_cap=4096):
        self.R, self.dev, self.f, self.seg_cap = int(R), torch.device(device), loudness_filter(fs), max(1, int(seg_cap))
        if not 1 <= self.R <= WAVE_JOIN_MAX_ROWS:
            raise ValueError(f"WaveLoudnessStream: {self.R} rows (1 .. {WAVE_JOIN_MAX_ROWS})")
        self.rec = torch.zeros(self.R, 8 + self.seg_cap, dtype=torch.float64, device=self.dev)
        self.tail = [torch.zeros(self.R, self.f["hop"], device=self.dev) for _ in range(2)]
        self.ws = torch.empty(4 * self.R, dtype=torch.float64, device=self.dev)
        self.n0, self.cur = [0] * self.R, 0

    def push(self, rows, target=None, ceiling=1.0):
        """rows: R 1-D fp32 tensors on the device, views of ONE allocation (None or an empty tensor: nothing new for that row).  Returns wave_loudness_push's
        (stats, gain)."""
        rows = list(rows)
        if len(rows) != self.R:
            raise ValueError(f"WaveLoudnessStream.push: {len(rows)} rows for {self.R} signals")
        anchor = next((w for w in rows if w is not None and w.numel()), self.tail[0].view(-1))  # (an empty tensor may have no allocation at all)
        rows = [anchor[:0] if (w is None or not w.numel()) else w for w in rows]
        need = max((a + int(w.numel())) // self.f["hop"] for a, w in zip(self.n0, rows))
        if need > self.seg_cap:
            cap = max(need, 2 * self.seg_cap)
            rec = torch.zeros(self.R, 8 + cap, dtype=torch.float64, device=self.dev)
            rec[:, : 8 + self.seg_cap].copy_(self.rec)
            self.rec, self.seg_cap = rec, cap
        return wave_loudness_push(self, rows, target, ceiling)


def wave_gain(rows, gain):
    """cbx_wave_gain_f32 on the current stream: row r times gain[r] (an (R,) fp32 device tensor), in place, one launch.  Returns rows."""
    base, offs, lens = _wave_rows(rows, "wave_gain")
    R = len(lens)
    assert gain.dtype == torch.float32 and gain.numel() == R and gain.is_contiguous() and gain.device == rows[0].device, "wave_gain: gain is (R,) fp32 on the rows' device"
    check(lib.cbx_wave_gain_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), R, _p(gain), _stream()), "cbx_wave_gain_f32")
    return rows


def wave_normalize(rows, target, ceiling=1.0, fs=WAVE_IN_RATE):
    """wave_loudness + wave_gain: every row with a target is brought to it in place (limited to a sample peak of `ceiling`); rows whose target is None, silent rows
    and rows shorter than 0.4 s keep their samples.  Returns the (R, 4) stats.  Five launches, no host synchronisation."""
    rows = list(rows)
    if _all_empty(rows):
        return torch.tensor([[float("-inf"), 0.0, 1.0, 0.0]] * len(rows), dtype=torch.float64).to(rows[0].device)
    stats, gain = wave_loudness(rows, target, ceiling, fs)
    wave_gain(rows, gain)
    return stats


# ----------------------------------------------------------------------------- true-peak limiter: a dBTP ceiling with look-ahead (wave_limit.hip)
TRUE_PEAK_MIN, TRUE_PEAK_MAX = -20.0, 0.0   # dBTP ceilings a caller may ask for
LIMIT_OVERSAMPLE = 4                        # U: the true peak is read on the 4-times oversampled signal (ITU-R BS.1770-4 annex 2 asks for at least 4 at 48 kHz)
LIMIT_LOOK = 120                            # H: look-ahead and release, samples at 24 kHz (5 ms).  UNMEASURED choice
LIMIT_LOOK_MAX = 480
_LIMIT_FILTER, _LIMIT_WINDOWS = [], {}


def true_peak_filter():
    """The oversampler of the true-peak meter, wave_filter's design (scipy.signal.resample_poly's, restated in NumPy fp64): U = 4, hl = 10 U = 40,
    h = U firwin(2 hl + 1, 1 / U, window=("kaiser", 5.0)), tab (U, T) fp32 = h[p + j U] (zero past 2 hl), T = ceil((2 hl + 1) / U) = 21.  Built once."""
    if not _LIMIT_FILTER:
        f = _poly_filter(LIMIT_OVERSAMPLE, 1)
        _LIMIT_FILTER.append({k: f[k] for k in ("U", "hl", "T", "h", "tab")})
    return _LIMIT_FILTER[0]


def limit_window(H=LIMIT_LOOK):
    """The limiter's smoothing window for a look-ahead of H samples (1 .. 480): w_k ~ 0.5 (1 + cos(pi k / (H + 1))), k = -H .. H, normalised to sum 1 in fp64,
    as 2 H + 1 float32 (cbx_wave_limit_f32's `win`).  Built once per H."""
    import numpy as np
    if isinstance(H, bool) or not isinstance(H, int):
        raise TypeError(f"limit_window: H: expected an int, got {type(H).__name__}")
    if not 1 <= H <= LIMIT_LOOK_MAX:
        raise ValueError(f"limit_window: H = {H} outside [1, {LIMIT_LOOK_MAX}]")
    if H not in _LIMIT_WINDOWS:
        w = 0.5 * (1.0 + np.cos(np.pi * np.arange(-H, H + 1, dtype=np.float64) / (H + 1)))
        _LIMIT_WINDOWS[H] = (w / w.sum()).astype(np.float32)
    return _LIMIT_WINDOWS[H]


def _limit_tables(H, device):
    """(phase table, window) on `device`, each uploaded once per device (the window per H)"""
    return _on_device("true_peak", device, lambda: true_peak_filter()["tab"]), _on_device(("limit_window", H), device, lambda: limit_window(H))


def check_true_peak(value, B, name="true_peak"):
    """A `true_peak` argument as a list of B entries -- a float (the ceiling of that request in dBTP) or None (that request is not limited) --, or None when no
    request is limited.  A number serves every request; anything else must be a list or tuple of exactly B numbers or Nones, each number finite and in [-20, 0].
    A bool or a non-number is a TypeError; a non-finite or out-of-range value and a wrong length are ValueErrors -- raised before anything is launched."""
    return _per_request_numbers(value, B, name, TRUE_PEAK_MIN, TRUE_PEAK_MAX, "a true-peak ceiling is a finite number of dBTP")


def _wave_limit(who, rows, C, ceilings_db, gain, look, out, measure):
    """The one body of wave_limit / wave_true_peak (C None: cbx_wave_limit_f32, a signal per row) and wave_limit_ch (cbx_wave_limit_ch_f32: signals of C rows).
    ceilings_db: a number of dBTP or None for every signal, or one per signal; out: None (measure: nothing is written; else ONE new allocation in the layout of
    `rows`) or rows of the lengths of `rows`, views of ONE allocation that is not the rows'.  Returns (out rows or None, the (S, 4) stats on the device)."""
    rows = list(rows)
    S, unit, letter = (len(rows), "rows", "R") if C is None else (len(rows) // C, "signals", "S")
    if ceilings_db is None or not isinstance(ceilings_db, (list, tuple)):
        ceilings_db = [ceilings_db] * S
    if len(ceilings_db) != S:
        raise ValueError(f"{who}: {len(ceilings_db)} ceilings for {S} {unit}")
    limit_window(look)
    if _all_empty(rows):
        outs = None if measure else (list(out) if out is not None else [torch.empty(0, dtype=torch.float32, device=w.device) for w in rows])
        return outs, torch.tensor([[0.0, 1.0, 0.0, 0.0]] * S, dtype=torch.float64).to(rows[0].device)
    base, offs, lens = _wave_rows(rows, who)
    R, dev, f = len(lens), rows[0].device, true_peak_filter()
    if out is None and not measure:
        lo = min(a for a, n in zip(offs, lens) if n)
        buf = torch.empty(max(a + n for a, n in zip(offs, lens) if n) - lo, dtype=torch.float32, device=dev)
        out = [buf[a - lo: a - lo + n] if n else buf[:0] for a, n in zip(offs, lens)]
    tab, win = _limit_tables(look, dev)
    ceil = (ctypes.c_double * S)(*[float("nan") if c is None else 10.0 ** (float(c) / 20.0) for c in ceilings_db])
    if gain is not None:
        assert gain.dtype == torch.float32 and gain.numel() == S and gain.is_contiguous() and gain.device == dev, f"{who}: gain is ({letter},) fp32 on the rows' device"
    obase, ooffs, cap = None, None, 0
    if out is not None:
        out = list(out)
        obase, o, olens = _wave_rows(out, f"{who}: out")
        if list(olens) != list(lens):
            raise ValueError(f"{who}: the rows of out have other lengths than the rows")
        ooffs, cap = ctypes.addressof(o), max((a + n for a, n in zip(o, olens)), default=0)
    stats = torch.empty(S, 4, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, 4 * S * -(-max(lens) // 1024)), dtype=torch.float64, device=dev)
    entry = f"cbx_{who}_f32"
    check(getattr(lib, entry)(base, ctypes.addressof(offs), ctypes.addressof(lens), R, *(() if C is None else (C,)), _p(gain), ctypes.addressof(ceil), _p(tab), f["U"], f["T"],
                              _p(win), look, obase, ooffs, cap, _p(stats), _p(ws), ws.numel(), _stream()), entry)
    return out, stats


def wave_true_peak(rows):
    """cbx_wave_limit_f32 as a meter, on the current stream: the true peak (4-times oversampled, linear) of every row (_wave_rows: 1 .. 64 1-D fp32 views of ONE
    allocation at 24 kHz).  Returns the (R, 4) float64 stats {true peak (NaN for a row with a NaN), 1, 0, 0} on the device; nothing is written but them, nothing is
    synchronised."""
    return _wave_limit("wave_limit", rows, None, None, None, LIMIT_LOOK, None, True)[1]


def wave_limit(rows, ceilings_db, gain=None, look=LIMIT_LOOK, out=None):
    """cbx_wave_limit_f32 on the current stream: every row (_wave_rows: 1 .. 64 1-D fp32 views of ONE allocation at 24 kHz) times gain[r] (an (R,) fp32 device
    tensor, wave_loudness's; None: 1) and held under its true-peak ceiling by a look-ahead limiter of `look` samples (include/cbx.h states the definition).
    ceilings_db: a number of dBTP, or R numbers / Nones (None: the row is not limited and comes back as x * gain, wave_gain's bits); no range is imposed here
    (check_true_peak is the public arguments' check).  Returns (out_rows, stats): out_rows are views of ONE new allocation in the layout of `rows` (out: R rows of
    the same lengths in an allocation of the caller's instead), stats (R, 4) float64 {true peak of x * gain, min g, samples with g < 1, samples over the ceiling} on
    the device.  Two launches, nothing is synchronised."""
    return _wave_limit("wave_limit", rows, None, ceilings_db, gain, look, out, False)


# ----------------------------------------------------------------------------- stereo dialogue: panned mix, channel-summed meter, linked limiter (wave_stereo.hip)
def check_pan(value, name="pan"):
    """A stereo position as a float: -1 is hard left, 0 the centre, +1 hard right.  A bool or a non-number is a TypeError, a value that is not finite or lies
    outside [-1, 1] a ValueError -- raised before anything is launched."""
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"{name}: expected a number in [-1, 1] (-1 left, 0 centre, +1 right), got {type(value).__name__}")
    value = float(value)
    if not math.isfinite(value) or not -1.0 <= value <= 1.0:
        raise ValueError(f"{name} = {value}: a stereo position is a finite number in [-1, 1] (-1 left, 0 centre, +1 right)")
    return value


def pan_gains(p):
    """The constant-power pan law: position p in [-1, 1] -> (left, right) gains as Python floats that hold fp32 values.  theta = (p + 1) pi / 4, left = cos theta,
    right = sin theta, evaluated in fp64 and rounded to fp32 once; left^2 + right^2 = 1, so a voice keeps its power wherever it sits.  By construction, not by
    trusting cos(pi / 2): p = -1 is exactly (1, 0), p = +1 exactly (0, 1), and p = 0 gives the SAME float on both sides (the fp32 of sqrt(1 / 2))."""
    import numpy as np
    p = check_pan(p, "pan_gains: p")
    if p == -1.0:
        return 1.0, 0.0
    if p == 1.0:
        return 0.0, 1.0
    if p == 0.0:
        c = float(np.float32(math.sqrt(0.5)))
        return c, c
    th = (p + 1.0) * math.pi / 4.0
    return float(np.float32(math.cos(th))), float(np.float32(math.sin(th)))


def wave_pan_mix(rows, starts, flags, pan, out, gain=None, gain_idx=None, fade=240, accumulate=False):
    """cbx_wave_pan_mix_f32 on the current stream: wave_mix into TWO planes.  rows, starts, flags, gain, gain_idx, fade, accumulate: wave_mix's.  pan: R pairs
    (left gain, right gain) of finite numbers (pan_gains gives the constant-power pair of a position).  out: a contiguous (2, n) fp32 tensor on the rows' device,
    not the rows' allocation: out[0] is the left plane, out[1] the right.  Row r times its balance gain and fades, times its left / right gain, ADDED into both
    planes at starts[r]; the covering rows are summed in ascending r per plane (include/cbx.h states the definition).  Every sample of both planes is written
    (+0.0 where no row is) unless accumulate.  One launch, nothing is synchronised.  Returns out."""
    return _wave_mix("wave_pan_mix", rows, starts, flags, pan, out, gain, gain_idx, fade, accumulate)


def _channel_groups(rows, channels, who):
    """the rows of a linked entry: a whole number of signals of `channels` rows of one length each"""
    rows, C = list(rows), int(channels)
    if C not in (1, 2):
        raise ValueError(f"{who}: channels = {channels} outside {{1, 2}}")
    if len(rows) % C:
        raise ValueError(f"{who}: {len(rows)} rows are no whole number of signals of {C} channels")
    if any(rows[k].numel() != rows[k - k % C].numel() for k in range(len(rows))):
        raise ValueError(f"{who}: the channels of a signal have different lengths")
    return rows, C


def wave_loudness_ch(rows, target=None, ceiling=1.0, fs=WAVE_IN_RATE, channels=2):
    """cbx_wave_loudness_ch_f32 on the current stream: wave_loudness for len(rows) / channels signals of `channels` (1 or 2) consecutive rows of one length each --
    the BS.1770-4 loudness of the channels' SUMMED block energies (weights 1: left and right), the larger channel's sample peak, ONE gain per signal.  target:
    None (measure only), a number, or one number / None per SIGNAL; ceiling: wave_loudness's.  Returns (stats (S, 4) float64, gain (S,) float32) on the device,
    S = len(rows) / channels; channels=1 is wave_loudness bit for bit.  Nothing is synchronised (include/cbx.h states the definition)."""
    rows, C = _channel_groups(rows, channels, "wave_loudness_ch")
    return _wave_loudness("wave_loudness_ch", rows, C, target, ceiling, fs)


def wave_limit_ch(rows, ceilings_db, gain=None, look=LIMIT_LOOK, out=None, channels=2):
    """cbx_wave_limit_ch_f32 on the current stream: wave_limit with LINKED channels, for len(rows) / channels signals of `channels` (1 or 2) consecutive rows of one
    length each: the per-sample peak is the larger channel's, ONE gain envelope multiplies both channels, so a peak on one side does not move the image.
    ceilings_db: None (measure only: the stats alone, nothing is written), a number of dBTP, or one number / None per SIGNAL (None: the signal comes back as
    x * gain); gain: an (S,) fp32 device tensor (wave_loudness_ch's) or None.  Returns (out_rows, stats): out_rows in the layout of `rows` (None when measuring only),
    stats (S, 4) float64 {true peak over the channels of x * gain, min g, samples with g < 1, samples over the ceiling}.  channels=1 is wave_limit bit for bit.
    Two launches, nothing is synchronised."""
    rows, C = _channel_groups(rows, channels, "wave_limit_ch")
    return _wave_limit("wave_limit_ch", rows, C, ceilings_db, gain, look, out, ceilings_db is None and out is None)


# ----------------------------------------------------------------------------- music bed: speech over a background that ducks while someone talks (wave_duck.hip)
BED_FRAME = 240                                                    # Q: samples of a control frame (10 ms at 24 kHz)
BED_HOLD_MAX, BED_S_MAX, BED_FADE_MAX = 200, 100, 24000            # the entry's caps: pre / post and S in frames, xf / fi / fo in samples
BED_DEFAULTS = dict(level=-12.0, duck=-9.0, threshold=-40.0, pre=0.10, post=0.30, ramp=0.25, lead=0.0, tail=0.0, fade_in=0.02, fade_out=0.5, loop=True, loop_fade=0.1)
_BED_RANGES = dict(level=(-60.0, 20.0), duck=(-60.0, 0.0), threshold=(-100.0, 0.0), pre=(0.0, 2.0), post=(0.0, 2.0), ramp=(0.02, 2.0), lead=(0.0, 600.0), tail=(0.0, 600.0),
                   fade_in=(0.0, 1.0), fade_out=(0.0, 1.0), loop_fade=(0.0, 1.0))


def check_bed(value, name="bed"):
    """A `bed` argument of generate_dialogue / generate_long -> None, or the plan ops.wave_duck takes.  value: None; an audio input (whatever audio_prompt_path=
    takes: check_audio_in); or a dict with `audio` plus overrides of BED_DEFAULTS:
      level      the bed's loudness in LU relative to the speech (BS.1770-4 over the whole of each), [-60, 20]                      default -12
      duck       dB the bed goes down by while someone talks, [-60, 0] (0: no ducking)                                              default  -9
      threshold  dBFS: a 10 ms frame whose speech peak is above it counts as talk, [-100, 0]                                        default -40
      pre, post  seconds the bed is down before a word / stays down after it, [0, 2]                                                default 0.10 / 0.30
      ramp       seconds a transition of the gain takes (the raised-cosine window: S = round(50 ramp) frames either side), [0.02, 2] default 0.25
      lead, tail seconds of bed alone before / after the speech, [0, 600]                                                           default 0 / 0
      fade_in, fade_out  seconds the bed fades in at the start / out at its end, [0, 1]                                             default 0.02 / 0.5
      loop       bool: a source shorter than the programme repeats (False: it ends, with its fade-out)                              default True
      loop_fade  seconds of cross-fade at the loop seam, [0, 1] (the source must be longer than twice that)                         default 0.1
    Every default is an UNMEASURED choice: nobody has tuned them by listening.  A wrong type or an unknown key is a TypeError, a value out of
    range or not finite a ValueError; both name `bed`.  The plan: dict(audio=the input as given (check_audio_in has passed it), level, duck, threshold (dB), lead, tail, fi, fo, xf (samples at
    24 kHz), pre, post, S (frames of 10 ms), loop)."""
    import math
    import numbers
    if value is None:
        return None
    if isinstance(value, dict):
        extra = set(value) - set(BED_DEFAULTS) - {"audio"}
        if extra or "audio" not in value:
            raise TypeError(f"{name}: keys {sorted(value, key=str)}: `audio` is required, the others are {tuple(BED_DEFAULTS)}")
        audio, given = value["audio"], {k: v for k, v in value.items() if k != "audio"}
    else:
        audio, given = value, {}
    if audio is None or isinstance(audio, (bool, numbers.Number, dict)):
        raise TypeError(f"{name}: expected None, an audio input or a dict with `audio`, got {type(audio).__name__}")
    check_audio_in(audio, name=f"{name}: audio")
    v = dict(BED_DEFAULTS, **given)
    if not isinstance(v["loop"], bool):
        raise TypeError(f"{name}['loop']: expected a bool, got {type(v['loop']).__name__}")
    for key, (lo, hi) in _BED_RANGES.items():
        x = v[key]
        if isinstance(x, bool) or not isinstance(x, numbers.Real):
            raise TypeError(f"{name}['{key}']: expected a number, got {type(x).__name__}")
        x = float(x)
        if not math.isfinite(x) or not lo <= x <= hi:
            raise ValueError(f"{name}['{key}'] = {x}: a finite number in [{lo}, {hi}]")
        v[key] = x
    sec = lambda t: int(round(t * WAVE_IN_RATE))
    fr = lambda t: int(round(t * WAVE_IN_RATE / BED_FRAME))
    return dict(audio=audio, level=v["level"], duck=v["duck"], threshold=v["threshold"], lead=sec(v["lead"]), tail=sec(v["tail"]), fi=sec(v["fade_in"]), fo=sec(v["fade_out"]),
                xf=sec(v["loop_fade"]), pre=fr(v["pre"]), post=fr(v["post"]), S=max(1, int(round(v["ramp"] * 50.0))), loop=v["loop"])


def bed_len(n, plan):
    """Samples of the output of wave_duck for n samples of speech: lead + n + tail"""
    return int(plan["lead"]) + int(n) + int(plan["tail"])


def wave_duck_level(stats_s, stats_b, level):
    """cbx_wave_duck_level_f32 on the current stream: the bed gains (R,) fp32 on the device from two (R, 4) float64 stats blocks of wave_loudness in measure-only
    mode (speech, bed): 10^((Ls + level - Lb) / 20), `level` (a number or R numbers) in LU relative to the speech; where a reading is not finite (silence, or
    shorter than 0.4 s) 10^(level / 20).  One launch, nothing is synchronised."""
    R, dev = int(stats_s.shape[0]), stats_s.device
    for st in (stats_s, stats_b):
        assert st.dtype == torch.float64 and tuple(st.shape) == (R, 4) and st.is_contiguous() and st.device == dev, "wave_duck_level: stats are (R, 4) float64 on one device"
    if not isinstance(level, (list, tuple)):
        level = [level] * R
    if len(level) != R:
        raise ValueError(f"wave_duck_level: {len(level)} levels for {R} rows")
    lv = (ctypes.c_double * R)(*[float(x) for x in level])
    gain = torch.empty(R, dtype=torch.float32, device=dev)
    check(lib.cbx_wave_duck_level_f32(_p(stats_s), _p(stats_b), ctypes.addressof(lv), R, _p(gain), _stream()), "cbx_wave_duck_level_f32")
    return gain


def wave_duck(speech_rows, bed_rows, plan, gain=None, out=None):
    """cbx_wave_duck_f32 on the current stream: every speech row (_wave_rows: 1 .. 64 1-D fp32 views of ONE allocation at 24 kHz; None or an empty tensor: no
    speech) over its bed source (bed_rows: None -- no bed at all --, or R rows of ONE allocation, None / empty ones allowed) times gain[r] (an (R,) fp32 device
    tensor, wave_duck_level's; None: 1), the bed pulled down by plan["duck"] dB around the frames where the speech peaks above plan["threshold"] dBFS
    (include/cbx.h states the definition).  plan: check_bed's dict, of which duck, threshold, lead, tail, pre, post, S, loop, xf, fi, fo are read.  Returns
    (out_rows, stats): out_rows of bed_len(n_r, plan) samples each, views of ONE new allocation, back to back (out: R rows of those lengths in an allocation of
    the caller's instead, overlapping neither input); stats (R, 4) float64 {the gain as applied, frames ducked, frames, max |out| (NaN: the row holds one)} on the
    device.  Three launches -- none when every output row is empty --, nothing is synchronised."""
    speech_rows = list(speech_rows)
    R = len(speech_rows)
    bed_rows = [None] * R if bed_rows is None else list(bed_rows)
    if len(bed_rows) != R:
        raise ValueError(f"wave_duck: {len(bed_rows)} bed rows for {R} speech rows")

    def anchored(rows, who):
        anchor = next((w for w in rows if w is not None and w.numel()), None)
        if anchor is None:
            return None
        return [anchor[:0] if (w is None or not w.numel()) else w for w in rows]
    dev = next((w.device for w in speech_rows + bed_rows + list(out or []) if w is not None), None)
    if gain is not None:
        dev = gain.device if dev is None else dev
        assert gain.dtype == torch.float32 and gain.numel() == R and gain.is_contiguous() and gain.device == dev, "wave_duck: gain is (R,) fp32 on the rows' device"
    sp, bd = anchored(speech_rows, "speech"), anchored(bed_rows, "bed")
    n = [0 if w is None else int(w.numel()) for w in speech_rows]
    N = [bed_len(k, plan) for k in n]
    win = limit_window(int(plan["S"]))  # (TypeError / ValueError for an S the window does not take; S <= 100 is the entry's own check)
    if max(N, default=0) == 0:
        if not 1 <= R <= WAVE_JOIN_MAX_ROWS:
            raise ValueError(f"wave_duck: {R} rows (1 .. {WAVE_JOIN_MAX_ROWS})")
        stats = torch.zeros(R, 4, dtype=torch.float64, device=dev)
        stats[:, 0] = 1.0 if gain is None else gain.double()
        return (list(out) if out is not None else [torch.empty(0, dtype=torch.float32, device=dev) for _ in range(R)]), stats
    if out is None:
        starts = [sum(N[:r]) for r in range(R)]
        buf = torch.empty(max(1, sum(N)), dtype=torch.float32, device=dev)
        out = [buf[a: a + k] for a, k in zip(starts, N)]
    else:
        out = list(out)
    obase, ooffs, olens = _wave_rows(out, "wave_duck: out")
    if list(olens) != N:
        raise ValueError(f"wave_duck: the rows of out have the lengths {list(olens)}, the plan gives {N}")
    cap = max((a + k for a, k in zip(ooffs, olens)), default=0)
    zero_off, zero_len = (ctypes.c_long * R)(), (ctypes.c_int * R)()
    if sp is None:  # (no speech at all: bed alone over lead + tail; the entry wants a pointer, and reads nothing through it)
        sbase, soffs, slens = obase, zero_off, zero_len
    else:
        sbase, soffs, slens = _wave_rows(sp, "wave_duck: speech")
    bbase, boffs, blens = (None, zero_off, zero_len) if bd is None else _wave_rows(bd, "wave_duck: bed")
    xf = int(plan["xf"])
    ramp = join_ramp(xf, dev) if plan["loop"] and xf > 0 else None
    stats = torch.empty(R, 4, dtype=torch.float64, device=dev)
    n_max = max(N)
    ws = torch.empty(max(1, R * (-(-n_max // BED_FRAME) + 4 * -(-n_max // 1024))), dtype=torch.float32, device=dev)
    check(lib.cbx_wave_duck_f32(sbase, ctypes.addressof(soffs), ctypes.addressof(slens), bbase, ctypes.addressof(boffs), ctypes.addressof(blens), R, _p(gain),
                                int(plan["lead"]), int(plan["tail"]), 10.0 ** (float(plan["threshold"]) / 20.0), 10.0 ** (float(plan["duck"]) / 20.0), int(plan["pre"]),
                                int(plan["post"]), int(plan["S"]), _p(_on_device(("limit_window", int(plan["S"])), dev, lambda: win)), int(bool(plan["loop"])), xf, _p(ramp),
                                int(plan["fi"]), int(plan["fo"]), obase, ctypes.addressof(ooffs), cap, _p(stats), _p(ws), ws.numel(), _stream()), "cbx_wave_duck_f32")
    return out, stats


# ----------------------------------------------------------------------------- audio in: decode + mixdown + resample, trim edges (wave_ingest.hip)
WAVE_IN_ENCODINGS =("u8", "s16", "s24", "s32", "f32", "mulaw", "alaw")   # cbx_wave_ingest's encoding 0 .. 6 (CBX_WAVE_IN_*)
WAVE_IN_SAMPLE_BYTES = dict(u8=1, s16=2, s24=3, s32=4, f32=4, mulaw=1, alaw=1)
WAVE_IN_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)   # the source rates every analysis rate (16000, 24000) is tested at
WAVE_INGEST_MAX_SPAN, WAVE_INGEST_MAX_TAB = 2048, 16384   # CBX_WAVE_INGEST_MAX_SPAN / _TAB of include/cbx.h
WAVE_IN_MAX_CHANNELS = 8
_WAVE_IN_DTYPES = {torch.uint8: None, torch.int16: "s16", torch.int32: "s32", torch.float32: "f32"}   # a typed row must hold its own encoding; uint8 rows hold any
_RESAMPLE_FILTERS = {}


def resample_filter(rate_in, rate_out):
    """wave_filter for any pair of rates: the resampler rate_in -> rate_out as scipy.signal.resample_poly designs it (NumPy fp64; _poly_filter states the design):
    dict(U, D, hl, T, h, tab (U, T) fp32).  Equal rates: no filter (U = D = T = 1, hl = 0).  Rates are positive ints (TypeError / ValueError); a pair whose reduced
    table or tile span is over cbx_wave_ingest's caps is a ValueError -- there is no host fallback.  Built once per pair."""
    import math
    for name, v in (("rate_in", rate_in), ("rate_out", rate_out)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name}: expected an int, got {type(v).__name__}")
        if v < 1:
            raise ValueError(f"{name} = {v}: a sample rate is a positive int")
    key = (rate_in, rate_out)
    if key not in _RESAMPLE_FILTERS:
        g = math.gcd(rate_in, rate_out)
        U, D = rate_out // g, rate_in // g
        T = -(-(20 * max(U, D) + 1) // U)  # (the caps are checked ahead of the design: a table over them is never built)
        if U != D and (U * T > WAVE_INGEST_MAX_TAB or 255 * D // U + T + 1 > WAVE_INGEST_MAX_SPAN):
            raise ValueError(f"no conversion from {rate_in} to {rate_out} samples per second: U / D = {U} / {D} needs a table of {U * T} floats (cap "
                             f"{WAVE_INGEST_MAX_TAB}) and a span of {255 * D // U + T + 1} frames (cap {WAVE_INGEST_MAX_SPAN})")
        f = _poly_filter(U, D)
        del f["H"]
        _RESAMPLE_FILTERS[key] = f
    return _RESAMPLE_FILTERS[key]


def _resample_table(rate_in, rate_out, device):
    """resample_filter's phase table on `device`, uploaded once per (device, pair)"""
    return _on_device(("resample", rate_in, rate_out), device, lambda: resample_filter(rate_in, rate_out)["tab"])


def resampled_len(n, rate_in, rate_out):
    """Samples at rate_out of n samples at rate_in: ceil(n U / D)"""
    f = resample_filter(rate_in, rate_out)
    return -(-int(n) * f["U"] // f["D"])


def check_audio_in(audio, name="audio"):
    """An audio input of the public classes, checked before anything is launched (TypeError / ValueError) -> a dict:
      a path (str / bytes / os.PathLike)                      dict(kind="path", path=)
      (waveform, sample_rate)                                 dict(kind="pair", wav=, rate=)
      (data, sample_rate, encoding[, channels])               dict(kind="raw", data=, rate=, encoding=, channels=, frames=)
    data: bytes / bytearray / memoryview, or a uint8 / int16 / int32 / float32 NumPy array or tensor holding interleaved frames (an int16, int32 or float32
    container must carry the encoding s16, s32 or f32; bytes and uint8 carry any); encoding: one of WAVE_IN_ENCODINGS; channels: an int in [1, 8], default 1;
    sample_rate: a positive int.  The data must be a whole number of frames."""
    import numpy as np
    if isinstance(audio, (str, bytes, os.PathLike)):
        return dict(kind="path", path=os.fspath(audio))
    if not isinstance(audio, (tuple, list)) or not 2 <= len(audio) <= 4:
        raise TypeError(f"{name}: expected a path, a (waveform, sample_rate) pair or a (data, sample_rate, encoding[, channels]) tuple, got {type(audio).__name__}")
    rate = audio[1]
    if isinstance(rate, (np.integer,)):
        rate = int(rate)
    if isinstance(rate, bool) or not isinstance(rate, int):
        raise TypeError(f"{name}: sample_rate: expected an int, got {type(audio[1]).__name__}")
    if rate < 1:
        raise ValueError(f"{name}: sample_rate = {rate}: a sample rate is a positive int")
    if len(audio) == 2:
        return dict(kind="pair", wav=audio[0], rate=rate)
    data, enc, ch = audio[0], audio[2], (audio[3] if len(audio) == 4 else 1)
    if not isinstance(enc, str):
        raise TypeError(f"{name}: encoding: expected a str, got {type(enc).__name__}")
    if enc not in WAVE_IN_ENCODINGS:
        raise ValueError(f"{name}: encoding = {enc!r}: expected one of {WAVE_IN_ENCODINGS}")
    if isinstance(ch, bool) or not isinstance(ch, int):
        raise TypeError(f"{name}: channels: expected an int, got {type(ch).__name__}")
    if not 1 <= ch <= WAVE_IN_MAX_CHANNELS:
        raise ValueError(f"{name}: channels = {ch}: expected 1 .. {WAVE_IN_MAX_CHANNELS}")
    if isinstance(data, (bytes, bytearray, memoryview)):
        nbytes, own = memoryview(data).nbytes, None
    elif torch.is_tensor(data) or isinstance(data, np.ndarray):
        dt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}.get(data.dtype, data.dtype) \
            if isinstance(data, np.ndarray) else data.dtype
        if dt not in _WAVE_IN_DTYPES:
            raise TypeError(f"{name}: data of dtype {data.dtype}: expected uint8, int16, int32 or float32")
        nbytes, own = (data.nbytes if isinstance(data, np.ndarray) else data.numel() * data.element_size()), _WAVE_IN_DTYPES[dt]
    else:
        raise TypeError(f"{name}: data: expected bytes, a bytearray, a memoryview, a NumPy array or a tensor, got {type(data).__name__}")
    if own is not None and own != enc:
        raise ValueError(f"{name}: {data.dtype} data holds the encoding {own!r}, not {enc!r} (pass bytes or uint8 for any encoding)")
    fb = ch * WAVE_IN_SAMPLE_BYTES[enc]
    if nbytes % fb:
        raise ValueError(f"{name}: {nbytes} bytes are not a whole number of frames of {ch} x {WAVE_IN_SAMPLE_BYTES[enc]} bytes")
    return dict(kind="raw", data=data, rate=rate, encoding=enc, channels=ch, frames=nbytes // fb)


def _ingest_rows(rows, enc, channels):
    """rows: 1 .. 64 1-D tensors of raw samples with unit stride, all views of ONE allocation -- uint8 for any encoding, or int16 / int32 / float32 holding s16 / s32
    / f32 -> (pointer of the allocation, ctypes arrays of the per-row byte offsets and frame counts)."""
    rows = list(rows)
    if not 1 <= len(rows) <= WAVE_JOIN_MAX_ROWS:
        raise ValueError(f"wave_ingest: {len(rows)} rows (1 .. {WAVE_JOIN_MAX_ROWS})")
    dev, fb = rows[0].device, channels * WAVE_IN_SAMPLE_BYTES[enc]
    frames = []
    for r, w in enumerate(rows):
        if w.dtype not in _WAVE_IN_DTYPES or _WAVE_IN_DTYPES[w.dtype] not in (None, enc):
            raise TypeError(f"wave_ingest: row {r} of dtype {w.dtype} cannot hold the encoding {enc!r}")
        if w.dim() != 1 or (w.numel() > 1 and w.stride(0) != 1) or w.device != dev:
            raise ValueError(f"wave_ingest: row {r} is not a 1-D tensor with unit stride on {dev}")
        nbytes = w.numel() * w.element_size()
        if nbytes % fb:
            raise ValueError(f"wave_ingest: row {r}: {nbytes} bytes are not a whole number of frames of {fb} bytes")
        frames.append(nbytes // fb)
    base = rows[0].untyped_storage().data_ptr()
    if any(w.untyped_storage().data_ptr() != base for w in rows):
        raise ValueError("wave_ingest: the rows are views of different allocations; pass views of one buffer")
    R = len(rows)
    offs = (ctypes.c_long * R)(*[w.data_ptr() - base if w.numel() else 0 for w in rows])
    return base, offs, (ctypes.c_long * R)(*frames), frames


def wave_ingest(rows, encoding, channels, rate_in, rate_out):
    """cbx_wave_ingest on the current stream: rows (_ingest_rows: 1 .. 64 1-D views of ONE allocation holding interleaved frames of `channels` samples in
    `encoding`, sampled at rate_in) decoded, mixed down to mono and resampled to rate_out in ONE launch.  Returns R 1-D fp32 tensors (row r has
    resampled_len(frames_r, rate_in, rate_out) samples) that are views of one packed device buffer.  No host synchronisation.  ValueError / TypeError before the
    launch: an unknown encoding, channels outside [1, 8], a pair of rates over the caps (resample_filter), rows that are not whole frames."""
    if encoding not in WAVE_IN_ENCODINGS:
        raise ValueError(f"wave_ingest: encoding = {encoding!r}: expected one of {WAVE_IN_ENCODINGS}")
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= WAVE_IN_MAX_CHANNELS:
        raise ValueError(f"wave_ingest: channels = {channels!r}: expected an int in 1 .. {WAVE_IN_MAX_CHANNELS}")
    f = resample_filter(rate_in, rate_out)
    rows = list(rows)
    if _all_empty(rows):
        return [torch.empty(0, dtype=torch.float32, device=w.device) for w in rows]
    base, offs, nfr, frames = _ingest_rows(rows, encoding, channels)
    R, dev = len(frames), rows[0].device
    cnt = [-(-n * f["U"] // f["D"]) for n in frames]
    starts = [sum(cnt[:r]) for r in range(R)]
    packed = torch.empty(max(1, sum(cnt)), dtype=torch.float32, device=dev)
    o = (ctypes.c_long * R)(*starts)
    check(lib.cbx_wave_ingest(base, ctypes.addressof(offs), ctypes.addressof(nfr), R, WAVE_IN_ENCODINGS.index(encoding), channels,
                              _p(_resample_table(rate_in, rate_out, dev)) if f["hl"] else None, f["U"], f["D"], f["T"], _p(packed), ctypes.addressof(o), packed.numel(),
                              _stream()), "cbx_wave_ingest")
    return [packed[a: a + c] for a, c in zip(starts, cnt)]


def wave_trim_edges(rows, top_db=20.0, edges=None):
    """cbx_wave_trim_edges_f32 on the current stream: the part {start, stop} of every row (_wave_rows) that frontend.trim_silence keeps, as an (R, 2) int32 device
    tensor.  Two launches, no host synchronisation."""
    base, offs, lens = _wave_rows(rows, "wave_trim_edges")
    R, dev = len(lens), rows[0].device
    if edges is None:
        edges = torch.empty(R, 2, dtype=torch.int32, device=dev)
    assert edges.dtype == torch.int32 and edges.numel() == 2 * R and edges.is_contiguous() and edges.device == dev, "wave_trim_edges: edges is (R, 2) int32 on the rows' device"
    ws = torch.empty(max(1, R * -(-max(lens) // 512)), dtype=torch.float64, device=dev)
    check(lib.cbx_wave_trim_edges_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), R, 10.0 ** (-float(top_db) / 10.0), _p(edges), _p(ws), ws.numel(), _stream()),
          "cbx_wave_trim_edges_f32")
    return edges


def hift_stft(s, spec, sample_lens=None):
    B, L = s.shape
    check(lib.cbx_hift_stft_f32(_p(s), _p(spec), _p(sample_lens), B, L, spec.stride(1), _stream()), "cbx_hift_stft_f32")
    return spec


def hift_istft(x, wav, clamp=0.99, fade_n=0, frame_lens=None):
    """x (B, frames, ld >= 18) -> wav (B, 4 (frames - 1)).  frame_lens (B,) int32 on x's device: row b owns frame_lens[b] frames; its samples equal the
    batch-1 launch on the cut row, everything beyond them is 0 (include/cbx.h cbx_hift_istft_rows_f32)."""
    B, frames = x.shape[0], x.shape[1]
    if frame_lens is None:
        check(lib.cbx_hift_istft_f32(_p(x), _p(wav), B, frames, x.stride(1), clamp, fade_n, _stream()), "cbx_hift_istft_f32")
        return wav
    assert frame_lens.dtype == torch.int32 and frame_lens.numel() == B and frame_lens.is_contiguous() and frame_lens.device == x.device, "hift_istft: frame_lens is (B,) int32 on x's device"
    check(lib.cbx_hift_istft_rows_f32(_p(x), _p(wav), _p(frame_lens), B, frames, x.stride(1), clamp, fade_n, _stream()), "cbx_hift_istft_rows_f32")
    return wav


# ----------------------------------------------------------------------------- front-end (prompt analysis / voice conversion) kernels

UN_LOG_CLAMP, UN_LOG10_CLAMP, UN_FLOOR_AFFINE, UN_AFFINE = 1, 2, 3, 4


def dwconv1d(x, w, y, taps, pad_left, lens=None, add_input=False):
    """Depthwise conv, channel-last: x, y (B, T, C); w (C, taps)."""
    B, T, C = x.shape
    check(lib.cbx_dwconv1d_f32(_p(_f32(x, "x")), _p(_f32(w, "w")), _p(y), _p(lens), B, T, C, taps, pad_left, x.stride(1), y.stride(1),
                               x.stride(0), y.stride(0), int(add_input), _stream()), "cbx_dwconv1d_f32")
    return y


def lstm_cell(pre, hh, c, h):
    B, H = c.shape
    check(lib.cbx_lstm_cell_f32(_p(pre), _p(hh), _p(c), _p(h), B, H, pre.stride(0), hh.stride(0), c.stride(0), h.stride(0), _stream()),
          "cbx_lstm_cell_f32")


def affine_act(x, y, scale, shift, act=NONE):
    rows, C = x.shape
    check(lib.cbx_affine_act_f32(_p(_f32(x, "x")), _p(y), _p(scale), _p(shift), rows, C, x.stride(0), y.stride(0), act, _stream()),
          "cbx_affine_act_f32")
    return y


def cplx_power(spec, out, mode=0, eps=0.0):
    rows, F = out.shape
    check(lib.cbx_cplx_power_f32(_p(_f32(spec, "spec")), _p(out), rows, F, spec.stride(0), out.stride(0), mode, eps, _stream()),
          "cbx_cplx_power_f32")
    return out


def unary(x, y, op, a=0.0, b=0.0, dev_scalar=None):
    rows, C = x.shape
    check(lib.cbx_unary_f32(_p(_f32(x, "x")), _p(y), rows, C, x.stride(0), y.stride(0), op, a, b, _p(dev_scalar), _stream()), "cbx_unary_f32")
    return y


def reduce_max(x, out):
    rows, C = x.shape
    check(lib.cbx_reduce_max_f32(_p(_f32(x, "x")), _p(out), rows, C, x.stride(0), _stream()), "cbx_reduce_max_f32")
    return out


def seg_context(x, ctx, seg_len=100):
    T, C = x.shape
    check(lib.cbx_seg_context_f32(_p(_f32(x, "x")), _p(ctx), T, C, seg_len, x.stride(0), ctx.stride(0), _stream()), "cbx_seg_context_f32")
    return ctx


def seg_gate_mul(y, m, seg_len=100):
    T, C = y.shape
    check(lib.cbx_seg_gate_mul_f32(_p(y), _p(m), T, C, seg_len, y.stride(0), m.stride(0), _stream()), "cbx_seg_gate_mul_f32")
    return y


def stats_pool(x, out):
    T, C = x.shape
    check(lib.cbx_stats_pool_f32(_p(_f32(x, "x")), _p(out), T, C, x.stride(0), _stream()), "cbx_stats_pool_f32")
    return out


def fsq_index(h, idx):
    check(lib.cbx_fsq_index(_p(_f32(h, "h")), _p(idx), h.shape[0], h.stride(0), _stream()), "cbx_fsq_index")
    return idx
