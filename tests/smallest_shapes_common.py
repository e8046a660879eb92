"""Shared bodies of tests/test_smallest_shapes_gpu.py (-m gpu) and of the SIMT emulator's reduced matrix (tests/test_simt_kernels.py, _SMALLSHAPE): the software-
pipelined kernels at the SMALLEST shapes they accept -- K walks shorter than the LDS ring (1, 2, 3 K tiles against 2 - 4 stages and against the four K tiles the
deferred epilogue rides on), a single part-filled tile, fewer tiles than workgroups, key sequences shorter than a KV tile and not a multiple of 8.  Every body takes
`dev` first (a CUDA device, or the CPU under the emulator).

Rules of every comparison (_cmp):
  * reference: fp64 on the values the operands hold (_planes_exact for plane operands, the fp32 values for fp32 operands);
  * outputs are NaN-prefilled VIEWS into larger NaN-filled buffers (guard rows and columns on every side) which must still be all-NaN afterwards; operands are views
    into NaN-filled buffers as well: a load outside an operand view, or a store outside an output view, shows;
  * NaN is a failure: bad = ~(err <= lim).
Tolerances are the neighbours' (tests/test_planes_gpu.py, tests/test_ops_gpu.py), nothing new: plane GEMM 3e-5 max(1, sqrt(K / 256)) (1 + |ref|), plane attention 2e-5,
LayerNorm epilogue 3e-6, split GEMM _SPLIT_TOL[prec], exact GEMM 3e-5 (all in the form tol (1 + |ref|)).

Every comparison prints `SMALLSHAPE <kernel> <form> <MxNxK | T> <max err> (tol ...)` before it asserts; every plane-GEMM body prints one
`SMALLSHAPE-COVER <kernel> form <f> persist <p>: (nk, tiles per workgroup) ...` line: the K-walk lengths and tile walks that form really ran (a form that needs
Cin % 64 == 0 is NOT run where the dispatcher would fall through to its automatic choice: the fall-through is form 0's business).  profiles/smallest_shapes_tests.log
keeps the lines of the emulator run and of the MI355X run.
"""
import functools
import math

import torch
import torch.nn.functional as F

NAN = float("nan")
G_ROWS, G_COLS = 2, 8  # guard rows / columns (8 halves = 16 bytes, 8 floats = 32 bytes: operand views keep the alignment the kernels require)

# the tile menu of gemm_planes.hip (cbx_gemm_planes, `switch (force)`): form -> (BM, BN, BK, LDS stages, loader waves)
FORMS = {1: (128, 64, 32, 2, 0), 2: (128, 64, 32, 2, 0), 3: (128, 128, 32, 2, 0), 4: (128, 128, 32, 2, 0), 5: (128, 64, 64, 2, 0), 6: (128, 64, 64, 2, 0),
         7: (128, 128, 64, 2, 0), 8: (128, 128, 64, 2, 0), 9: (64, 64, 32, 2, 0), 10: (256, 64, 32, 2, 0), 11: (256, 128, 32, 2, 0), 12: (128, 128, 32, 3, 0),
         13: (128, 64, 32, 3, 0), 14: (128, 128, 32, 2, 0), 15: (128, 256, 32, 2, 0), 16: (64, 128, 32, 2, 0), 17: (128, 128, 32, 3, 0), 18: (256, 128, 32, 3, 0),
         19: (128, 256, 32, 3, 0), 21: (128, 128, 64, 2, 1), 22: (128, 128, 32, 3, 1), 23: (256, 128, 32, 3, 1), 24: (128, 128, 32, 2, 1), 25: (128, 128, 32, 4, 1),
         26: (256, 128, 32, 2, 0), 27: (256, 128, 32, 3, 0), 28: (128, 256, 32, 2, 0), 31: (128, 128, 64, 2, 2), 32: (128, 128, 64, 2, 4), 33: (128, 128, 32, 3, 4),
         34: (128, 128, 32, 4, 4), 35: (128, 128, 64, 2, 4), 36: (256, 128, 32, 3, 4), 37: (128, 128, 32, 4, 2), 41: (128, 128, 64, 2, 4), 42: (128, 128, 64, 2, 4),
         43: (64, 64, 32, 3, 0), 44: (64, 64, 64, 2, 0), 45: (64, 64, 64, 3, 0)}
LN_FORM = (64, 256, 32, 3, 0)  # the row-spanning form of the LayerNorm epilogue

LINEAR_SHAPES = ((1, 2, 32), (2, 66, 64), (31, 62, 96), (65, 130, 128), (300, 258, 192))  # nk = 1, 2, 3, 4, 6 at BK = 32; 1, 2, 3 at BK = 64
DF_KS = (64, 128, 192)                                                                     # nk = 1, 2, 3 < the PKT = 4 K tiles the deferred quads ride on
LN_KS, LN_MS = (32, 64, 96), (1, 63, 64, 65, 130)
CONV_FORMS, CONV_TS, CONV_CINS = (0, 2, 9, 12, 21, 33, 43), (1, 2, 3), (32, 64)
PT_FORMS, PT_MS, PT_KS = (0, 4, 9, 14, 21), (4, 8), (32, 64)
ATTN_TS = (1, 2, 7, 8, 9, 63, 65, 127, 129, 191, 193)
F32_P1_M, F32_P1_N, F32_P1_K = (1, 32, 33), (1, 63, 65), (4, 8, 20, 36, 16, 48, 80)
F32_SPLIT_M, F32_SPLIT_N, F32_SPLIT_K = (33, 129), (2, 65), (32, 64, 96, 4, 36)
SPLIT_TOL = {6: 3e-5, 16: 3e-5, 3: 1e-4}  # tests/test_ops_gpu.py::_SPLIT_TOL


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _planes_exact(x):
    """What a planes tensor holds for fp32 x: h + l / 2048 in fp64 (tests/test_planes_gpu.py)."""
    h = x.half()
    l = ((x.double() - h.double()) * 2048.0).half()
    return h.double() + l.double() / 2048.0


def _cmp(kernel, form, shape, got, ref, tol, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (kernel, form, shape, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= tol * (1.0 + ref.abs()))  # NaN is a failure
    worst = float(torch.nan_to_num(err, nan=math.inf).max()) if err.numel() else 0.0
    print(f"SMALLSHAPE {kernel} {form} {shape} {worst:.3e} (tol {tol:g}, ref max {float(ref.abs().max()) if ref.numel() else 0.0:.3e}){' ' + what if what else ''}")
    assert not bad.any(), (f"{kernel} {form} {shape} {what}: max err {worst:.3e}, {int(bad.sum())} / {bad.numel()} over tol {tol}, "
                           f"{int((~torch.isfinite(got)).sum())} non-finite in the output")


# ------------------------------------------------------------------------------------------------ NaN-guarded operands and outputs

class GuardedPlanes:
    """A Planes view (rows, C) inside a NaN-filled fp16 tensor: G_ROWS rows above and below, G_COLS columns left and right of BOTH planes."""

    def __init__(self, dev, rows, C, x=None, zero=False, gc=G_COLS):
        from chatterbox_amd import ops
        self.rows, self.C, self.gc = rows, C, gc
        self.big = torch.full((rows + 2 * G_ROWS, 2 * (C + 2 * gc)), NAN, dtype=torch.float16, device=dev)
        self.p = ops.Planes(0, 0, None, t=self.big[G_ROWS:G_ROWS + rows], c0=gc, width=C)
        if x is not None:
            assert tuple(x.shape) == (rows, C)
            ops.split_planes(x.contiguous().to(dev), self.p)
        elif zero:
            for c in self._ranges():
                self.big[G_ROWS:G_ROWS + rows, c:c + C] = 0

    def _ranges(self):
        return (self.gc, self.big.shape[1] // 2 + self.gc)

    def intact(self):
        """Everything outside the view is still NaN."""
        m = torch.ones_like(self.big, dtype=torch.bool)
        for c in self._ranges():
            m[G_ROWS:G_ROWS + self.rows, c:c + self.C] = False
        return bool(torch.isnan(self.big[m]).all())

    def float(self):
        return self.p.float()


def _f32_guarded(dev, x=None, shape=None, gc=G_COLS):
    """(big, view): a (..., R, C) fp32 view inside a NaN-filled tensor with G_ROWS / gc guard rows / columns; x = its contents (NaN where None)."""
    shape = tuple(x.shape if x is not None else shape)
    big = torch.full(shape[:-2] + (shape[-2] + 2 * G_ROWS, shape[-1] + 2 * gc), NAN, device=dev)
    view = big[..., G_ROWS:G_ROWS + shape[-2], gc:gc + shape[-1]]
    if x is not None:
        view.copy_(x.to(dev))
    return big, view


def _f32_intact(big, view_shape, gc=G_COLS):
    m = torch.ones_like(big, dtype=torch.bool)
    m[..., G_ROWS:G_ROWS + view_shape[-2], gc:gc + view_shape[-1]] = False
    return bool(torch.isnan(big[m]).all())


class _geometry:
    """cbx_set_planes_persist for the duration (0: one tile per workgroup, n > 1: exactly n workgroups) + the tile form per call."""

    def __init__(self, tile, persist):
        self.tile, self.persist = tile, persist

    def __enter__(self):
        from chatterbox_amd import ops
        ops.lib.cbx_set_planes_persist(self.persist)
        self.scope = ops.planes_geometry(tile=self.tile)
        self.scope.__enter__()

    def __exit__(self, *a):
        from chatterbox_amd import ops
        self.scope.__exit__(*a)
        ops.lib.cbx_set_planes_persist(1)


def runs_own_kernel(tile, cin):
    """Does cbx_gemm_planes run form `tile` itself at this Cin?  (the 64-wide K tiles need Cin % 64 == 0: otherwise the call falls through to the automatic choice)"""
    return tile == 0 or FORMS[tile][2] == 32 or cin % 64 == 0


def walk(form, M, N, K, persist, nz=1, cin=None):
    """(form that runs, nk, tiles per workgroup of the busiest workgroup) -- mirrors launch_pl_act's grid and, for form 0, the dispatcher's choice for small grids
    ((M / 128) (N / 128) nz < 64, true of every shape here: 64 x 64 tiles, 64-wide K tiles where Cin % 64 == 0)."""
    cin = cin or K
    if form == 0:
        assert (M + 127) // 128 * ((N + 127) // 128) * nz < 64
        form = 44 if cin % 64 == 0 else 9
    BM, BN, BK = (LN_FORM if form == "ln" else FORMS[form])[:3]
    total = (M + BM - 1) // BM * ((N + BN - 1) // BN) * nz
    grid = min(total, persist) if persist > 1 else total
    return form, K // BK, (total + grid - 1) // grid


def _cover_line(kernel, tile, persist, ran):
    print(f"SMALLSHAPE-COVER {kernel} form {tile} persist {persist}: (nk, tiles per workgroup) = " + " ".join(f"({a},{b})" for a, b in sorted(set(ran))))


# ------------------------------------------------------------------------------------------------ 1. plane GEMM

@functools.lru_cache(maxsize=None)
def _linear_case(M, N, K):
    x, w, b, r = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3), _r((M, N), 4)
    return x, w, b, r, F.linear(_planes_exact(x), _planes_exact(w), b.double())


def check_linear_tile(dev, tile, persist, shapes=LINEAR_SHAPES):
    """One tile form on every Linear shape: bias + in-place residual to fp32 | GELU to planes | both at once."""
    from chatterbox_amd import ops
    ran = []
    with _geometry(tile, persist):
        for (M, N, K) in shapes:
            if not runs_own_kernel(tile, K):
                continue
            form, nk, tpw = walk(tile, M, N, K, persist)
            ran.append((nk, tpw))
            x, w, b, r, ref0 = _linear_case(M, N, K)
            xP, wP, bd = GuardedPlanes(dev, M, K, x), GuardedPlanes(dev, N, K, w), b.to(dev)
            tol = 3e-5 * max(1.0, math.sqrt(K / 256))
            shp, frm = f"{M}x{N}x{K}", f"tile{tile}/p{persist}"
            # bias + in-place residual -> fp32
            big, out = _f32_guarded(dev, r)
            ops.linear_planes(xP.p, wP.p, out=out, bias=bd, residual=out)
            _cmp("gemm_planes", frm, shp, out, ref0 + r.double(), tol, "bias+residual->fp32")
            assert _f32_intact(big, (M, N)), f"{frm} {shp}: a store outside the fp32 output view"
            # GELU -> planes
            oP = GuardedPlanes(dev, M, N)
            ops.linear_planes(xP.p, wP.p, outp=oP.p, bias=bd, act=ops.GELU_ERF)
            _cmp("gemm_planes", frm, shp, oP.float(), F.gelu(ref0), tol, "gelu->planes")
            assert oP.intact(), f"{frm} {shp}: a store outside the plane output view"
            # both at once
            big, out = _f32_guarded(dev, r)
            oP = GuardedPlanes(dev, M, N)
            ops.linear_planes(xP.p, wP.p, out=out, outp=oP.p, bias=bd, act=ops.GELU_ERF, residual=out)
            ref = F.gelu(ref0) + r.double()
            _cmp("gemm_planes", frm, shp, out, ref, tol, "gelu+residual->fp32 (both)")
            _cmp("gemm_planes", frm, shp, oP.float(), ref, tol, "gelu+residual->planes (both)")
            assert bool(((oP.float() - out).abs() <= 2.0 ** -21 * out.abs().max()).all()), "plane output = split of the fp32 output"
            assert _f32_intact(big, (M, N)) and oP.intact(), f"{frm} {shp}: a store outside an output view"
            assert xP.intact() and wP.intact()
    _cover_line("gemm_planes", tile, persist, ran)
    return ran


def check_deferred_epilogue(dev, tile, plain, persist, M, N, Ks=DF_KS):
    """Forms 41 / 42 against their plain twins 32 / 35 BIT FOR BIT on K walks of 1 .. 3 K tiles (the `nk < PKT` arm: quads without a K tile to ride on), both df_kinds:
    plane output only (df_kind 1), fp32 output with and without an in-place residual (df_kind 2); each also against fp64."""
    from chatterbox_amd import ops
    ran = []
    for K in Ks:
        _, nk, tpw = walk(tile, M, N, K, persist)
        ran.append((nk, tpw))
        x, w, b, r, ref0 = _linear_case(M, N, K)
        xP, wP, bd = GuardedPlanes(dev, M, K, x), GuardedPlanes(dev, N, K, w), b.to(dev)
        shp = f"{M}x{N}x{K}"
        ops.lib.cbx_set_planes_persist(persist)
        try:
            for act, fn in ((ops.NONE, lambda t: t), (ops.GELU_ERF, F.gelu)):
                got, want = GuardedPlanes(dev, M, N), GuardedPlanes(dev, M, N)
                ops.gemm_planes(xP.p, wP.p, M=M, N=N, K=K, P=got.p, bias=bd, act=act, tile=tile)
                ops.gemm_planes(xP.p, wP.p, M=M, N=N, K=K, P=want.p, bias=bd, act=act, tile=plain)
                _cmp("gemm_planes_df1", f"tile{tile}/p{persist}", shp, got.float(), fn(ref0), 3e-5, f"act {act} ->planes")
                assert got.intact() and want.intact(), f"tile {tile} {shp}: a store outside the plane output view"
                assert torch.equal(got.float(), want.float()) and torch.equal(torch.nan_to_num(got.big, nan=7.0), torch.nan_to_num(want.big, nan=7.0)), \
                    f"planes, tile {tile} vs {plain}, {shp} act {act}: not bit-identical"
            for res in (False, True):
                outs = []
                for t in (tile, plain):
                    big, out = _f32_guarded(dev, r if res else None, (M, N))
                    ops.gemm_planes(xP.p, wP.p, M=M, N=N, K=K, C=out, ldc=out.stride(0), R=out if res else None, ldr=out.stride(0) if res else 0, bias=bd, tile=t)
                    assert _f32_intact(big, (M, N)), f"tile {t} {shp}: a store outside the fp32 output view"
                    outs.append(out)
                _cmp("gemm_planes_df2", f"tile{tile}/p{persist}", shp, outs[0], ref0 + (r.double() if res else 0), 3e-5, f"residual {int(res)} ->fp32")
                assert torch.equal(outs[0], outs[1]), f"fp32 out, tile {tile} vs {plain}, {shp} residual {res}: not bit-identical"
        finally:
            ops.lib.cbx_set_planes_persist(1)
    _cover_line("gemm_planes_df", tile, persist, ran)
    return ran


@functools.lru_cache(maxsize=None)
def _ln_case(M, K):
    N = 256
    x, w, b = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3)
    r = _r((M, N), 4) * 3.0 + 0.5  # a residual stream with a non-zero row mean
    lw, lb = 1 + 0.1 * _r((N,), 5), 0.1 * _r((N,), 6)
    return x, w, b, r, lw, lb, F.linear(_planes_exact(x), _planes_exact(w), b.double())


def check_layernorm_epilogue(dev, K, persist, Ms=LN_MS):
    """The 64 x 256 x 32 three-stage form with the LayerNorm epilogue on K walks of 1 .. 3 K tiles (shorter than or equal to its ring), M from one row up:
    against fp64, and against the two launches it replaces (fp32 row bit-identical; LayerNorm at tests/test_planes_gpu.py::test_gemm_planes_layernorm_epilogue's tolerances)."""
    from chatterbox_amd import ops
    N, ran = 256, []
    ops.lib.cbx_set_planes_persist(persist)
    try:
        for M in Ms:
            _, nk, tpw = walk("ln", M, N, K, persist)
            ran.append((nk, tpw))
            x, w, b, r, lw, lb, ref0 = _ln_case(M, K)
            xP, wP = GuardedPlanes(dev, M, K, x), GuardedPlanes(dev, N, K, w)
            for res in (False, True):
                shp, frm = f"{M}x{N}x{K}", f"ln64x256/p{persist}/res{int(res)}"
                big, out = _f32_guarded(dev, r if res else None, (M, N))
                lnP = GuardedPlanes(dev, M, N)
                ops.linear_planes(xP.p, wP.p, out=out, bias=b.to(dev), residual=out if res else None, ln=(lw.to(dev), lb.to(dev)), lnp=lnP.p)
                _cmp("gemm_planes_ln", frm, shp, out, ref0 + (r.double() if res else 0), 3e-5, "fp32 row")
                ln_ref = F.layer_norm(out.double().cpu(), (N,), lw.double(), lb.double(), 1e-5)
                _cmp("gemm_planes_ln", frm, shp, lnP.float(), ln_ref, 3e-6, "LayerNorm planes")
                assert _f32_intact(big, (M, N)) and lnP.intact(), f"{frm} {shp}: a store outside an output view"
                # the two launches it replaces
                big2, out2 = _f32_guarded(dev, r if res else None, (M, N))
                ops.linear_planes(xP.p, wP.p, out=out2, bias=b.to(dev), residual=out2 if res else None)
                assert torch.equal(out2, out), f"{frm} {shp}: the fp32 row must not depend on the tile form"
                ln2 = GuardedPlanes(dev, M, N)
                ops.layernorm_planes(out2, lw.to(dev), lb.to(dev), ln2.p, 1e-5)
                d = (ln2.float() - lnP.float()).abs().max()
                print(f"SMALLSHAPE gemm_planes_ln {frm} {shp} {float(d):.3e} (tol 4e-06 absolute) vs layernorm_planes")
                assert bool(d <= 4e-6), f"{frm} {shp} vs layernorm_planes: {float(d):.3e}"
                assert _f32_intact(big2, (M, N)) and ln2.intact() and xP.intact() and wP.intact()
    finally:
        ops.lib.cbx_set_planes_persist(1)
    _cover_line("gemm_planes_ln", "ln64x256", persist, ran)
    return ran


@functools.lru_cache(maxsize=None)
def _conv_case(T, cin, masked):
    B, N = 3, 130
    x, w, b = _r((B, T, cin), 1), _r((N, cin, 3), 2, 1 / math.sqrt(3 * cin)), _r((N,), 3)
    lens = [T, 1, 0] if masked else None
    xm = x.clone()
    if masked:
        for z in range(B):
            xm[z, lens[z]:] = 0
    ref = F.conv1d(F.pad(_planes_exact(xm).transpose(1, 2), (2, 0)), _planes_exact(w), b.double()).transpose(1, 2)
    return x, w, b, lens, ref


def check_conv_tile(dev, tile, persist, cins=CONV_CINS, Ts=CONV_TS):
    """Causal 3-tap Conv1d on planes, T = 1 .. 3: taps wholly in the left padding, every K tile (Cin = 32) or every second one (Cin = 64 at BK = 32) starts a new tap;
    B = 3, lens None / [T, 1, 0] with the input rows at and beyond lens[z] set to NaN (they must read as zero)."""
    from chatterbox_amd import ops
    B, N, ran = 3, 130, []
    with _geometry(tile, persist):
        for cin in cins:
            if not runs_own_kernel(tile, cin):
                continue
            for T in Ts:
                _, nk, tpw = walk(tile, T, N, 3 * cin, persist, nz=B, cin=cin)
                ran.append((nk, tpw))
                for masked in (False, True):
                    x, w, b, lens, ref = _conv_case(T, cin, masked)
                    xin = x.clone()
                    if masked:
                        for z in range(B):
                            xin[z, lens[z]:] = NAN  # rows >= lens[z] read as zero whatever they hold
                    wp = w.permute(0, 2, 1).reshape(N, 3 * cin).contiguous()  # tap-major packing (weights.pack_conv)
                    xP, wP = GuardedPlanes(dev, B * T, cin, xin.reshape(B * T, cin)), GuardedPlanes(dev, N, 3 * cin, wp)
                    big, out = _f32_guarded(dev, None, (B, T, N))
                    oP = GuardedPlanes(dev, B * T, N)
                    ops.conv1d_planes(xP.p, wP.p, B=B, T=T, taps=3, cin=cin, out=out, outp=oP.p, bias=b.to(dev), pad_left=2,
                                      lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev))
                    shp, frm = f"{B}x{T}x{N}x{3 * cin}", f"tile{tile}/p{persist}/lens{int(masked)}"
                    _cmp("gemm_planes_conv", frm, shp, out, ref, 3e-5, "->fp32")
                    _cmp("gemm_planes_conv", frm, shp, oP.float().view(B, T, N), ref, 3e-5, "->planes")
                    assert _f32_intact(big, (T, N)) and oP.intact() and xP.intact() and wP.intact(), f"{frm} {shp}: a store outside an output view"
    _cover_line("gemm_planes_conv", tile, persist, ran)
    return ran


@functools.lru_cache(maxsize=None)
def _pt_case(M, K):
    N = 320
    h, w = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K))
    return h, w, F.linear(_planes_exact(h), _planes_exact(w))


def check_transposed_tile(dev, tile, persist, Ms=PT_MS, Ks=PT_KS):
    """q | k | V^T from one launch at the smallest legal shape: pt_T = 4 (one V^T row holds 4 keys + 4 zero pad keys), pt_n0 = 256, one and two groups."""
    from chatterbox_amd import ops
    N, n0, T, Tp, ran = 320, 256, 4, 8, []
    with _geometry(tile, persist):
        for K in Ks:
            if not runs_own_kernel(tile, K):
                continue
            for M in Ms:
                Z = M // T
                _, nk, tpw = walk(tile, M, N, K, persist)
                ran.append((nk, tpw))
                h, w, ref = _pt_case(M, K)
                hP, wP = GuardedPlanes(dev, M, K, h), GuardedPlanes(dev, N, K, w)
                qk, vt = GuardedPlanes(dev, M, n0), GuardedPlanes(dev, Z * 64, Tp, zero=True)
                ops.gemm_planes(hP.p, wP.p, M=M, N=N, K=K, P=qk.p, PT=vt.p, pt_n0=n0, pt_T=T, pt_zs=64 * vt.p.ld)
                shp, frm = f"{M}x{N}x{K}", f"tile{tile}/p{persist}"
                _cmp("gemm_planes_pt", frm, shp, qk.float(), ref[:, :n0], 3e-5, "q|k columns")
                got = vt.float().view(Z, 64, Tp)
                _cmp("gemm_planes_pt", frm, shp, got[:, :, :T], ref[:, n0:].view(Z, T, 64).transpose(1, 2), 3e-5, "V^T")
                assert float(got[:, :, T:].abs().max()) == 0.0, f"{frm} {shp}: pad keys of V^T stay zero"
                assert qk.intact() and vt.intact() and hP.intact() and wP.intact(), f"{frm} {shp}: a store outside an output view"
    _cover_line("gemm_planes_pt", tile, persist, ran)
    return ran


# ------------------------------------------------------------------------------------------------ 2. plane attention

@functools.lru_cache(maxsize=None)
def _attn_case(T, masked):
    Z, H = 3, 2
    q, k, v = _r((Z, T, H, 64), 1) * 1.5, _r((Z, T, H, 64), 2) * 1.5, _r((Z, T, H, 64), 3)
    lens = [T, 1, 0] if masked else None
    s = torch.einsum("zqhd,zkhd->zhqk", _planes_exact(q), _planes_exact(k)) * 0.125
    if masked:
        for z, n in enumerate(lens):
            s[z, :, :, n:] = -math.inf
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)  # an utterance without a key: zeros (tests/test_softmax_stress_gpu.py's convention)
    return q, k, v, lens, torch.einsum("zhqk,zkhd->zqhd", p, _planes_exact(v)).reshape(Z * T, H * 64)


def check_attention(dev, version, Ts=ATTN_TS):
    """T below one KV tile, not a multiple of 8 (V^T rows padded to 8 keys, the pad ZERO as the interface requires), two and three KV tiles against the three-stage ring
    of versions 2 .. 6; key_lens None / [T, 1, 0] (an all-masked utterance gives zeros); q and k are column ranges of one planes tensor; everything else is NaN."""
    from chatterbox_amd import ops
    Z, H, D = 3, 2, 128
    for T in Ts:
        Tp = (T + 7) // 8 * 8
        for masked in (False, True):
            q, k, v, lens, ref = _attn_case(T, masked)
            qk = GuardedPlanes(dev, Z * T, 2 * D)
            ops.split_planes(q.reshape(Z * T, D).to(dev), qk.p.cols(0, D))
            ops.split_planes(k.reshape(Z * T, D).to(dev), qk.p.cols(D, D))
            vtt = torch.zeros(Z, D, Tp)
            vtt[:, :, :T] = v.reshape(Z, T, D).transpose(1, 2)
            # V^T: guard ROWS only -- the interface wants the tail of a V^T row finite (the 64-key tiles of versions 2 .. 6 read on past the pad into the row's
            # second plane), so the row stride is exactly [h | l] of Tp keys
            vt = GuardedPlanes(dev, Z * D, Tp, vtt.reshape(Z * D, Tp), gc=0)
            out = GuardedPlanes(dev, Z * T, D)
            kl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
            ops.flash_attn_planes(qk.p.cols(0, D), qk.p.cols(D, D), vt.p, out.p, Z=Z, H=H, T=T, vt_sb=D * vt.p.ld, scale=0.125, key_lens=kl, version=version)
            _cmp("flash_attn_planes", f"v{version}/lens{int(masked)}", f"T{T}", out.float(), ref, 2e-5)
            assert out.intact() and qk.intact() and vt.intact(), f"version {version} T {T}: a store outside the output view"
            if masked:
                assert float(out.float().view(Z, T, D)[2].abs().max()) == 0.0, f"version {version} T {T}: an utterance without a key gives zeros"


# ------------------------------------------------------------------------------------------------ 3. fp32-operand GEMMs (gemm_f32.hip, gemm_split.hip)

@functools.lru_cache(maxsize=None)
def _f32_case(M, N, K):
    x, w, b, r = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3), _r((M, N), 4)
    return x, w, b, r, F.silu(F.linear(x.double(), w.double(), b.double())) + r.double()


def _linear_guarded(dev, x, w, b, r, act, gc=G_COLS):
    """ops.linear on NaN-guarded strided views: bias + act + residual; returns (out view, guards intact)."""
    from chatterbox_amd import ops
    (bx, xv), (bw, wv), (br, rv) = _f32_guarded(dev, x, gc=gc), _f32_guarded(dev, w, gc=gc), _f32_guarded(dev, r, gc=gc)
    bo, out = _f32_guarded(dev, None, r.shape, gc=gc)
    ops.linear(xv, wv, out, bias=b.to(dev), act=act, residual=rv)
    return out, _f32_intact(bo, r.shape, gc) and _f32_intact(bx, x.shape, gc) and _f32_intact(bw, w.shape, gc) and _f32_intact(br, r.shape, gc)


def check_f32_linear(dev, prec, Ms, Ns, Ks):
    """Linear with bias + SiLU + residual.  precision 1: the skinny form (M <= 32), its last row count and the first of the 128 x 64 forms; K = 4, 8, 20, 36 on the
    generic loader (tail only, tail after full tiles), K = 16, 48, 80 on the buffer-load loader (an ODD number of K tiles: its two-ahead loop reads past the end).
    precision 3 / 6 / 16 (gemm_split.hip): K = 32, 64, 96 on the fast loader (1 .. 3 K tiles), K = 4, 36 on the generic one."""
    from chatterbox_amd import ops
    tol = 3e-5 if prec == 1 else SPLIT_TOL[prec]
    with ops.gemm_precision(prec):
        for M in Ms:
            for N in Ns:
                for K in Ks:
                    x, w, b, r, ref = _f32_case(M, N, K)
                    out, ok = _linear_guarded(dev, x, w, b, r, ops.SILU)
                    _cmp("gemm_f32" if prec == 1 or M <= 32 else "gemm_split", f"prec{prec}", f"{M}x{N}x{K}", out, ref, tol * max(1.0, math.sqrt(K / 256)))
                    assert ok, f"precision {prec} {M}x{N}x{K}: a store outside the output view"


def check_f32_layernorm_fold(dev):
    """LayerNorm folded into the A operand at the smallest shape ln_fusable admits (M = 33, K = 256), precision 16."""
    from chatterbox_amd import ops
    M, N, K = 33, 65, 256
    x, w, b = _r((M, K), 1) * 2.0 + 0.3, _r((N, K), 2, 1 / 16), _r((N,), 3)
    g, be = 1 + 0.1 * _r((K,), 4), 0.1 * _r((K,), 5)
    ref = F.linear(F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5), w.double(), b.double())
    (bx, xv), (bw, wv) = _f32_guarded(dev, x), _f32_guarded(dev, w)
    bo, out = _f32_guarded(dev, None, (M, N))
    stats = torch.empty(M, 2, device=dev)
    with ops.gemm_precision(16):
        assert ops.ln_fusable(M, K, xv.stride(0)) and not ops.ln_fusable(32, K, xv.stride(0))
        ops.row_stats(xv, stats)
        ops.linear(xv, wv, out, bias=b.to(dev), ln=(stats, g.to(dev), be.to(dev)))
    _cmp("gemm_split", "prec16/ln_fold", f"{M}x{N}x{K}", out, ref, SPLIT_TOL[16])
    assert _f32_intact(bo, (M, N)) and _f32_intact(bx, (M, K)) and _f32_intact(bw, (N, K))


# ------------------------------------------------------------------------------------------------ 4. the K % 4 contract of cbx_gemm_f32

def check_k_multiple_of_4_contract(dev, prec, M):
    """include/cbx.h: "K % 4 == 0, except with w_kn".  A Linear on strided views with K = 18, lda = ldw = 24 is REFUSED (its float4 tail would multiply columns 18
    and 19 of both operands in) and leaves the NaN-prefilled output untouched; K = 20 on the same views is right although columns 20 .. 23 hold NaN."""
    import pytest

    from chatterbox_amd import ops
    N = 5
    xb, wb, b = torch.full((M, 24), NAN), torch.full((N, 24), NAN), _r((N,), 3)
    xb[:, :20], wb[:, :20] = _r((M, 20), 1), _r((N, 20), 2, 0.25)
    xd, wd = xb.to(dev), wb.to(dev)
    with ops.gemm_precision(prec):
        out = torch.full((M, N), NAN, device=dev)
        with pytest.raises(RuntimeError, match="K % 4"):
            ops.linear(xd[:, :18], wd[:, :18], out, bias=b.to(dev))
        assert bool(torch.isnan(out).all()), "a refused call must not touch its output"
        ops.linear(xd[:, :20], wd[:, :20], out, bias=b.to(dev))
    _cmp("gemm_f32", f"prec{prec}/K20-of-24", f"{M}x{N}x20", out, F.linear(xb[:, :20].double(), wb[:, :20].double(), b.double()), 3e-5)
