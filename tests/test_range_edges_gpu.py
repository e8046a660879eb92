"""Both ends of the fp16 range in every f16x3 kernel (-m gpu; the same bodies run on the SIMT emulator, tests/test_simt_kernels.py).

S3Gen's default numerics (precision 16, "f16x3") carry every fp32 operand as two fp16 planes a = h + l / 2048.  A value beyond 65504 becomes inf in the h plane; the
only thing between that and garbage audio is the device range flag, of which every kernel that PRODUCES planes or splits fp32 operands on the fly carries its own
copy: gemm_planes.hip (plain plane epilogue, V^T store, LayerNorm epilogue, amax_df of the deferred-epilogue forms, split_planes_kernel), gemm_split.hip (one check
behind the K loop for three loaders and the LayerNorm fold), attention_split.hip (q after pre-scaling, k, v), norm.hip (the plane-output LayerNorm).  The other
suites draw operands from N(0, 1): no copy of the check but three is ever tripped there.  Here the operands are prescribed.

The guard's contract, asserted for EVERY launch of section 1 (_run + _verdict):
  C1  no silent overflow: either the flag word that was registered when the launch was enqueued is set, or every stored output element is within that kernel's
      existing parity tolerance of the fp64 reference -- plane GEMM 3e-5 max(1, sqrt(K / 256)) against fp64 on the values the planes hold (tests/test_planes_gpu.py),
      split GEMM _SPLIT_TOL[16] and attention 2e-5 (tests/test_ops_gpu.py), plane LayerNorm 2e-6 / 3e-6 (test_planes_gpu.py), all in the form tol (1 + |ref|);
      split_planes: the pair it stores is the pair the format defines (1e-12 absolute, test_planes_gpu.py).  After a trip the outputs may hold inf / NaN and are not
      compared;
  C2  must trip: a converted value with |v| >= 65536 trips the flag, +-inf included;
  C3  no false trip: if every value the kernel converts has |v| <= 61440 the flag stays clear (a false trip costs a discarded pass and a bf16x6 repeat); values
      between 61440 and 65536 may go either way.  A launch that converts nothing (fp32 output only) is held to C3 as well;
  C4  flag hygiene: reading clears the word, the OTHER word of the pair is never touched (launches alternate between word 0 and word 1), every test leaves both
      words clear and word 0 registered.

Construction: in-range seeded operands plus ONE prescribed outlier, every case with a twin that differs only in the outlier's size.
  * operand outlier (kernels that split fp32 operands): one element 7.0e4 (trip) or 6.0e4 (twin); q of the attention is checked AFTER its pre-scaling by
    scale log2(e) = 0.18034: 4.0e5 (72135 scaled) and 3.3e5 (59511 scaled);
  * output outlier (kernels that write planes from in-range operands): x[m, k0] = 256 and w[n, k0] = 320 (81920, exact in planes) or 224 (57344); with x ~ N(0, 1),
    w ~ N(0, 1 / sqrt(K)) the rest of row m stays near +-50 and the rest of column n near +-1300.  The reference asserts that exactly one output exceeds 65504 in the
    trip case and none exceeds 61440 in the twin (_outliers).  For the LayerNorm epilogue and layernorm_planes one column is driven out through ln_b[n] / post_add[n]
    = 7e4 (6e4), for the fp32 + plane output with an in-place residual through R[m, n];
  * post-activation: a -8e4 pre-activation under GELU / SILU stores (-)0: C1 only.
Positions: first element, last element of the ragged last tile in M and N, first row of the second row tile (row 64, 128 and 256: every tile height of the menu), an
even and an odd column, the last k of the last K tile.

Section 2, the lower end: below 2^-14 the h plane is an fp16 subnormal; gemm_split.hip promises "degrades gracefully (absolute precision 3e-11)".  Every tolerance of
the other suites has the form tol (1 + |ref|), vacuous for tiny outputs.  Here x is scaled by 2^e, e in {-10, -14, -17, -20, -23, -26} (from -17 down every h is
subnormal) with in-range w, one case with both operands small (2^-8 and 2^-12); reference fp64 on the original fp32 operands, per output element
    |err| <= 2^-22 sqrt(max(1, K / 256)) sum_k |x_k w_k|  +  2^-35 (sum_k |w_k| [+ sum_k |x_k| when both are small])
(22 significand bits + fp32 accumulation; a value below 2^-14 has a pair exact to 2^-36, the dropped l * l term adds at most 2^-37 per product).  An all-zero output
row fails; precision 6 runs the same inputs as a control against the first term alone; precision 16 must not trip on any of them.  The attention (v operand scaled)
has p = softmax in the x role, whose own error is the 2e-5 of the attention's parity test and not 2^-22: |err| <= 2e-5 sum_j p_j |v_j| + 2^-35 sum_j p_j -- the
neighbour's tolerance made scale-covariant (for v of order 1 it is below 2e-5 (1 + |ref|)).

Section 3, the engine: the alternating flag words of synthesize_pipelined on a real engine, a ragged batch of which one row is out of range, and streaming rounds
that are repeated at bf16x6 (a discarded f16x3 pass leaves no trace in the carried state).

Every comparison prints `RANGEEDGE <kernel> <case> tripped=<0|1> <max err> (tol ...)` before it asserts (profiles/range_edges_tests.log: the figures of the SIMT
emulator and of the MI355X).  All inputs are in bounds; tripped launches produce inf / NaN VALUES only.
"""
import functools
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TRIP, CLEAR = 65536.0, 61440.0
MNK = (333, 258, 256)
# (m, n, k0): first element | last element of the ragged last tile (last k of the last K tile) | first row of the second row tile for BM = 64 / 128 / 256, even and odd columns
POSITIONS = ((0, 0, 0), (332, 257, 255), (64, 130, 37), (128, 129, 255), (256, 2, 64))
LAST = POSITIONS[1]
SWEEP_TILES = (0, 3, 21, 26, 32, 35)  # the dispatcher's choice, a symmetric form, a loader-wave form, a 16-wave workgroup, four loader waves (32 x 64 and 64 x 32 per wave)
_LAUNCH = [0]


def _tiles():
    from test_planes_gpu import TILES
    return TILES


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _planes_exact(x):
    """What a planes tensor holds for fp32 x: h + l / 2048 in fp64 (tests/test_planes_gpu.py)."""
    h = x.half()
    l = ((x.double() - h.double()) * 2048.0).half()
    return h.double() + l.double() / 2048.0


def _reset(dev):
    """C4: both words clear, word 0 registered."""
    from chatterbox_amd import ops
    ops.enable_range_flag(dev)
    ops.select_range_flag(dev, 0)
    ops.range_flag_tripped(dev, 0)
    ops.range_flag_tripped(dev, 1)


def _run(dev, fn):
    """One launch under C4: registered into word `which` (alternating from launch to launch), both words clear before, the other word untouched after, reading clears.
    Returns whether the launch tripped its word."""
    from chatterbox_amd import ops
    which = _LAUNCH[0] & 1
    _LAUNCH[0] += 1
    ops.select_range_flag(dev, which)
    try:
        assert not ops.range_flag_tripped(dev, which) and not ops.range_flag_tripped(dev, 1 - which), "a flag word was left set by an earlier launch"
        fn()
        other = ops.range_flag_tripped(dev, 1 - which)
        hit = ops.range_flag_tripped(dev, which)
        again = ops.range_flag_tripped(dev, which)
    finally:
        ops.select_range_flag(dev, 0)
    assert not other, f"C4: the launch was enqueued under word {which} and touched word {1 - which}"
    assert not again, "C4: reading the flag must clear it"
    assert not ops.range_flag_tripped(dev), "C4: the registered word (0) is clear"
    return hit


def _verdict(kernel, case, tripped, pairs, expect, always=False):
    """pairs: (got, ref, tol[, "abs"]) per output (one RANGEEDGE line each); expect: "trip" (C2), "clear" (C3) or None (C1 only); always: the outputs are compared
    whatever the flag says (launches that must not trip, outputs that are legal beside a trip)."""
    fails = []
    for i, pr in enumerate(pairs):
        got, ref, tol = pr[0].detach().double().cpu(), pr[1].detach().double().cpu(), pr[2]
        assert got.shape == ref.shape, (kernel, case, got.shape, ref.shape)
        err = torch.nan_to_num((got - ref).abs(), nan=math.inf)
        lim = tol if len(pr) > 3 else tol * (1.0 + ref.abs())
        bad = ~(err <= lim)
        out = f" [output {i}]" if len(pairs) > 1 else ""
        print(f"RANGEEDGE {kernel} {case}{out} tripped={int(tripped)} {float(err.max()):.3e} (tol {tol:g}{' absolute' if len(pr) > 3 else ''}, ref max {float(ref.abs().max()):.3e})")
        if bad.any():
            fails.append(f"max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e}), {int(bad.sum())} / {bad.numel()} over tol {tol}")
    assert (tripped and not always) or not fails, f"C1 {kernel} {case}: flag clear and " + "; ".join(fails)
    if expect == "trip":
        assert tripped, f"C2 {kernel} {case}: a converted value >= 65536 and the flag is clear"
    if expect == "clear":
        assert not tripped, f"C3 {kernel} {case}: no converted value above 61440 and the flag is set"


def _outliers(conv, expect, what=""):
    """The reference's own check of a construction: `conv` = the values the kernel converts (fp64)."""
    a = conv.abs()
    if expect == "trip":
        assert float(a.max()) >= TRIP, f"{what}: the trip case is not one"
    elif expect == "clear":
        assert float(a.max()) <= CLEAR, f"{what}: the twin has a converted value of {float(a.max()):.1f}"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1a. split_planes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_split_planes_range(dev):
    """cbx_split_planes_f32 at (37, 320): the whole tensor and a column range of a wider Planes read from a column range of a wider fp32 tensor; 7e4 / 6e4 at the
    first and the last element and inside; +-inf; a 7e4 in the fp32 column just left / right of the range must not trip and must not be stored."""
    from chatterbox_amd import ops
    R, C = 37, 320
    base = _r((R, C), 1)
    try:
        _reset(dev)
        for (r, c) in ((0, 0), (R - 1, C - 1), (17, 5), (36, 2)):
            for val, expect in ((7.0e4, "trip"), (-7.0e4, "trip"), (6.0e4, "clear"), (math.inf, "trip"), (-math.inf, "trip")):
                x = base.clone()
                x[r, c] = val
                _outliers(x.double(), expect)
                P = ops.Planes(R, C, dev, zero=True)
                hit = _run(dev, lambda: ops.split_planes(x.to(dev), P))
                _verdict("split_planes", f"whole ({r},{c}) {val:g}", hit, [(P.float(), _planes_exact(x), 1e-12, "abs")], expect)
                wide = torch.zeros(R, 400)
                wide[:, 40:360] = x
                W = ops.Planes(R, 512, dev, zero=True)
                xv = wide.to(dev)[:, 40:360]
                hit = _run(dev, lambda: ops.split_planes(xv, W.cols(64, C)))
                _verdict("split_planes", f"column range ({r},{c}) {val:g}", hit, [(W.cols(64, C).float(), _planes_exact(x), 1e-12, "abs")], expect)
        wide = torch.zeros(R, 400)
        wide[:, 40:360] = base
        wide[0, 39] = wide[R - 1, 39] = wide[0, 360] = wide[R - 1, 360] = 7.0e4  # just outside the range
        W = ops.Planes(R, 512, dev, zero=True)
        xv = wide.to(dev)[:, 40:360]
        hit = _run(dev, lambda: ops.split_planes(xv, W.cols(64, C)))
        _verdict("split_planes", "7e4 just outside the column range", hit, [(W.cols(64, C).float(), _planes_exact(base), 1e-12, "abs")], "clear", always=True)
        t = W.t.float().cpu()
        assert float(t[:, :64].abs().max()) == 0.0 and float(t[:, 64 + C:512 + 64].abs().max()) == 0.0 and float(t[:, 512 + 64 + C:].abs().max()) == 0.0, "planes outside the range"
    finally:
        _reset(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1b. gemm_planes: plain plane epilogue, deferred-epilogue forms, V^T column range, LayerNorm epilogue
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm_base(M, N, K):
    return _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3), _r((M, N), 4)


@functools.lru_cache(maxsize=64)
def _product_case(M, N, K, m, n, k0, wval):
    """Operands with the output outlier 256 * wval at (m, n) and the fp64 product (+ bias) of the values their planes hold."""
    x, w, b, _ = _gemm_base(M, N, K)
    x, w = x.clone(), w.clone()
    x[m, k0], w[n, k0] = 256.0, wval
    return x, w, F.linear(_planes_exact(x), _planes_exact(w), b.double())


_WVALS = ((320.0, "trip", "80k"), (224.0, "clear", "56k"), (-320.0, None, "-80k"))


def _plain_position(dev, tag, pos, acts=("gelu", "silu"), residual=True):
    """Every plain-epilogue case at one position: plane-only output with bias + GELU / SILU (outlier through the product: +80k, +56k, and -80k that the activation
    turns into 0), fp32-only output of 80k (nothing is converted), fp32 + plane output with an in-place residual (outlier through R[m, n])."""
    from chatterbox_amd import ops
    M, N, K = MNK
    m, n, k0 = pos
    tol = 3e-5 * max(1.0, math.sqrt(K / 256))
    b = _gemm_base(M, N, K)[2]
    bd = b.to(dev)
    fns = dict(gelu=(ops.GELU_ERF, F.gelu), silu=(ops.SILU, F.silu))
    for wval, expect, name in _WVALS:
        x, w, ref0 = _product_case(M, N, K, m, n, k0, wval)
        xP, wP = ops.split_planes(x.to(dev)), ops.split_planes(w.to(dev))
        for an in acts:
            act, fn = fns[an]
            ref = fn(ref0)
            _outliers(ref, expect, f"{an} {name}")
            if expect == "trip":
                assert int((ref.abs() > 65504).sum()) == 1
            if expect is None:
                assert float(ref0.min()) < -65504 and float(ref.abs().max()) <= CLEAR
            outP = ops.Planes(M, N, dev, zero=True)
            hit = _run(dev, lambda: ops.linear_planes(xP, wP, outp=outP, bias=bd, act=act))
            _verdict("gemm_planes.plain", f"{tag} ({m},{n},{k0}) P+{an} {name}", hit, [(outP.float(), ref, tol)], expect)
        if expect == "trip":  # fp32 only: 80k is a legal fp32 value and nothing is converted
            out = torch.zeros(M, N).to(dev)
            hit = _run(dev, lambda: ops.linear_planes(xP, wP, out=out, bias=bd))
            _verdict("gemm_planes.plain", f"{tag} ({m},{n},{k0}) C only {name}", hit, [(out, ref0, tol)], "clear", always=True)
    if residual:
        x, w, _, r = _gemm_base(M, N, K)
        xP, wP = ops.split_planes(x.to(dev)), ops.split_planes(w.to(dev))
        ref0 = F.linear(_planes_exact(x), _planes_exact(w), b.double())
        for rval, expect in ((7.0e4, "trip"), (6.0e4, "clear")):
            rr = r.clone()
            rr[m, n] = rval
            ref = ref0 + rr.double()
            _outliers(ref, expect)
            out, outP = rr.clone().to(dev), ops.Planes(M, N, dev, zero=True)
            hit = _run(dev, lambda: ops.linear_planes(xP, wP, out=out, outp=outP, bias=bd, residual=out))
            _verdict("gemm_planes.plain", f"{tag} ({m},{n}) C+P residual {rval:g}", hit, [(out, ref, tol), (outP.float(), ref, tol)], expect)


@pytest.mark.parametrize("tile", _tiles())
def test_gemm_planes_plain_epilogue_range(dev, tile, persists=(1, 2, 0), sweep=None, acts=("gelu", "silu")):
    """The plain plane epilogue of every tile form at (333, 258, 256): the last element of the ragged last tile under persist 1, 2 and 0 (the chip-sized grid, two
    workgroups walking all tiles, one tile per workgroup); the forms of SWEEP_TILES take the whole position sweep, the persist setting cycling over the positions.
    Tiles 41 / 42 with a plane-only or fp32-only output run their deferred-epilogue kernels here (amax_df), with both outputs their plain twins."""
    from chatterbox_amd import ops
    sweep = tile in SWEEP_TILES if sweep is None else sweep
    try:
        _reset(dev)
        ops.lib.cbx_set_planes_tile(tile)
        for persist in persists:
            ops.lib.cbx_set_planes_persist(persist)
            _plain_position(dev, f"tile{tile}/persist{persist}", LAST, acts)
        if sweep:
            for i, pos in enumerate(p for p in POSITIONS if p != LAST):
                ops.lib.cbx_set_planes_persist(persists[i % len(persists)])
                _plain_position(dev, f"tile{tile}/persist{persists[i % len(persists)]}", pos, acts)
    finally:
        ops.lib.cbx_set_planes_tile(0)
        ops.lib.cbx_set_planes_persist(1)
        _reset(dev)


@pytest.mark.parametrize("tile,persist", [(41, 2), (41, 1), (42, 2), (42, 1)])
def test_gemm_planes_deferred_epilogue_range(dev, tile, persist, grid_tiles=None):
    """The deferred-epilogue forms (a finished tile's epilogue rides on the next tile's K loop; the last tile of a workgroup drains): one launch pair (trip, twin) per
    output tile of the 3 x 3 grid of 128 x 128 tiles, the outlier at a seeded position inside that tile -- with persist = 2 the two workgroups walk tiles 0, 2, 4, 6, 8 and
    1, 3, 5, 7: tiles 7 and 8 drain and every other one is folded; with persist = 1 every tile drains.  Both must feed amax_df."""
    from chatterbox_amd import ops
    M, N, K = MNK
    tol = 3e-5 * max(1.0, math.sqrt(K / 256))
    bd = _gemm_base(M, N, K)[2].to(dev)
    g = torch.Generator().manual_seed(41)
    try:
        _reset(dev)
        ops.lib.cbx_set_planes_persist(persist)
        for tm in range(3):
            for tn in range(3):
                m = tm * 128 + int(torch.randint(0, min(128, M - tm * 128), (1,), generator=g))
                n = tn * 128 + int(torch.randint(0, min(128, N - tn * 128), (1,), generator=g))
                k0 = int(torch.randint(0, K, (1,), generator=g))
                if grid_tiles is not None and (tm, tn) not in grid_tiles:
                    continue
                for wval, expect, name in _WVALS[:2]:
                    x, w, ref0 = _product_case(M, N, K, m, n, k0, wval)
                    xP, wP = ops.split_planes(x.to(dev)), ops.split_planes(w.to(dev))
                    ref = F.gelu(ref0)
                    _outliers(ref, expect)
                    outP = ops.Planes(M, N, dev, zero=True)
                    hit = _run(dev, lambda: ops.gemm_planes(xP, wP, M=M, N=N, K=K, P=outP, bias=bd, act=ops.GELU_ERF, tile=tile))
                    _verdict("gemm_planes.deferred", f"tile{tile}/persist{persist} grid tile ({tm},{tn}) at ({m},{n},{k0}) P+gelu {name}", hit, [(outP.float(), ref, tol)], expect)
                    if expect == "trip":  # the fp32 kind of the deferred epilogue converts nothing
                        out = torch.zeros(M, N).to(dev)
                        hit = _run(dev, lambda: ops.gemm_planes(xP, wP, M=M, N=N, K=K, C=out, ldc=N, bias=bd, tile=tile))
                        _verdict("gemm_planes.deferred", f"tile{tile}/persist{persist} grid tile ({tm},{tn}) C only {name}", hit, [(out, ref0, tol)], "clear", always=True)
    finally:
        ops.lib.cbx_set_planes_persist(1)
        _reset(dev)


@pytest.mark.parametrize("tile,persist", [(0, 1), (4, 2), (41, 2), (42, 1)])
@pytest.mark.parametrize("Z,T", [(3, 36), (2, 132)])
def test_gemm_planes_transposed_range(dev, Z, T, tile, persist, only=None):
    """q | k | V^T from one launch (PT, pt_n0 = 1024, N = 1536, K = 256): the outlier in a q | k column (plain plane store) and in a v column at (last group, t = T - 1)
    and (group 0, t = 0) (the transposed store).  The pad keys of V^T stay zero in both planes, tripped or not."""
    from chatterbox_amd import ops
    M, K, N, n0 = Z * T, 256, 1536, 1024
    Tp = (T + 7) // 8 * 8
    h0, w0 = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K))
    try:
        _reset(dev)
        ops.lib.cbx_set_planes_persist(persist)
        for what, (m, n, k0) in (("q|k", (M - 1, 1023, 255)), ("q|k", (0, 512, 0)), ("v last group t=T-1", (M - 1, N - 1, 255)), ("v group 0 t=0", (0, n0, 77)),
                                 ("v last group t=0", (M - T, n0 + 257, 3)))[slice(None) if only is None else only]:
            for wval, expect, name in _WVALS[:2]:
                h, w = h0.clone(), w0.clone()
                h[m, k0], w[n, k0] = 256.0, wval
                ref = F.linear(_planes_exact(h), _planes_exact(w))
                _outliers(ref, expect)
                hP, wP = ops.split_planes(h.to(dev)), ops.split_planes(w.to(dev))
                qkP, vtP = ops.Planes(M, n0, dev, zero=True), ops.Planes(Z * 512, Tp, dev, zero=True)
                hit = _run(dev, lambda: ops.gemm_planes(hP, wP, M=M, N=N, K=K, P=qkP, PT=vtP, pt_n0=n0, pt_T=T, pt_zs=512 * vtP.ld, tile=tile))
                vt = vtP.float().view(Z, 512, Tp)
                _verdict("gemm_planes.vt", f"tile{tile}/persist{persist} Z{Z} T{T} {what} ({m},{n},{k0}) {name}", hit,
                         [(qkP.float(), ref[:, :n0], 3e-5), (vt[:, :, :T], ref[:, n0:].reshape(Z, T, 512).transpose(1, 2), 3e-5)], expect)
                raw = vtP.t.float().cpu().view(Z * 512, 2, Tp)
                assert float(raw[:, :, T:].abs().max()) == 0.0, "pad keys of V^T stay zero"
    finally:
        ops.lib.cbx_set_planes_persist(1)
        _reset(dev)


@pytest.mark.parametrize("res", [False, True])
def test_gemm_planes_layernorm_epilogue_range(dev, res, M=333):
    """The LayerNorm epilogue (ln=, lnp=, N = 256, K = 256): an fp32 row that holds 8e4 is legal and its LayerNorm (|y| < 17) must come out right without a trip;
    LayerNorm planes driven out of range through ln_b[n] must trip (twin 6e4)."""
    from chatterbox_amd import ops
    N = K = 256
    x0, w0, b = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3)
    r = _r((M, N), 4) * 3.0 + 0.5
    lw, lb0 = 1 + 0.1 * _r((N,), 5), 0.1 * _r((N,), 6)
    tol = 3e-5

    def launch(x, w, lb):
        xP, wP = ops.split_planes(x.to(dev)), ops.split_planes(w.to(dev))
        out = r.clone().to(dev) if res else torch.zeros(M, N).to(dev)
        lnP = ops.Planes(M, N, dev, zero=True)
        hit = _run(dev, lambda: ops.linear_planes(xP, wP, out=out, bias=b.to(dev), residual=out if res else None, ln=(lw.to(dev), lb.to(dev)), lnp=lnP))
        ref = F.linear(_planes_exact(x), _planes_exact(w), b.double()) + (r.double() if res else 0)
        ln_ref = F.layer_norm(out.double().cpu(), (N,), lw.double(), lb.double(), 1e-5)
        return hit, out, lnP, ref, ln_ref

    try:
        _reset(dev)
        for (m, n, k0) in ((0, 0, 0), (M - 1, 255, 255), (64, 129, 37)):
            x, w = x0.clone(), w0.clone()
            x[m, k0], w[n, k0] = 256.0, 320.0
            hit, out, lnP, ref, ln_ref = launch(x, w, lb0)
            assert int((ref.abs() > 65504).sum()) == 1
            _outliers(ln_ref, "clear")
            _verdict("gemm_planes.ln", f"res{int(res)} fp32 row holds 80k at ({m},{n},{k0})", hit, [(out, ref, tol), (lnP.float(), ln_ref, 3e-6)], "clear", always=True)
        for n in (0, 255, 129):
            for val, expect in ((7.0e4, "trip"), (-7.0e4, "trip"), (6.0e4, "clear")):
                lb = lb0.clone()
                lb[n] = val
                hit, out, lnP, ref, ln_ref = launch(x0, w0, lb)
                _outliers(ln_ref, expect)
                _verdict("gemm_planes.ln", f"res{int(res)} ln_b[{n}]={val:g}", hit, [(lnP.float(), ln_ref, 3e-6)], expect)
                _verdict("gemm_planes.ln", f"res{int(res)} ln_b[{n}]={val:g} fp32 row", hit, [(out, ref, tol)], None, always=True)  # the fp32 row is legal beside a trip
    finally:
        _reset(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1c. layernorm_planes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_layernorm_planes_range(dev, rows=77):
    """cbx_layernorm_planes_f32 (C = 256; 77 rows: the narrow kernel, 16 lanes per row): one column driven out through ln_b[n] and through post_add[n], with and
    without MISH, at the first, the last and an inner column."""
    from chatterbox_amd import ops
    C = 256
    x, w, b0, pa0 = _r((rows, C), 1) * 3 + 0.5, 1 + 0.1 * _r((C,), 2), 0.1 * _r((C,), 3), _r((C,), 4)
    try:
        _reset(dev)
        for n in (0, C - 1, 130):
            for val, expect in ((7.0e4, "trip"), (-7.0e4, "trip"), (6.0e4, "clear")):
                for via in ("ln_b", "post_add"):
                    for mish in (False, True):
                        if val < 0 and via == "ln_b" and mish:
                            continue  # mish(-7e4) = -0: the post-activation case below
                        b, pa = b0.clone(), pa0.clone()
                        (b if via == "ln_b" else pa)[n] = val
                        ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
                        ref = (F.mish(ref) if mish else ref) + pa.double()
                        _outliers(ref, expect)
                        out = ops.Planes(rows, C, dev, zero=True)
                        hit = _run(dev, lambda: ops.layernorm_planes(x.to(dev), w.to(dev), b.to(dev), out, act=ops.MISH if mish else ops.NONE, post_add=pa.to(dev)))
                        _verdict("layernorm_planes", f"rows{rows} {via}[{n}]={val:g} mish{int(mish)}", hit, [(out.float(), ref, 3e-6)], expect)
        b = b0.clone()
        b[5] = -8.0e4  # post-activation: mish(-8e4) = -0, every stored value in range
        ref = F.mish(F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5))
        out = ops.Planes(rows, C, dev, zero=True)
        hit = _run(dev, lambda: ops.layernorm_planes(x.to(dev), w.to(dev), b.to(dev), out, act=ops.MISH))
        _verdict("layernorm_planes", f"rows{rows} ln_b[5]=-8e4 under mish", hit, [(out.float(), ref, 3e-6)], None)
    finally:
        _reset(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1d. the split GEMM at precision 16 (gemm_split.hip): A and W operand, every loader
# ---------------------------------------------------------------------------------------------------------------------------------------------
SPLIT_TOL = 3e-5  # tests/test_ops_gpu.py::_SPLIT_TOL[16]
_OPERAND = ((7.0e4, "trip"), (-7.0e4, "trip"), (6.0e4, "clear"))


@pytest.mark.parametrize("M,N,K", [(129, 257, 320), (65, 100, 36)])
def test_split_gemm_linear_range(dev, M, N, K):
    """Linear at precision 16: (129, 257, 320) the buffer-load loader, (65, 100, 36) the generic loader with a K tail; one element of A resp. W at the first and
    the last position and inside.  A 7e4 at column K of a strided lda > K view is outside the operand: no trip, and the output does not change by a bit."""
    from chatterbox_amd import ops
    import test_ops_gpu
    assert test_ops_gpu._SPLIT_TOL[16] == SPLIT_TOL
    x0, w0, b = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3)
    try:
        _reset(dev)
        with ops.gemm_precision(16):
            for opnd, where in (("A", ((0, 0), (M - 1, K - 1), (64, 33))), ("W", ((0, 0), (N - 1, K - 1), (64, 32)))):
                for (i, k) in where:
                    for val, expect in _OPERAND:
                        x, w = x0.clone(), w0.clone()
                        (x if opnd == "A" else w)[i, k] = val
                        out = torch.zeros(M, N).to(dev)
                        hit = _run(dev, lambda: ops.linear(x.to(dev), w.to(dev), out, bias=b.to(dev)))
                        _verdict("gemm_split.linear", f"{M}x{N}x{K} {opnd}[{i},{k}]={val:g}", hit, [(out, F.linear(x.double(), w.double(), b.double()), SPLIT_TOL)], expect)
            wide = torch.zeros(M, K + 4)
            wide[:, :K] = x0
            plain, guard = torch.zeros(M, N).to(dev), torch.zeros(M, N).to(dev)
            xv = wide.to(dev)
            hit = _run(dev, lambda: ops.linear(xv[:, :K], w0.to(dev), plain, bias=b.to(dev)))
            _verdict("gemm_split.linear", f"{M}x{N}x{K} strided view", hit, [(plain, F.linear(x0.double(), w0.double(), b.double()), SPLIT_TOL)], "clear", always=True)
            wide[0, K] = wide[M - 1, K] = wide[M // 2, K + 3] = 7.0e4
            xv = wide.to(dev)
            hit = _run(dev, lambda: ops.linear(xv[:, :K], w0.to(dev), guard, bias=b.to(dev)))
            _verdict("gemm_split.linear", f"{M}x{N}x{K} 7e4 at column K of a strided view", hit, [(guard, F.linear(x0.double(), w0.double(), b.double()), SPLIT_TOL)], "clear", always=True)
            assert torch.equal(plain, guard), "an element outside the operand changed the output"
    finally:
        _reset(dev)


def test_split_gemm_layernorm_fold_range(dev, M=333):
    """LayerNorm folded into the A operand (333, 80, 256).  The check looks at the values that are CONVERTED, the normalised ones: rows offset by 1e5 (raw values
    far outside fp16) whose normalised values are in range keep the flag clear and come out right; an ln_w[k] that pushes the normalised values of column k out of
    range must trip.  The rows are exact by construction (even integers in [-64, 64] in antisymmetric pairs + 1e5: every partial sum of the row is a multiple of 2
    below 2^25 and exact in fp32 in any order, so the mean is 1e5 exactly and only the guard is measured; the statistics themselves: tests/test_norm_stress_gpu.py)."""
    from chatterbox_amd import ops
    N, K = 80, 256
    g = torch.Generator().manual_seed(7)
    v = torch.randint(-32, 33, (M, K // 2), generator=g).float() * 2
    d = torch.cat([v, -v], 1)
    d = torch.stack([row[torch.randperm(K, generator=g)] for row in d])
    x = d + 1.0e5
    assert torch.equal(x.double(), d.double() + 1.0e5) and torch.equal(x.sum(1), torch.full((M,), 256.0e5))
    w, b = _r((N, K), 2, 1 / math.sqrt(K)), _r((N,), 3)
    lw0, lb = 1 + 0.1 * _r((K,), 4), 0.1 * _r((K,), 5)
    try:
        _reset(dev)
        with ops.gemm_precision(16):
            assert ops.ln_fusable(M, K)
            stats = ops.row_stats(x.to(dev), torch.zeros(M, 2).to(dev))
            for k0, gain, expect in ((None, None, "clear"), (0, 1.0e5, "trip"), (255, -1.0e5, "trip"), (130, 1.0e5, "trip"), (130, 3.0e4, "clear")):
                lw = lw0.clone()
                if k0 is not None:
                    lw[k0] = gain
                norm = F.layer_norm(x.double(), (K,), lw.double(), lb.double(), 1e-5)
                _outliers(norm, expect)
                out = torch.zeros(M, N).to(dev)
                hit = _run(dev, lambda: ops.linear(x.to(dev), w.to(dev), out, bias=b.to(dev), ln=(stats, lw.to(dev), lb.to(dev))))
                _verdict("gemm_split.ln_fold", f"{M}x{N}x{K} rows + 1e5, " + ("plain ln_w" if k0 is None else f"ln_w[{k0}]={gain:g}"), hit,
                         [(out, F.linear(norm, w.double(), b.double()), SPLIT_TOL)], expect)
    finally:
        _reset(dev)


def _conv_case(dev, kernel, case, x, w, b, expect, *, k, dil=1, pad=0, up=1, lens=None, transpose=None):
    """One Conv1d launch at precision 16 against fp64 conv1d (x (B, cin, T), w torch layout)."""
    from chatterbox_amd import ops, weights
    B, cin, T = x.shape
    if transpose is not None:
        s, p = transpose
        ref = F.conv_transpose1d(x.double(), w.double(), b.double(), stride=s, padding=p)
        wp, bp = weights.pack_conv_transpose(w, b, s, p)
        out = torch.zeros(B, T, wp.shape[0]).to(dev)
        hit = _run(dev, lambda: ops.conv1d(x.transpose(1, 2).contiguous().to(dev), wp.to(dev), out, taps=3, cin=cin, bias=bp.to(dev), pad_left=1))
        got = out.view(B, T * s, w.shape[1]).transpose(1, 2)
        _verdict(kernel, case, hit, [(got, ref, SPLIT_TOL)], expect)
        return
    xd = x.double().repeat_interleave(up, dim=2) if up > 1 else x.double()
    if up > 1:  # nearest upsample + left pad
        ref = F.conv1d(F.pad(xd, (pad, 0)), w.double(), b.double())
    elif lens is not None:  # look-ahead conv: zeros beyond each row's own length
        ref = None
    else:
        ref = F.conv1d(xd, w.double(), b.double(), dilation=dil, padding=pad)
    Tout = T * up if ref is None or up > 1 else ref.shape[2]
    out = torch.zeros(B, Tout, w.shape[0]).to(dev)
    hit = _run(dev, lambda: ops.conv1d(x.transpose(1, 2).contiguous().to(dev), weights.pack_conv(w).to(dev), out, taps=k, cin=cin, bias=b.to(dev), dil=dil, pad_left=pad,
                                        up=up, lens=None if lens is None else lens.to(dev)))
    if lens is None:
        _verdict(kernel, case, hit, [(out.transpose(1, 2), ref, SPLIT_TOL)], expect)
    else:
        pairs = []
        for i in range(B):
            n = int(lens[i])
            pairs.append((out[i, :n].t(), F.conv1d(F.pad(x[i:i + 1, :, :n].double(), (0, k - 1)), w.double(), b.double())[0], SPLIT_TOL))
        _verdict(kernel, case, hit, pairs, expect)


@pytest.mark.parametrize("which", ["fast_taps", "dilated", "upsample", "ragged", "transpose"])
def test_split_gemm_conv_range(dev, which):
    """Conv1d at precision 16: (32, 48, 3, 1, 1, 1, 77) the fast tap loader, (64, 64, 11, 5, 1, 25, 300) dilation, nearest x2 upsample + 5 taps (C = 32, T = 50) on the
    generic loader, ConvTranspose (32, 16, 11, 5, 3) as a 3-tap conv -- the outlier at t = 0, at t = T - 1 and in a weight tap.  The ragged 4-tap conv
    (lens = [50, 31, 7]) with a 7e4 at a row >= lens[z]: such a row reads as zero, C1 only, whether it tripped is printed."""
    from chatterbox_amd import ops
    B = 3
    try:
        _reset(dev)
        with ops.gemm_precision(16):
            if which == "ragged":
                C, T = 32, 50
                lens = torch.tensor([50, 31, 7], dtype=torch.int32)
                x0, w, b = _r((B, C, T), 1), _r((C, C, 4), 2, 0.1), _r((C,), 3)
                _conv_case(dev, "gemm_split.conv_ragged", "in range", x0, w, b, "clear", k=4, lens=lens)
                for (z, t) in ((1, 31), (2, 7), (2, T - 1)):
                    x = x0.clone()
                    x[z, 5, t] = 7.0e4
                    _conv_case(dev, "gemm_split.conv_ragged", f"7e4 at masked row (z {z}, t {t})", x, w, b, None, k=4, lens=lens)
                return
            cin, cout, k, dil, pad, T, kw = {"fast_taps": (32, 48, 3, 1, 1, 77, {}), "dilated": (64, 64, 11, 5, 25, 300, {}), "upsample": (32, 32, 5, 1, 4, 50, dict(up=2)),
                                             "transpose": (32, 16, 11, 1, 0, 41, dict(transpose=(5, 3)))}[which]
            tr = which == "transpose"
            x0, b = _r((B, cin, T), 1), _r((cout,), 3)
            w0 = _r((cin, cout, k), 2, 0.1) if tr else _r((cout, cin, k), 2, 1 / math.sqrt(cin * k))
            spots = [("x", (1, 0, 0)), ("x", (2, cin - 1, T - 1)), ("x", (0, 7, T // 2)), ("w", (0, 0, 0)), ("w", (w0.shape[0] - 1, w0.shape[1] - 1, k - 1)), ("w", (3, 5, k // 2))]
            for opnd, idx in spots:
                for val, expect in _OPERAND:
                    x, w = x0.clone(), w0.clone()
                    (x if opnd == "x" else w)[idx] = val
                    _conv_case(dev, f"gemm_split.conv_{which}", f"{opnd}{list(idx)}={val:g}", x, w, b, expect, k=k, dil=dil, pad=pad, **kw)
    finally:
        _reset(dev)


def test_precision16_shapes_on_the_exact_kernels_range(dev):
    """Shapes that precision 16 hands to the exact fp32 kernels (M <= 32: the skinny GEMM; cin = 80: no 32-wide K tile inside a tap): the operands are never
    converted, so 7e4 is a legal value.  C1 only; whether the flag tripped is printed."""
    from chatterbox_amd import ops
    try:
        _reset(dev)
        with ops.gemm_precision(16):
            M, N, K = 16, 100, 64
            x, w, b = _r((M, K), 1), _r((N, K), 2, 1 / 8), _r((N,), 3)
            x[M - 1, K - 1] = 7.0e4
            w[0, 0] = -7.0e4
            out = torch.zeros(M, N).to(dev)
            hit = _run(dev, lambda: ops.linear(x.to(dev), w.to(dev), out, bias=b.to(dev)))
            _verdict("gemm_f32.skinny", f"{M}x{N}x{K} precision 16, +-7e4 operands", hit, [(out, F.linear(x.double(), w.double(), b.double()), SPLIT_TOL)], None)
            xc, wc, bc = _r((2, 80, 60), 1), _r((48, 80, 7), 2, 1 / math.sqrt(560)), _r((48,), 3)
            xc[1, 79, 59] = 7.0e4
            _conv_case(dev, "gemm_f32.conv_cin80", "precision 16, x = 7e4", xc, wc, bc, None, k=7, pad=3)
    finally:
        _reset(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1e. the split flash attention at precision 16 (attention_split.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, lens, causal):
    q, k, v = (qkv[:, :, i].transpose(1, 2).double() for i in range(3))
    Z, T = qkv.shape[0], qkv.shape[1]
    s = torch.einsum("zhqd,zhkd->zhqk", q, k) * 0.125
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), -math.inf)
    if lens is not None:
        for z in range(Z):
            s[z, :, :, int(lens[z]):] = -math.inf
    return torch.einsum("zhqk,zhkd->zqhd", torch.softmax(s, -1), v)


def _attn_launch(dev, qkv, lens, causal, po):
    from chatterbox_amd import ops
    from chatterbox_amd._lib import check
    Z, T, _, H, _ = qkv.shape
    d = qkv.to(dev)
    kl = None if lens is None else lens.to(dev)
    qq, kk, vv = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    if not po:
        out = torch.zeros(Z, T, H, 64).to(dev)
        hit = _run(dev, lambda: ops.flash_attn(qq, kk, vv, out, 0.125, key_lens=kl, causal=causal))
        return hit, out
    outP = ops.Planes(Z * T, H * 64, dev, zero=True)
    hit = _run(dev, lambda: check(ops.lib.cbx_flash_attn_split_po(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), outP.ptr, None if kl is None else kl.data_ptr(), Z, H, T, T,
                                                                  qq.stride(0), qq.stride(1), kk.stride(0), kk.stride(1), vv.stride(0), vv.stride(1), T * outP.ld, outP.ld, outP.lo,
                                                                  0.125, int(causal), ops._stream()), "cbx_flash_attn_split_po"))
    return hit, outP.float().view(Z, T, H, 64)


@pytest.mark.parametrize("po", [False, True], ids=["f32_out", "plane_out"])
@pytest.mark.parametrize("T,causal", [(130, False), (103, True)])
def test_split_flash_attn_range(dev, T, causal, po):
    """cbx_flash_attn_split_f32 at precision 16 and cbx_flash_attn_split_po (plane output), (Z, H) = (2, 4), T = 130 with key lengths (130, 93) and T = 103 causal:
    one element of q, of k and of v each, at token 0 and at token T - 1 (of the utterance whose keys are all valid).  q is converted AFTER its pre-scaling by
    scale log2(e) = 0.18034: 4.0e5 -> 72135 trips, 3.3e5 -> 59511 must not; a q of 7e4 (12624 scaled) must not either.  A masked key (index >= its utterance's
    length) holding 7e4 in k and v reads as zero: C1 only, whether it tripped is printed.  The plane output converts a convex combination of v: nothing new to check."""
    from chatterbox_amd import ops
    Z, H = 2, 4
    base = _r((Z, T, 3, H, 64), 1)
    lens = None if causal else torch.tensor([T, T - 37], dtype=torch.int32)
    sc = 0.125 * 1.4426950408889634
    kern = "attention_split.po" if po else "attention_split"
    try:
        _reset(dev)
        with ops.gemm_precision(16):
            for tok in (0, T - 1):
                for i, name in enumerate("qkv"):
                    vals = ((4.0e5, "trip"), (-4.0e5, "trip"), (3.3e5, "clear"), (7.0e4, "clear")) if name == "q" else _OPERAND
                    for val, expect in vals:
                        qkv = base.clone()
                        h, dd = (1 + i) % H, (17 * (i + 1) + tok) % 64
                        qkv[0, tok, i, h, dd] = val
                        conv = torch.stack([qkv[:, :, 0].double() * sc, qkv[:, :, 1].double(), qkv[:, :, 2].double()])
                        _outliers(conv, expect)
                        hit, got = _attn_launch(dev, qkv, lens, causal, po)
                        _verdict(kern, f"T{T} causal{int(causal)} {name}[token {tok}, head {h}, d {dd}]={val:g}", hit, [(got, _attn_ref(qkv, lens, causal), 2e-5)], expect)
            if lens is not None:
                for tok in (T - 37, T - 1):
                    qkv = base.clone()
                    qkv[1, tok, 1, 2, 9] = qkv[1, tok, 2, 3, 40] = 7.0e4
                    hit, got = _attn_launch(dev, qkv, lens, causal, po)
                    _verdict(kern, f"T{T} masked key {tok} of utterance 1 (length {T - 37}) holds 7e4 in k and v", hit, [(got, _attn_ref(qkv, lens, causal), 2e-5)], None)
    finally:
        _reset(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the lower end
# ---------------------------------------------------------------------------------------------------------------------------------------------
SCALES = (-10, -14, -17, -20, -23, -26)


def _low_check(kernel, case, tripped, got, ref, bound):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = torch.nan_to_num((got - ref).abs(), nan=math.inf)
    ratio = float((err / bound).max())
    print(f"RANGEEDGE {kernel} {case} tripped={int(tripped)} {float(err.max()):.3e} (max err / bound {ratio:.3f}, ref max {float(ref.abs().max()):.3e})")
    rows = got.reshape(-1, got.shape[-1])
    assert bool((rows != 0).any(-1).all()), f"{kernel} {case}: an all-zero output row (flushed subnormals?)"
    assert bool((err <= bound).all()), f"{kernel} {case}: max err / bound {ratio:.3f}, {int((err > bound).sum())} / {err.numel()} elements over the bound"
    assert not tripped, f"{kernel} {case}: tiny operands tripped the range flag"


def _low_cases(x, w):
    """(name, x, w, both_small) over the scales of the module docstring."""
    for e in SCALES:
        yield f"x*2^{e}", x * 2.0 ** e, w, False
    yield "x*2^-8 w*2^-12", x * 2.0 ** -8, w * 2.0 ** -12, True


def _bound(xa, wa, K, both, first_only=False):
    """xa (M, K), wa (N, K): |operands| in fp64 -> the per-element bound (M, N) of the module docstring."""
    first = 2.0 ** -22 * math.sqrt(max(1.0, K / 256)) * (xa @ wa.t())
    if first_only:
        return first
    second = wa.sum(1)[None, :] + (xa.sum(1)[:, None] if both else 0.0)
    return first + 2.0 ** -35 * second


@pytest.mark.parametrize("M,N,K", [(64, 96, 256), (65, 100, 36)])
def test_lower_end_linear(dev, M, N, K):
    """ops.linear at precision 16 (and 6 as the control) on operands whose h plane is subnormal or zero."""
    from chatterbox_amd import ops
    x0, w0 = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K))
    try:
        _reset(dev)
        for name, x, w, both in _low_cases(x0, w0):
            ref = x.double() @ w.double().t()
            for prec in (16, 6):
                out = torch.zeros(M, N).to(dev)
                with ops.gemm_precision(prec):
                    hit = _run(dev, lambda: ops.linear(x.to(dev), w.to(dev), out))
                _low_check(f"gemm_split.linear.p{prec}", f"{M}x{N}x{K} {name}", hit, out, ref, _bound(x.double().abs(), w.double().abs(), K, both, first_only=prec == 6))
    finally:
        _reset(dev)


@pytest.mark.parametrize("tile", [9, 35])
def test_lower_end_linear_planes(dev, tile):
    """split_planes + linear_planes (fp32 and plane output) through a symmetric 64 x 64 form and a loader-wave form on the same tiny operands."""
    from chatterbox_amd import ops
    M, N, K = 64, 96, 256
    x0, w0 = _r((M, K), 1), _r((N, K), 2, 1 / math.sqrt(K))
    try:
        _reset(dev)
        ops.lib.cbx_set_planes_tile(tile)
        for name, x, w, both in _low_cases(x0, w0):
            ref = x.double() @ w.double().t()
            bound = _bound(x.double().abs(), w.double().abs(), K, both)
            xP, wP = ops.Planes(M, K, dev, zero=True), ops.Planes(N, K, dev, zero=True)
            hit = _run(dev, lambda: (ops.split_planes(x.to(dev), xP), ops.split_planes(w.to(dev), wP)))
            out, outP = torch.zeros(M, N).to(dev), ops.Planes(M, N, dev, zero=True)
            hit |= _run(dev, lambda: ops.linear_planes(xP, wP, out=out, outp=outP))
            _low_check("gemm_planes", f"tile{tile} {M}x{N}x{K} {name} (fp32 out)", hit, out, ref, bound)
            # the plane output stores the result as a pair again: 2^-22 of it, or 2^-36 absolute below 2^-14
            _low_check("gemm_planes", f"tile{tile} {M}x{N}x{K} {name} (plane out)", hit, outP.float(), ref, bound + 2.0 ** -22 * ref.abs() + 2.0 ** -36)
    finally:
        ops.lib.cbx_set_planes_tile(0)
        _reset(dev)


def test_lower_end_conv(dev):
    """Conv1d (32, 48, 3, 1, 1, 1, 77) at precision 16 / 6 on a tiny input: the bound with the taps as the contraction (zero padding contributes nothing)."""
    from chatterbox_amd import ops, weights
    B, cin, cout, k, T = 3, 32, 48, 3, 77
    x0, w0 = _r((B, cin, T), 1), _r((cout, cin, k), 2, 1 / math.sqrt(cin * k))
    try:
        _reset(dev)
        for name, x, w, both in _low_cases(x0, w0):
            ref = F.conv1d(x.double(), w.double(), padding=1).transpose(1, 2)
            sabs = F.conv1d(x.double().abs(), w.double().abs(), padding=1).transpose(1, 2)
            wsum = w.double().abs().sum((1, 2))[None, None, :]
            xsum = F.conv1d(x.double().abs(), torch.ones(1, cin, k, dtype=torch.float64), padding=1).transpose(1, 2)
            for prec in (16, 6):
                bound = 2.0 ** -22 * sabs + (0.0 if prec == 6 else 2.0 ** -35 * (wsum + (xsum if both else 0.0)))
                out = torch.zeros(B, T, cout).to(dev)
                with ops.gemm_precision(prec):
                    hit = _run(dev, lambda: ops.conv1d(x.transpose(1, 2).contiguous().to(dev), weights.pack_conv(w).to(dev), out, taps=k, cin=cin, pad_left=1))
                _low_check(f"gemm_split.conv.p{prec}", f"cin{cin} k{k} T{T} {name}", hit, out, ref, bound)
    finally:
        _reset(dev)


def test_lower_end_attention_v(dev):
    """The split flash attention at precision 16 with the v operand scaled down (q, k of order 1): p = softmax is the in-range operand of P V.  Its own error is
    the attention's 2e-5 and not 2^-22: |err| <= 2e-5 sum_j p_j |v_j| + 2^-35 sum_j p_j, and sum_j p_j = 1 (module docstring)."""
    from chatterbox_amd import ops
    Z, T, H = 2, 130, 4
    base = _r((Z, T, 3, H, 64), 1)
    lens = torch.tensor([T, T - 37], dtype=torch.int32)
    try:
        _reset(dev)
        for e in SCALES:
            qkv = base.clone()
            qkv[:, :, 2] *= 2.0 ** e
            ref = _attn_ref(qkv, lens, False)
            absv = qkv.clone()
            absv[:, :, 2] = absv[:, :, 2].abs()
            q, k = (qkv[:, :, i].transpose(1, 2).double() for i in range(2))
            s = torch.einsum("zhqd,zhkd->zhqk", q, k) * 0.125
            for z in range(Z):
                s[z, :, :, int(lens[z]):] = -math.inf
            bound = 2e-5 * torch.einsum("zhqk,zhkd->zqhd", torch.softmax(s, -1), absv[:, :, 2].transpose(1, 2).double()) + 2.0 ** -35
            for prec in (16, 6):
                with ops.gemm_precision(prec):
                    hit, got = _attn_launch(dev, qkv, lens, False, False)
                _low_check(f"attention_split.p{prec}", f"T{T} v*2^{e}", hit, got, ref, bound)
    finally:
        _reset(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the engine
# ---------------------------------------------------------------------------------------------------------------------------------------------
SAMP = dict(temperature=0.8, top_p=1.0, min_p=0.05, repetition_penalty=1.2, cfg_weight=0.5)


def _hift_noise(B, frames, seed):
    from chatterbox_amd import synth
    phase = (synth.rand((B, 9), seed=seed) * 2 - 1) * math.pi
    phase[:, 0] = 0
    return phase, synth.randn((B, 9, frames * 480), seed=seed + 1)


def _s3gen_at(eng, sd, dev, precision):
    """The engine's flow and vocoder BUILT at `precision` (the constructors' own argument)."""
    from chatterbox_amd.hift import HiFTEngine
    from chatterbox_amd.s3gen import FlowEngine
    eng.flow, eng.hift = FlowEngine(sd, dev, precision=precision), HiFTEngine(sd, dev, precision=precision)
    assert eng.flow.precision == precision and eng.hift.precision == precision
    return eng


def _engine(dev, L=2, precision=None):
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine
    sd = synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1)
    eng = ChatterboxEngine(synth.t3_state_dict(L, 0), sd, dev, n_t3_layers=L)
    return eng if precision is None else _s3gen_at(eng, sd, dev, precision)


def _words_clear_and_word0_registered(dev):
    from chatterbox_amd import ops
    assert not ops.range_flag_tripped(dev, 0) and not ops.range_flag_tripped(dev, 1), "a flag word was left set"
    assert ops._RANGE_FLAGS[ops._dev_index(dev)][1] == 0, "word 0 is registered"


def test_pipelined_schedule_attributes_a_trip_to_its_job(dev):
    """synthesize_pipelined on a real engine, three jobs of which job 1's z is scaled by 1e5: RANGE_TRIPS rises by exactly 1; jobs 0 and 2 are bit-identical to the
    same schedule without the scaled job (their word never tripped, nothing was repeated); job 1 equals the serial call, which trips and repeats at bf16x6."""
    from chatterbox_amd import engine as E, synth
    L, steps, P = 2, 10, 6
    eng = _engine(dev, L)
    assert eng.flow.precision == 16 and eng.hift.precision == 16
    cond, ref = synth.t3_cond(), synth.s3gen_ref(n_prompt_tokens=P)

    def jobs(scale1):
        out = []
        for j in range(3):
            texts = [synth.text_tokens(8 + 3 * j, seed=10 + j), synth.text_tokens(12, seed=20 + j)]
            ph, no = _hift_noise(2, 2 * steps, 50 + 2 * j)
            z = synth.randn((2, 2 * (P + steps), 80), seed=40 + j) * (scale1 if j == 1 else 1.0)
            out.append(dict(text_tokens=texts, t3_conds=cond, gen_ref=ref, uniforms=synth.rand((2, steps), seed=30 + j).to(dev), z=z.to(dev), phase=ph, noise=no))
        return out
    kw = dict(max_new_tokens=steps, ban_eos=True, ban_from=6561, n_cfm_timesteps=2, **SAMP)
    try:
        _reset(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            trips = E.RANGE_TRIPS
            clean = list(eng.synthesize_pipelined(jobs(1.0), **kw))
            assert E.RANGE_TRIPS == trips, "in-range jobs tripped"
            _words_clear_and_word0_registered(dev)
            mixed = list(eng.synthesize_pipelined(jobs(1.0e5), **kw))
            assert E.RANGE_TRIPS == trips + 1, f"RANGE_TRIPS rose by {E.RANGE_TRIPS - trips}: one job is out of range"
            _words_clear_and_word0_registered(dev)
            j1 = jobs(1.0e5)[1]
            w_serial, t_serial = eng.synthesize(j1["text_tokens"], cond, ref, uniforms=j1["uniforms"], z=j1["z"], phase=j1["phase"], noise=j1["noise"], **kw)
            assert E.RANGE_TRIPS == trips + 2, "the serial call of the scaled job trips as well"
        for j in (0, 2):
            assert [t.tolist() for t in clean[j][1]] == [t.tolist() for t in mixed[j][1]]
            for a, b in zip(clean[j][0], mixed[j][0]):
                assert torch.equal(a, b), f"job {j} changed beside an out-of-range job"
        assert [t.tolist() for t in mixed[1][1]] == [t.tolist() for t in t_serial]
        for a, b in zip(w_serial, mixed[1][0]):
            assert torch.isfinite(b).all() and torch.equal(a.cpu(), b), "job 1: the pipelined repeat differs from the serial tripped call"
        _words_clear_and_word0_registered(dev)
    finally:
        _reset(dev)


def test_batch_with_one_row_out_of_range_equals_bf16x6(dev):
    """vocode() of a batch of two whose row 1 alone is out of range (its z scaled by 1e5): the whole batch is repeated, and the result is that of an engine at
    precision 6, bit for bit."""
    from chatterbox_amd import engine as E, synth
    P, N = 6, 14
    eng, eng6 = _engine(dev, L=1), _engine(dev, L=1, precision=6)
    assert eng.flow.precision == 16 and eng.hift.precision == 16
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    toks = [synth.speech_tokens(N, seed=1), synth.speech_tokens(N - 5, seed=2)]
    z = synth.randn((2, 2 * (P + N), 80), seed=5)
    z[1] *= 1.0e5
    ph, no = _hift_noise(2, 2 * N, 60)
    try:
        _reset(dev)
        trips = E.RANGE_TRIPS
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            wav16, mel16 = eng.vocode(toks, ref, z=z.to(dev), phase=ph, noise=no, n_cfm_timesteps=2)
        assert E.RANGE_TRIPS == trips + 1 and any("fp16 range" in str(x.message) for x in w)
        wav6, mel6 = eng6.vocode(toks, ref, z=z.to(dev), phase=ph, noise=no, n_cfm_timesteps=2)
        assert E.RANGE_TRIPS == trips + 1
        assert torch.isfinite(mel16[0]).all() and torch.equal(mel16, mel6)
        for a, b in zip(wav16, wav6):
            assert torch.equal(a, b)
        _words_clear_and_word0_registered(dev)
    finally:
        _reset(dev)


@pytest.mark.parametrize("window", [None, 9], ids=["plain", "windowed"])
def test_streaming_rounds_repeated_at_bf16x6_leave_no_trace(dev, window):
    """vocode_stream (26 and 19 tokens, six rounds; windowed: the window moves from round 4 on) with a prompt mel scaled by 3e4: EVERY round trips and is repeated at
    bf16x6.  The stream is bit-identical to that of an engine at precision 6 and RANGE_TRIPS rises once per vocoded round: the discarded f16x3 pass leaves nothing in
    the carried state (source cache, phase scan, tails).  A clean stream on the same engine afterwards raises no warning and equals that of a fresh precision-16 engine."""
    from chatterbox_amd import engine as E, synth
    from chatterbox_amd.api import ChatterboxVC
    P, lens = 8, [26, 19]
    sd = synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1)
    eng, eng6, fresh = (ChatterboxVC._engine(sd, dev) for _ in range(3))
    assert eng.flow.precision == 16 and eng.hift.precision == 16
    _s3gen_at(eng6, sd, dev, 6)
    ref = synth.s3gen_ref(n_prompt_tokens=P)
    big = dict(ref, prompt_feat=ref["prompt_feat"] * 3.0e4)
    toks = [synth.speech_tokens(n, seed=3 + b) for b, n in enumerate(lens)]
    z = synth.randn((2, 2 * (P + lens[0]), 80), seed=5)
    ph, no = _hift_noise(2, 2 * lens[0], 70)
    kw = dict(first_chunk=5, chunk=4, lookahead=1, fade=240, window=window, z=z, phase=ph, noise=no, n_cfm_timesteps=2)

    def stream(e, voice):
        return [[w.clone() for w in r["wavs"]] for r in e.vocode_stream(toks, voice, **kw)]
    try:
        _reset(dev)
        trips = E.RANGE_TRIPS
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = stream(eng, big)
        assert len(got) == 6 and E.RANGE_TRIPS - trips == len(got), f"{E.RANGE_TRIPS - trips} repeats for {len(got)} vocoded rounds"
        want = stream(eng6, big)
        assert E.RANGE_TRIPS - trips == len(got), "the precision-6 engine does not look at the flag"
        assert len(want) == len(got)
        for r, (a, b) in enumerate(zip(got, want)):
            for u in range(2):
                assert torch.isfinite(a[u]).all() and torch.equal(a[u], b[u]), f"round {r}, utterance {u}: the repeated round differs from the bf16x6 stream"
        assert all(sum(r[u].numel() for r in got) == 960 * n for u, n in enumerate(lens))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            clean = stream(eng, ref)
        assert not any("fp16 range" in str(x.message) for x in w) and E.RANGE_TRIPS - trips == len(got)
        want = stream(fresh, ref)
        assert len(clean) == len(want)
        for r, (a, b) in enumerate(zip(clean, want)):
            for u in range(2):
                assert torch.equal(a[u], b[u]), f"round {r}, utterance {u}: a clean stream after repeated rounds differs from a fresh engine's"
        _words_clear_and_word0_registered(dev)
    finally:
        _reset(dev)
