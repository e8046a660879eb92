"""Bodies of tests/test_two_tile_decode_gpu.py (they take `dev` first; tests/test_simt_two_tile.py runs the kernel bodies on the emulator with a CPU device).

The packed five-launch decode layer at 17 .. 32 rows runs every launch on TWO 16-row tiles that share the weight registers and nothing else, so a row of a
two-tile launch must be bit for bit the row a one-tile launch on its own 16-row image gives.  The bodies here state that identity launch by launch -- each v2
GEMV form, the decode attention with and without the q|k|v partial fold --, for the engine (logits of every step against the same utterances decoded in
batches of at most 8) and for the throughput schedule (synthesize_pipelined(t3_pair=True) against t3_pair=False).  Every comparison is torch.equal: no tolerance.

Shapes the entry point refuses at every row count are not bent to fit: out_packed and swiglu need N % 32 == 0, so at N = 48 the out_packed forms write
row-major and the swiglu form is checked to be refused (one tile and two alike); a workgroup of nw waves needs K % (32 ksplit nw) == 0, so `down` takes the
largest of (ksplit 4, 4 waves), (2, 4) that K admits, and 16 waves (ksplit 1) where K % 512 == 0, else 8.  n_xpart = 1 does not exist (a down projection with
ksplit 1 adds the residual itself and leaves no partial image): it is checked to be refused.
"""
import math

import pytest
import torch

ROWS = (17, 31, 32)
KS = (256, 512)
NS = (32, 48)
FORMS = ("qkv_np0", "qkv_np2", "qkv_np4", "qkv_np1_refused", "qkv_ct_np0", "qkv_ct_np2", "qkv_ct_np4", "o_res", "o_res_tile8", "o_res_pre_epi", "gu", "gu_shallow",
         "gu_pre_epi", "down_ks1", "down_ks4", "head_ct_np0", "head_ct_np2", "head_ct_np4")
FMAX = torch.finfo(torch.float32).max

_CACHE = {}


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def packed_index(rows16, K):
    """flat offset, in the lane-ordered packed operand image (include/cbx.h), of element (r, k) of a (rows16, K) matrix: (rows16, K) long tensor."""
    r = torch.arange(rows16).view(-1, 1)
    k = torch.arange(K).view(1, -1)
    return (((r >> 4) * (K >> 5) + (k >> 5)) * 2 + ((k >> 2) & 1)) * 256 + ((((k >> 3) & 3) << 4) + (r & 15)) * 4 + (k & 3)


def pack_rows(x, rows16, pad=0.0):
    """(M, K) row-major -> the packed image (rows16, K) whose rows past M hold `pad`."""
    M, K = x.shape
    full = torch.full((rows16, K), float(pad))
    full[:M] = x
    img = torch.empty(rows16 * K)
    img[packed_index(rows16, K).reshape(-1)] = full.reshape(-1)
    return img.view(rows16, K)


def unpack_rows(img, M, K):
    flat = img.detach().cpu().reshape(-1)
    return flat[packed_index(img.shape[0], K)[:M].reshape(-1)].view(M, K)


def _tiles(rows):
    return [(0, 16), (16, rows - 16)]


def _gemv_case(form, K, N):
    """(keyword arguments common to the launches, number of partial images, output kind) of a form at (K, N); output kind: 'rm' row-major, 'pk' packed,
    'parts' split-K partial slices (row-major or packed per `pk`)."""
    from chatterbox_amd import ops
    pkd = N % 32 == 0
    if form.startswith("qkv_ct") or form.startswith("head_ct"):
        ct, ks = (3, K // 256) if form.startswith("qkv") else (2, 1)
        return dict(nw=8, col_tiles=ct, ksplit=ks, norm=True), int(form[-1]), ("parts" if ks > 1 else "rm"), False
    if form.startswith("qkv"):
        return dict(nw=8, norm=True), int(form[6]), "rm", False
    if form.startswith("o_res"):
        return dict(nw=8, res=True, half_tile=8 if "tile8" in form else False, flags=ops.gemv_flags(pre_epi=1) if "pre_epi" in form else 0), 0, ("pk" if pkd else "rm"), pkd
    if form.startswith("gu"):
        return dict(nw=8, norm=True, swiglu=True, flags=ops.gemv_flags(pre_epi="pre_epi" in form, shallow="shallow" in form)), 0, "pk", True
    if form == "down_ks1":
        return dict(nw=16 if K % 512 == 0 else 8, res=True, half_tile=8), 0, ("pk" if pkd else "rm"), pkd
    assert form == "down_ks4"
    ks = 4 if K % (32 * 4 * 4) == 0 else 2
    return dict(nw=4, ksplit=ks, half_tile=8), 0, "parts", pkd


def check_gemv_two_tile(dev, form, rows, K, N):
    """One two-tile launch of `form` on `rows` rows against two one-tile launches (rows 0 .. 15, rows 16 .. rows - 1) of the same geometry on the same operands:
    the output, the x_out image and the ssq words are torch.equal; at 17 and 31 rows the launch is repeated with the pad rows of every input image at
    FMAX / K, and every valid row comes back unchanged to the bit."""
    from chatterbox_amd import ops
    what = f"{form} rows {rows} K {K} N {N}"
    if form == "qkv_np1_refused":
        wp = ops.pack_gemv_weight(_r((N, K), 2).to(dev))
        for M in (16, rows):
            r16 = (M + 15) // 16 * 16
            with pytest.raises(Exception):
                ops.gemv(torch.zeros(r16, K, device=dev), wp, torch.zeros(M, N, device=dev), N=N, K=K, M=M, nw=8, w_packed=True, x_packed=True,
                         norm_w=torch.ones(K, device=dev), xpart=torch.zeros(1, r16, K, device=dev), x_out=torch.zeros(r16, K, device=dev))
        return
    geo, n_part, okind, pkd = _gemv_case(form, K, N)
    swiglu, norm, ks = bool(geo.get("swiglu")), bool(geo.pop("norm", False)), geo.get("ksplit", 1)
    res = bool(geo.pop("res", False))
    w = _r((2 * N if swiglu else N, K), 2, 1 / math.sqrt(K)).to(dev)
    wp = ops.pack_gemv_weight(w, swiglu=swiglu, half_tile=geo.get("half_tile", False))
    nw_ = (1 + 0.1 * _r((K,), 3)).to(dev) if norm else None
    if swiglu and N % 32:
        for M in (16, rows):  # the entry point refuses this width at every row count
            r16 = (M + 15) // 16 * 16
            with pytest.raises(Exception):
                ops.gemv(torch.zeros(r16, K, device=dev), wp, torch.zeros(r16, N, device=dev), N=N, K=K, M=M, w_packed=True, x_packed=True, norm_w=nw_, out_packed=True, **geo)
        return
    x = _r((rows, K), 1)
    parts = [_r((rows, K), 10 + j, 0.5) for j in range(n_part)]
    r0 = _r((rows, N), 5)

    def run(lo, M, pad):
        """rows lo .. lo + M - 1 as ONE launch: (out valid rows, x_out valid rows or None, ssq words or None)"""
        r16 = (M + 15) // 16 * 16
        kw = dict(geo)
        xi = pack_rows(x[lo:lo + M], r16, pad).to(dev)
        x_out = None
        if n_part:
            kw["xpart"] = torch.stack([pack_rows(p[lo:lo + M], r16, pad) for p in parts]).to(dev)
            kw["x_out"] = x_out = torch.zeros(r16, K, device=dev)
        ssq = None
        if kw.get("col_tiles") and ks > 1:
            kw["ssq_out"] = ssq = torch.full((ks, r16), -1.0, device=dev)
        lead = (ks,) if ks > 1 else ()
        if pkd and okind in ("pk", "parts"):
            out = torch.zeros(*lead, r16, N, device=dev)
            if res:
                out.copy_(pack_rows(r0[lo:lo + M], r16, pad))
        else:
            out = torch.zeros(*lead, M, N, device=dev)
            if res:
                out.copy_(r0[lo:lo + M])
        ops.gemv(xi, wp, out, N=N, K=K, M=M, w_packed=True, x_packed=True, norm_w=nw_, res=out if res else None, out_packed=bool(pkd and okind in ("pk", "parts")), **kw)
        o = out.detach().cpu()
        if pkd and okind in ("pk", "parts"):
            o = torch.stack([unpack_rows(t, M, N) for t in o.reshape(-1, r16, N)]).reshape(*lead, M, N)
        return o, None if x_out is None else unpack_rows(x_out, M, K), None if ssq is None else ssq.cpu()[:, :M]

    two = run(0, rows, 0.0)
    assert torch.isfinite(two[0]).all() and float(two[0].abs().max()) > 0, what
    for lo, M in _tiles(rows):
        one = run(lo, M, 0.0)
        assert torch.equal(two[0][..., lo:lo + M, :], one[0]), f"{what}: rows {lo} .. {lo + M - 1} differ from their one-tile launch"
        if n_part:
            assert torch.equal(two[1][lo:lo + M], one[1]), f"{what}: x_out rows {lo} .. differ from their one-tile launch"
            want = x[lo:lo + M].clone()
            for p in parts:
                want += p[lo:lo + M]
            assert torch.equal(one[1], want), f"{what}: x_out is x + the partial images in order"
        if two[2] is not None:
            assert torch.equal(two[2][:, lo:lo + M], one[2]), f"{what}: ssq words of rows {lo} .. differ from their one-tile launch"
    if rows % 16:
        poisoned = run(0, rows, FMAX / K)
        for a, b, name in zip(two, poisoned, ("out", "x_out", "ssq")):
            if a is not None:
                assert torch.equal(a, b), f"{what}: {name} changed with the pad rows at FMAX / K"


ATTN_ROWS = (18, 32)
ATTN_CTX = (1, 63, 64, 200)


def check_attn_two_tile(dev, rows, ctx, fold):
    """decode_attn_rope of `rows` rows x 2 heads at context `ctx` (the new token included) as one launch against the launches of rows 0 .. 15 and 16 .. rows - 1:
    packed outputs and the appended cache rows are torch.equal.  fold: q|k|v arrives as 4 split-K partial sums + sums of squares (the column-tile projection)."""
    from chatterbox_amd import ops
    H, D, max_ctx = 2, 128, 256
    what = f"attention rows {rows} ctx {ctx} fold {fold}"
    cos, sin = _r((max_ctx, 64), 1).to(dev), _r((max_ctx, 64), 2).to(dev)
    kc0, vc0 = _r((rows, H, max_ctx, 64), 3), _r((rows, H, max_ctx, 64), 4)
    qkv = _r((4, rows, 3 * D), 5) if fold else _r((rows, 3 * D), 5)
    r16 = (rows + 15) // 16 * 16
    ssq = (_r((4, r16), 6).abs() * D / 4 + 1.0) if fold else None
    pos = torch.full((rows,), ctx - 1, dtype=torch.int32)

    def run(lo, M):
        m16 = (M + 15) // 16 * 16
        kc, vc = kc0[lo:lo + M].clone().to(dev), vc0[lo:lo + M].clone().to(dev)
        out = torch.zeros(m16, D, device=dev)
        geom = ops.DecodeAttnGeom(dev, split=M * H < 128)
        kw = {}
        if fold:
            q = qkv[:, lo:lo + M].contiguous().to(dev)
            s = torch.zeros(4, m16)
            s[:, :M] = ssq[:, lo:lo + M]
            kw = dict(qkv_ssq=s.to(dev), rms_dim=D, rms_eps=1e-5)
        else:
            q = qkv[lo:lo + M].contiguous().to(dev)
        ops.decode_attn_rope(q, pos[lo:lo + M].contiguous().to(dev), cos, sin, kc, vc, out, 0.125, out_packed=True, geom=geom, **kw)
        return unpack_rows(out, M, D), kc.cpu()[:, :, ctx - 1], vc.cpu()[:, :, ctx - 1]

    two = run(0, rows)
    assert torch.isfinite(two[0]).all() and float(two[0].abs().max()) > 0, what
    for lo, M in _tiles(rows):
        one = run(lo, M)
        for a, b, name in zip(two, one, ("output", "appended K", "appended V")):
            assert torch.equal(a[lo:lo + M], b), f"{what}: {name} of rows {lo} .. {lo + M - 1} differs from the 16-row launch"


# ---------------------------------------------------------------------------------------------------------------- the engine
ENG_STEPS = 8
ENG_MODES = ("eager", "graph", "c_loop")


def _requests(B):
    import wide_batch_common as W
    from chatterbox_amd import synth
    conds, texts, _ = W.llama_requests(B)
    return conds, texts, synth.rand((W.LLAMA_MAX_B, ENG_STEPS), seed=12)[:B].clone()


def _stepwise(eng, conds, texts, u, mode, two_tile):
    """(logits (ENG_STEPS, rows, V) -- the prefill's and those of every decode step --, sampled ids) of one generate call in `mode`."""
    import wide_batch_common as W
    kw = dict(max_new_tokens=ENG_STEPS, uniforms=u, ban_eos=True, two_tile=two_tile, **W.SAMP)
    if mode == "eager":
        toks, logits = eng.generate(conds, texts, debug_logits=True, **kw)
        return logits.cpu(), [t.tolist() for t in toks]
    saved = eng.c_loop
    eng.c_loop = mode == "c_loop"
    try:
        if mode == "c_loop":  # advance() replays a torch-captured graph where the state holds one (an earlier mode's): drop it, so the steps below run the library's loop
            for key, st in eng._state.items():
                if key[0] == len(texts):
                    st["graph"] = None
        h = eng.generate(conds, texts, async_mode=True, run_steps=1, **kw)
        st, logits = h["st"], []
        assert ("cloop" in st and st["graph"] is None) if mode == "c_loop" else st["graph"] is not None, (mode, sorted(st))
        logits.append(st["logits"].clone())  # the prefill's: run_steps = 1 sampled from them and ran no decode step
        for _ in range(ENG_STEPS - 1):
            assert eng.advance(h, 1) == 1
            logits.append(st["logits"].clone())
        toks = eng.collect(h)
    finally:
        eng.c_loop = saved
    return torch.stack(logits).cpu(), [t.tolist() for t in toks]


def _reference(eng, B):
    """The B utterances decoded as batches of at most 8 (16 rows: one tile), eagerly: per utterance (logits (ENG_STEPS, 2, V), ids).  Computed once per device."""
    key = ("ref", str(eng.dev), B)
    if key not in _CACHE:
        conds, texts, u = _requests(B)
        ref = []
        for lo in range(0, B, 8):
            hi = min(B, lo + 8)
            logits, toks = _stepwise(eng, conds[lo:hi], texts[lo:hi], u[lo:hi], "eager", False)
            n = hi - lo
            ref += [(torch.stack([logits[:, b], logits[:, n + b]], 1), toks[b]) for b in range(n)]
        _CACHE[key] = ref
    return _CACHE[key]


def check_engine_two_tile(dev, B, mode):
    """T3Engine.generate(two_tile=True) of B utterances of unequal text lengths (2 B rows on the packed five-launch layer, two row tiles): the logits of rows b
    and B + b at each of ENG_STEPS steps are torch.equal to those of the same utterance in a batch of at most 8, and the sampled ids are the same."""
    import wide_batch_common as W
    eng = W._engine("llama", dev, W.LLAMA_L)
    conds, texts, u = _requests(B)
    assert len({int(t.numel()) for t in texts}) > 1
    if ("warm", str(dev)) not in _CACHE:  # every voice's prefix cached: the reference and the two-tile call prefill the text positions alone
        eng.generate(conds[:3], texts[:3], max_new_tokens=1, uniforms=u[:3], **W.SAMP)
        _CACHE[("warm", str(dev))] = True
    ref = _reference(eng, B)
    calls = W._counted(eng, W._LLAMA_FORMS)
    try:
        logits, toks = _stepwise(eng, conds, texts, u, mode, True)
        st = next(s for k, s in eng._state.items() if k[0] == B)
        assert st["rows"] == 2 * B > 16 and eng._packed_rows(st) and eng._use_c_step(st)
        assert calls["_forward_decode"] == 0, calls
    finally:
        W._uncounted(eng, W._LLAMA_FORMS)
    assert logits.shape[:2] == (ENG_STEPS, 2 * B)
    for b in range(B):
        got = torch.stack([logits[:, b], logits[:, B + b]], 1)
        for i in range(ENG_STEPS):
            assert torch.equal(got[i], ref[b][0][i]), (f"B = {B} ({mode}), utterance {b}, step {i}: logits differ from the batch of <= 8 by "
                                                      f"{float((got[i] - ref[b][0][i]).abs().max()):.3e}")
        assert toks[b] == ref[b][1], f"B = {B} ({mode}), utterance {b}: ids {toks[b]} vs {ref[b][1]}"


# ---------------------------------------------------------------------------------------------------------------- the throughput schedule
def check_schedule_pairs(dev):
    """Three jobs of 2 utterances on a tiny engine (job 1 with seeds of its own, job 2 with a temperature of its own): synthesize_pipelined(t3_pair=True) -- jobs 0
    and 1 as one 8-row T3 call, job 2 alone -- yields the tokens and waveforms of t3_pair=False in the same order; with a guard on job 1 nothing pairs with it
    and its report is its own."""
    from chatterbox_amd import synth
    from chatterbox_amd.engine import ChatterboxEngine
    L, steps, P = 2, 10, 6
    eng = ChatterboxEngine(synth.t3_state_dict(L, 0), synth.s3gen_state_dict(0, n_mid=1, n_enc=1, n_up_enc=1), dev, n_t3_layers=L)
    cond, ref = synth.t3_cond(), synth.s3gen_ref(n_prompt_tokens=P)

    def jobs(guard_on=None):
        out = []
        for j in range(3):
            texts = [synth.text_tokens(8 + 3 * j, seed=10 + j), synth.text_tokens(12, seed=20 + j)]
            # (every draw -- T3's uniforms, the flow's z, the vocoder's phase and noise -- comes from the job's seeds: a guarded job's length is not known here)
            job = dict(text_tokens=texts, t3_conds=cond, gen_ref=ref, seeds=[100 + j, 200 + j] if j == 1 else 7)
            if j == 2:
                job["temperature"] = [0.7, 0.9]
            if guard_on == j:
                job["guard"] = dict(heads=((1, 0), (1, 3)))
            out.append(job)
        return out

    calls = []
    gen = eng.t3.generate
    eng.t3.generate = lambda *a, **k: (calls.append((len(k.get("text_tokens", a[1] if len(a) > 1 else ())), bool(k.get("two_tile")), "guard" in k)), gen(*a, **k))[1]
    try:
        for guard_on in (None, 1):
            kw = dict(max_new_tokens=steps, n_cfm_timesteps=2, **({} if guard_on is not None else dict(ban_eos=True, ban_from=6561)),
                      temperature=0.8, top_p=1.0, min_p=0.05, repetition_penalty=1.2, cfg_weight=0.5)
            res, reports = {}, {}
            for pair in (False, True):
                del calls[:]
                res[pair], reports[pair] = [], []
                for wavs, toks, lat in eng.synthesize_pipelined(jobs(guard_on), t3_pair=pair, **kw):
                    res[pair].append((wavs, toks))
                    reports[pair].append(eng.last_guard)
                want = [2, 2, 2] if (not pair or guard_on is not None) else [4, 2]
                assert [c[0] for c in calls] == want, (pair, guard_on, calls)
                assert [c[1] for c in calls] == [pair and n == 4 for n in want]
            assert len(res[True]) == len(res[False]) == 3
            for j in range(3):
                assert [t.tolist() for t in res[True][j][1]] == [t.tolist() for t in res[False][j][1]], f"job {j} (guard on job {guard_on}): tokens"
                for a, b in zip(res[True][j][0], res[False][j][0]):
                    assert torch.equal(a, b), f"job {j} (guard on job {guard_on}): waveforms differ between t3_pair=True and False"
                assert (reports[True][j] is None) == (guard_on != j) and (reports[False][j] is None) == (guard_on != j)
                if guard_on == j:
                    assert len(reports[True][j]) == 2 and repr(reports[True][j]) == repr(reports[False][j]), "the guarded job's report is its own"
    finally:
        eng.t3.generate = gen
