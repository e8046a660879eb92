"""Shared by test_guard_host.py (SIMT emulator), test_turbo_stream_guard_kernels_gpu.py and test_guard_api_gpu.py: restatements of the two alignment-guard kernels
(include/cbx.h cbx_guard_text_mass_f32 / cbx_guard_update_f32) -- the text mass of the current decode query in fp64 from (q parts, ssq, cos /
sin, K, position), on word_times_common.mass_ref; the update as a NumPy fp32 state machine with the order of adds and compares of the header --, designed mass
trajectories, and the runners of the two ops wrappers."""
import numpy as np
import torch

import word_times_common as W

MASS_TOL = W.MASS_TOL
EOS, V = 6562, 8194
T0 = 34
NTHR = 8
DEFAULTS = dict(back=3, ahead=6, end_tokens=3, tail=5.0, repeat=5.0, repeat_skip=5, token_run=3, hold_eos=True, min_text=6)
OFF = dict(tail=float("inf"), repeat=float("inf"), token_run=0, hold_eos=False)  # every rule off: the hooks only read


def thr_row(**kw):
    """the eight thresholds of one utterance as the device holds them"""
    g = dict(DEFAULTS, **kw)
    return [g["back"], g["ahead"], g["end_tokens"], g["tail"], g["repeat"], g["repeat_skip"], g["token_run"], g["min_text"] if g["hold_eos"] else -1]


# ----------------------------------------------------------------------------- the mass of the current query
def guard_q64(qkv, nparts, ssq, rms_dim, rms_eps, cos, sin, b, head, pos, H):
    """q of conditional row b, head `head`, in fp64: the parts added in part order, rstd, RoPE at pos.  qkv (rows, 3 H 64) or (nparts, rows, 3 H 64)."""
    if nparts > 1:
        q = sum(qkv[j, b, head * 64: head * 64 + 64].astype(np.float64) for j in range(nparts))
        q = q / np.sqrt(sum(float(ssq[j, b]) for j in range(nparts)) / rms_dim + rms_eps)
    else:
        q = (qkv[0] if qkv.ndim == 3 else qkv)[b, head * 64: head * 64 + 64].astype(np.float64)
    if cos is None:
        return q
    c, s = cos[pos].astype(np.float64), sin[pos].astype(np.float64)
    return q * c + np.concatenate([-q[32:], q[:32]]) * s


def guard_mass_ref(qkv, nparts, ssq, rms_dim, rms_eps, cos, sin, kc, positions, heads, t_len, t0, scale, H):
    """p[s][b] (fp64 arrays of t_len[b]) for every selected head s and conditional row b: the softmax over the keys j <= positions[b], then the text columns.
    kc (rows, H, max_ctx, 64); keys beyond positions[b] are never touched."""
    out = []
    for h in heads:
        row = []
        for b in range(len(t_len)):
            pos = int(positions[b])
            q = guard_q64(qkv, nparts, ssq, rms_dim, rms_eps, cos, sin, b, h, pos, H)
            k = kc[b, h, : pos + 1][None, :, None, :]                      # (1, Tk, 1, 64)
            row.append(W.mass_ref(q[None, None, None, :], k, [0], [1], [pos], [t0], [int(t_len[b])], scale, 1.0)[0][0])
        out.append(row)
    return out


def mass_case(B, H, ctx, t_len, nparts, seed, spread=1.0, rope=True, max_ctx=None, poison=True):
    """Inputs of one mass launch: conditional row b at context ctx[b] (an int: every row; positions = ctx - 1) with t_len text columns at T0.  qkv and ssq are
    ALWAYS the full 4-part buffers, (4, rows, 3 H 64) and (4, 16); run_mass hands the kernel a view of the first nparts parts of the device copy, so what lies
    behind them is in device memory.  poison: NaN in the cache beyond each row's context, in the unconditional rows' q, in the parts >= nparts of qkv and ssq and
    in the ssq entries of the rows >= B."""
    g = np.random.default_rng(seed)
    ctxs = [int(ctx)] * B if np.isscalar(ctx) else [int(v) for v in ctx]
    rows, max_ctx = 2 * B, max_ctx or max(ctxs) + 3
    P = max(nparts, 1)
    qkv = (g.standard_normal((4, rows, 3 * H * 64)) * spread).astype(np.float32)
    ssq = (g.uniform(0.5, 1.5, (4, 16)) * 256 / P).astype(np.float32)
    kc = g.standard_normal((rows, H, max_ctx, 64)).astype(np.float32)
    cos = sin = None
    if rope:
        ang = g.uniform(0, 2 * np.pi, (max_ctx, 32))
        cos, sin = np.cos(np.concatenate([ang, ang], 1)).astype(np.float32), np.sin(np.concatenate([ang, ang], 1)).astype(np.float32)
    if poison:
        for r in range(rows):
            kc[r, :, ctxs[r % B]:] = np.nan
        qkv[P:] = np.nan
        qkv[:, B:, : H * 64] = np.nan
        ssq[P:] = np.nan
        ssq[:, B:] = np.nan
    positions = np.asarray([c - 1 for c in ctxs] * 2, dtype=np.int32)
    return dict(B=B, H=H, qkv=qkv, nparts=nparts, ssq=ssq, rms_dim=256, rms_eps=1e-5, cos=cos, sin=sin, kc=kc, positions=positions,
                t_len=np.full(B, t_len, dtype=np.int32) if np.isscalar(t_len) else np.asarray(t_len, dtype=np.int32), max_ctx=max_ctx)


def run_mass(ops, dev, c, heads, done=None, sentinel=-7.0, slots=None, t_cap=None):
    """ops.guard_text_mass on `dev` over a mass_case -> p (slots, B, t_cap) as an array; untouched elements hold the sentinel.  The whole 4-part qkv and the
    (4, 16) ssq go to the device; the kernel gets the strided view [:nparts] of each (nparts 0: part 0 alone, no ssq), the poison right behind it."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, P = c["B"], c["nparts"]
    t_cap = t_cap or min(1024, int(max(c["t_len"].max(), 1)) + 3)   # (1024: the kernel's cap -- such a row has no column beyond its text)
    p = torch.full((slots or len(heads), B, t_cap), sentinel, device=dev)
    done = np.zeros(B, dtype=np.int32) if done is None else np.asarray(done, dtype=np.int32)
    qkv4, ssq4 = t(c["qkv"]), t(c["ssq"])
    assert qkv4.shape[0] == 4 and tuple(ssq4.shape) == (4, 16)
    qkv, ssq = (qkv4[:P], ssq4[:P]) if P > 1 else (qkv4[0], None)
    ops.guard_text_mass(qkv, t(c["positions"]), t(c["cos"]), t(c["sin"]), t(c["kc"]), heads, t(done), t(c["t_len"]), T0, 0.125, p, qkv_ssq=ssq,
                        rms_dim=c["rms_dim"] if P > 1 else 0, rms_eps=c["rms_eps"], max_ctx=c["max_ctx"])
    return p.cpu().numpy()


def check_mass(p, c, heads, done=None, sentinel=-7.0, tol=MASS_TOL):
    """p against the fp64 restatement within tol (1 + |ref|); done rows, columns beyond t_len and slots beyond the heads keep the sentinel.  Returns the worst figure."""
    ref = guard_mass_ref(c["qkv"], c["nparts"], c["ssq"], c["rms_dim"], c["rms_eps"], c["cos"], c["sin"], c["kc"], c["positions"], heads, c["t_len"], T0, 0.125, c["H"])
    worst = 0.0
    for s in range(p.shape[0]):
        for b in range(c["B"]):
            n = int(c["t_len"][b]) if s < len(heads) and not (done is not None and done[b]) else 0
            assert (p[s, b, n:] == sentinel).all(), (s, b, "written beyond the row's text columns, or by a row that is done")
            if n:
                got = p[s, b, :n].astype(np.float64)
                assert np.isfinite(got).all(), (s, b, "not finite")
                worst = max(worst, float((np.abs(got - ref[s][b]) / (1.0 + np.abs(ref[s][b]))).max()))
    assert worst <= tol, worst
    return worst


# ----------------------------------------------------------------------------- the update: fp32 state machine
def new_state(B):
    return dict(state=np.zeros((B, 8), dtype=np.int32), sums=np.zeros((B, 4), dtype=np.float32))


def update_ref(st, b, a, m, i, thr, tokens, done=False):
    """One step of utterance b on the fp32 mass row a[:m] (what the device stored to its history): the header's steps 2 .. 8 with its order of adds and
    compares.  st: new_state's dict, updated in place; tokens: the utterance's sampled tokens so far (index i - 1 is the last).  Returns None when the row does
    nothing (done, fired, or outside the caps), else dict(trace, ban, reason)."""
    s, f = st["state"][b], st["sums"][b]
    if done or s[3] or not 1 <= m <= 1024 or i < 0:
        return None
    back, ahead, rskip, token_run, hold_min = int(thr[0]), int(thr[1]), int(thr[5]), int(thr[6]), int(thr[7])
    et = min(max(int(thr[2]), 1), 3)
    a = np.asarray(a, dtype=np.float32)[:m]
    cur = int(np.argmax(a))                                   # the lowest t with the largest a[t]
    if -back <= cur - int(s[0]) <= ahead:
        s[0] = cur
    if not s[1] and s[0] >= m - et:
        s[1], s[2] = 1, i
    nt = min(et, m)
    first = m - nt
    if s[1]:
        for j in range(nt):
            f[j] = np.float32(f[j] + a[first + j])
        f[3] = np.float32(f[3] + (a[: m - rskip].max() if m - rskip > 0 else np.float32(0.0)))
    tail_max = max(float(f[j]) for j in range(nt))
    run = token_run > 0 and i >= token_run and len(set(int(t) for t in tokens[i - token_run: i])) == 1
    reason = 1 if s[1] and tail_max >= np.float32(thr[3]) else 2 if s[1] and float(f[3]) >= np.float32(thr[4]) else 3 if run else 0
    ban = -1
    if reason:
        s[3], s[4] = reason, i
    elif hold_min >= 0 and m >= hold_min and not s[1]:
        ban = EOS
    return dict(trace=int(s[0]) | int(s[1]) << 16 | (1 if ban >= 0 else 0) << 17 | reason << 18, ban=ban, reason=reason)


def first_ban(m, thr):
    """the ban frame 0 is sampled under (the host writes it): pos = 0, complete iff 0 >= m - end_tokens"""
    et = min(max(int(thr[2]), 1), 3)
    return EOS if int(thr[7]) >= 0 and m >= int(thr[7]) and m > et else -1


def replay(mass, tokens, m, thr, n_steps):
    """The state machine over one utterance's history mass[i][:m] and its tokens for the steps i = 1 .. n_steps - 1 that ran (tokens[i] exists): (trace list
    indexed by step, final state row, final sums row).  A step behind EOS does not run: the sampler set done."""
    st = new_state(1)
    trace = [0] * n_steps
    for i in range(1, n_steps):
        if i >= len(tokens) or int(tokens[i - 1]) == EOS:
            break
        r = update_ref(st, 0, mass[i], m, i, thr, tokens)
        if r is None:
            break
        trace[i] = r["trace"]
    return trace, st["state"][0], st["sums"][0]


# ---- designed trajectories: mass rows with one dominant column per step
def peaked(m, cols, peak=0.6):
    """(len(cols), m) fp32: step i puts `peak` on column cols[i] and spreads 0.2 over the others"""
    a = np.full((len(cols), m), 0.2 / max(m - 1, 1), dtype=np.float32)
    for i, c in enumerate(cols):
        a[i, c] = peak
    return a


def head_mean(a, n_sel):
    """what the kernel makes of n_sel slots that all hold a: the fp32 sum in slot order, times the fp32 weight 1 / n_sel"""
    a = np.asarray(a, dtype=np.float32)
    s = np.zeros_like(a)
    for _ in range(n_sel):
        s = (s + a).astype(np.float32)
    return (np.float32(1.0) / np.float32(n_sel) * s).astype(np.float32)


def run_update(ops, dev, a_rows, m, i, thr, st, tokens, done=None, n_sel=2, ld=None, max_steps=None, logits=None, sentinel=-3.0):
    """ONE ops.guard_update launch for B utterances at step i[b].  Every one of the n_sel slots of p holds a_rows[b] (NaN beyond m[b]), so the device's a is
    head_mean(a_rows[b], n_sel).  st: new_state's arrays (host), updated from the device.  Returns dict(mass history, trace, dp = the sampler rows, logits)."""
    B = len(m)
    ld = ld or int(max(max(m), 1)) + 3
    ld4 = (ld + 3) // 4 * 4
    max_steps = max_steps or int(max(i)) + 2
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    p = torch.full((n_sel, B, ld4), float("nan"), device=dev)
    for b in range(B):
        for s in range(n_sel):
            p[s, b, : m[b]] = t(np.asarray(a_rows[b], dtype=np.float32)[: m[b]])
    mass = torch.full((B, max_steps, ld4), sentinel, device=dev)
    trace = torch.full((B, max_steps), -9, dtype=torch.int32, device=dev)
    out_tokens = torch.zeros(B, max_steps, dtype=torch.int64, device=dev)
    for b in range(B):
        tk = list(tokens[b])[: max_steps]
        out_tokens[b, : len(tk)] = torch.tensor(tk, dtype=torch.int64)
    ldl = V + 6
    lg = torch.full((2 * B, ldl), 1.5, device=dev) if logits is None else logits
    dp = torch.full((B, 8), 0.25, device=dev)
    state, sums = t(st["state"]), t(st["sums"])
    done = np.zeros(B, dtype=np.int32) if done is None else np.asarray(done, dtype=np.int32)
    ops.guard_update(p, t(np.asarray(m, dtype=np.int32)), t(np.asarray(i, dtype=np.int32)), t(done), t(np.asarray(thr, dtype=np.float32)), out_tokens, mass, state, sums,
                     trace, lg, V, EOS, dp)
    st["state"][:], st["sums"][:] = state.cpu().numpy(), sums.cpu().numpy()
    return dict(mass=mass.cpu().numpy(), trace=trace.cpu().numpy(), dp=dp.cpu().numpy(), logits=lg.cpu().numpy(), sentinel=sentinel)


def drive(ops, dev, cols, m, thr, tokens, n_sel=2, peak=0.6, tie=False):
    """ops.guard_update step by step over peaked(m, cols) beside the state machine: history row, trace, ban column, state, sums and forced logits are compared
    exactly at every step; returns the step that fired (None: none).  tie: every step has two equal largest columns."""
    a = peaked(m, [0] + list(cols), peak)
    if tie:  # a second column two to the right holds the same peak: the lowest t wins
        for i, c in enumerate([0] + list(cols)):
            a[i, c + 2] = a[i, c]
    st_d, st_r = new_state(1), new_state(1)
    fired = None
    for i in range(1, len(cols) + 1):
        r = update_ref(st_r, 0, head_mean(a[i], n_sel), m, i, thr, tokens)
        d = run_update(ops, dev, [a[i]], [m], [i], [thr], st_d, [tokens], n_sel=n_sel, max_steps=len(cols) + 2)
        assert np.array_equal(st_d["state"], st_r["state"]) and np.array_equal(st_d["sums"], st_r["sums"]), (i, st_d, st_r)
        if r is None:
            assert (d["mass"] == d["sentinel"]).all() and (d["trace"] == -9).all() and (d["dp"] == 0.25).all() and (d["logits"] == 1.5).all(), "a fired row does nothing"
            continue
        assert np.array_equal(d["mass"][0, i, :m], head_mean(a[i], n_sel)) and (d["mass"][0, i, m:] == d["sentinel"]).all()
        assert (np.delete(d["mass"][0], i, 0) == d["sentinel"]).all() and d["trace"][0, i] == r["trace"] and (np.delete(d["trace"][0], i) == -9).all()
        assert d["dp"][0, 6] == r["ban"] and (np.delete(d["dp"][0], 6) == 0.25).all(), "only the ban column of the sampler's row is written"
        want = np.where(np.arange(V) == EOS, 32768.0, 0.0) if r["reason"] else np.full(V, 1.5)
        assert (d["logits"][:, :V] == want).all() and (d["logits"][:, V:] == 1.5).all(), "both CFG rows forced, the padding untouched"
        if r["reason"]:
            fired = i
    return fired
