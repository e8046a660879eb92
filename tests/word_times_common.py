"""Shared by test_word_times_host.py (SIMT emulator), test_turbo_stream_word_times_kernels_gpu.py and test_word_times_api_gpu.py: NumPy restatements of the two
word-timestamp kernels (include/cbx.h cbx_attn_text_mass_f32 / cbx_align_path_f32) -- the text mass in fp64 (the full causal softmax, then
the column slice, then the head sum), the path recurrence in fp32 exactly as the header states it -- the case tables of the kernel tests, and an fp64 restatement
of the Llama layers the alignment pass runs, pinned against oracle.ref_torch.llama_forward (a read-only import)."""
import ctypes

import numpy as np
import torch

MASS_TOL = 2e-5   # |err| <= MASS_TOL * (1 + |ref|): the project's tolerance for fp32 attention kernels (test_softmax_stress_gpu.py)
QW, KT = 4, 64    # attn_align.hip: queries of a wave (TM_QW), keys / text columns of a tile (TM_KT)
CHUNK = 64        # attn_align.hip: frames of move words staged for the walk back (AP_CHUNK); a wave of the path kernel owns 64 columns


def mass_ref(q, k, heads, q_len, ctx0, t0, t_len, scale, weight):
    """q (Z, Tq, H, 64), k (Z, Tk, H, 64) arrays -> list of Z fp64 arrays (q_len[z], t_len[z]): weight * sum over heads of softmax_j(scale q_i . k_j)[t0 + t],
    the softmax over the keys j <= ctx0 + i.  Keys beyond are never touched."""
    out = []
    for z in range(len(q_len)):
        res = np.zeros((q_len[z], t_len[z]))
        for i in range(q_len[z]):
            vis = ctx0[z] + i + 1
            for h in heads:
                s = scale * (k[z, :vis, h].astype(np.float64) @ q[z, i, h].astype(np.float64))
                p = np.exp(s - s.max())
                p /= p.sum()
                res[i] += p[t0[z]: t0[z] + t_len[z]]
        out.append(weight * res)
    return out


def path_ref(score, n, m):
    """The fp32 recurrence of cbx_align_path_f32 on score[:n, :m] -> (spans (m, 2) int32, frame_tok (n,) int32)."""
    s = np.asarray(score, dtype=np.float32)[:n, :m]
    ninf = np.float32(-np.inf)
    D = np.full(m, ninf, dtype=np.float32)
    D[0] = s[0, 0]
    move = np.zeros((n, m), dtype=bool)
    for i in range(1, n):
        diag = np.concatenate([np.array([ninf], dtype=np.float32), D[:-1]])
        move[i] = diag > D
        D = (s[i] + np.where(move[i], diag, D)).astype(np.float32)
    e = m - 1 if n >= m else int(np.argmax(D[:n]))  # (argmax: the lowest index of the largest value)
    frame_tok = np.zeros(n, dtype=np.int32)
    t = e
    for i in range(n - 1, -1, -1):
        frame_tok[i] = t
        t -= int(move[i, t])
    spans = np.full((m, 2), n, dtype=np.int32)
    for tok in range(e + 1):
        fr = np.nonzero(frame_tok == tok)[0]
        spans[tok] = (fr[0], fr[-1] + 1)
    return spans, frame_tok


# ---- case tables.  Mass: (name, H, heads, rows of (q_len, ctx0, t0, t_len)); every q_len / context is placed around the kernel's tile sizes: QW = 4 queries per
# wave (3, 4, 5), KT = 64 keys per tile in pass 1 (contexts 63, 64, 65, 127, 128, 129) and 64 text columns per tile in pass 2 (t_len 63, 64, 65)
MASS_CASES = [
    ("one query, one key, one text column: p = 1", 1, [0], [(1, 0, 0, 1)]),
    ("t_len = 1 at t0 = 0", 2, [1], [(3, 4, 0, 1)]),
    ("t_len = 1 at t0 > 0", 2, [1], [(3, 4, 3, 1)]),
    ("q_len = 0 beside a full row", 2, [0], [(0, 5, 1, 2), (5, 5, 1, 2)]),
    ("n_sel = 3", 4, [3, 0, 2], [(5, 9, 2, 6)]),
    ("a repeated head", 4, [1, 1, 2], [(5, 9, 2, 6)]),
    ("queries 3 / 4 / 5 around the wave's 4", 2, [0, 1], [(3, 7, 1, 5), (4, 7, 1, 5), (5, 7, 1, 5)]),
    ("contexts 63 / 64 / 65 around the key tile", 2, [1], [(2, 61, 3, 20), (2, 62, 3, 20), (2, 63, 3, 20)]),
    ("contexts 127 / 128 / 129: a second key tile", 2, [0], [(3, 124, 10, 30), (3, 125, 10, 30), (3, 126, 10, 30)]),
    ("text columns 63 / 64 / 65 around the column tile", 2, [1, 0], [(2, 70, 2, 63), (2, 70, 2, 64), (2, 70, 2, 65)]),
    ("ragged rows: other ctx0, t0, t_len, q_len in one launch", 3, [2, 0], [(9, 40, 34, 7), (1, 3, 0, 4), (6, 140, 5, 70), (13, 20, 20, 1)]),
]

PATH_SHAPES = [(1, 1), (1, 3), (2, 3), (3, 3), (5, 2), (7, 1), (64, 65), (65, 64), (130, 33)]   # the issue's list; the kernel tests add (1000, 1024) on the GPU


def mass_inputs(H, rows, seed, spread=1.0):
    """q (Z, Tq, H, 64), k (Z, Tk, H, 64) fp32 arrays for the rows of a case; scores scale * q . k of about +-spread * 3."""
    g = np.random.default_rng(seed)
    Z, Tq, Tk = len(rows), max(1, max(r[0] for r in rows)), max(r[0] + r[1] for r in rows) + 3  # (three keys nobody sees)
    q = (g.standard_normal((Z, Tq, H, 64)) * spread).astype(np.float32)
    k = g.standard_normal((Z, Tk, H, 64)).astype(np.float32)
    return q, k


def run_mass(ops, dev, q, k, heads, rows, scale=0.125, weight=1.0, accumulate=False, mass=None, poison=False, cache_layout=True):
    """ops.attn_text_mass on `dev` over the rows of a case.  k travels as a view of a [row][head][Tk][64] cache (its own head stride) unless cache_layout is
    False; poison: every key a query does not see is NaN for THAT query -- keys beyond ctx0 + q_len - 1 of a row -- and keys inside the row's context stay."""
    ql, c0, t0, tl = ([r[i] for r in rows] for i in range(4))
    kk = k.copy()
    if poison:
        for z in range(len(rows)):
            kk[z, c0[z] + ql[z]:] = np.nan
    qt = torch.from_numpy(q).to(dev)
    kt = torch.from_numpy(kk).to(dev)
    if cache_layout:
        kt = kt.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    if mass is None:
        mass = torch.full((len(rows), max(1, max(ql)) + 2, max(tl) + 3), -7.0, device=dev)
    ops.attn_text_mass(qt, kt, mass, heads, ql, c0, t0, tl, scale, weight=weight, accumulate=accumulate)
    return mass


def check_mass(mass, ref, rows, sentinel=-7.0, tol=MASS_TOL):
    """mass (Z, I, T) against the restatement's list; everything outside [q_len) x [t_len) still holds the sentinel.  Returns the largest err / (1 + |ref|)."""
    got = mass.detach().cpu().numpy().astype(np.float64)
    worst = 0.0
    for z, r in enumerate(rows):
        a = got[z, :r[0], :r[3]]
        assert np.isfinite(a).all(), (z, "not finite")
        if a.size:
            worst = max(worst, float((np.abs(a - ref[z]) / (1.0 + np.abs(ref[z]))).max()))
        outside = got[z].copy()
        outside[:r[0], :r[3]] = sentinel
        assert (outside == sentinel).all(), (z, "written outside [q_len) x [t_len)")
    assert worst <= tol, worst
    return worst


def path_scores(n, m, seed, kind="random"):
    """random: N(0, 1); halves: quantised to multiples of 0.5 in [0, 2], so that ties are common; diagonal: 1 on the cells of a known path, 0 elsewhere."""
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.standard_normal((n, m)).astype(np.float32)
    if kind == "halves":
        return (g.integers(0, 5, (n, m)) * 0.5).astype(np.float32)
    assert kind == "diagonal" and n >= m
    s = np.zeros((n, m), dtype=np.float32)
    s[np.arange(n), diagonal_tok(n, m)] = 1.0
    return s


def diagonal_tok(n, m):
    """the token of frame i on the path the diagonal-dominant matrix is built around: token t owns frames [ceil(t n / m), ceil((t + 1) n / m))"""
    return (np.arange(n) * m) // n


def run_path(ops, dev, scores, pad=(2, 3)):
    """ops.align_path over a list of (n, m) score arrays in ONE launch, rows padded to a common (N + pad, M + pad) with NaN beyond each row's own (n, m)."""
    ns, ms = [s.shape[0] for s in scores], [s.shape[1] for s in scores]
    buf = np.full((len(scores), max(ns) + pad[0], max(ms) + pad[1]), np.nan, dtype=np.float32)
    for z, s in enumerate(scores):
        buf[z, :ns[z], :ms[z]] = s
    spans, frame_tok = ops.align_path(torch.from_numpy(buf).to(dev), ns, ms)
    return spans.cpu().numpy(), frame_tok.cpu().numpy()


def check_path(spans, frame_tok, scores):
    """bit-exact against path_ref row by row; nothing written beyond m[z] pairs / n[z] frames (ops.align_path hands out zeros)"""
    for z, s in enumerate(scores):
        n, m = s.shape
        sp, ft = path_ref(s, n, m)
        assert np.array_equal(frame_tok[z, :n], ft), (z, n, m, "frame_tok")
        assert np.array_equal(spans[z, :m], sp), (z, n, m, "spans")
        assert (frame_tok[z, n:] == 0).all() and (spans[z, m:] == 0).all(), (z, "written beyond the row")
        assert ft[0] == 0 and (np.diff(ft) >= 0).all() and (np.diff(ft) <= 1).all(), "the path starts at token 0 and moves by 0 or 1"
        if n >= m:
            assert ft[-1] == m - 1 and (sp[:, 1] > sp[:, 0]).all(), "n >= m: the path ends at m - 1 and every span is non-empty"


def c_ints(a):
    return (ctypes.c_int * len(a))(*a)


# ---- the Llama layers of the alignment pass in fp64 (RMSNorm, q/k/v, RoPE, causal attention, o, SwiGLU MLP), pinned against oracle.ref_torch.llama_forward
def rope64(x, cos, sin):
    """x (S, H, 64) fp64; cos / sin (S, 64): HF rotate_half"""
    x1, x2 = x[..., :32], x[..., 32:]
    return x * cos[:, None, :] + np.concatenate([-x2, x1], -1) * sin[:, None, :]


def _rms64(x, w, eps, oracle_norm):
    """RMSNorm in fp64; oracle_norm: the mean square and its rsqrt in fp32, as oracle.ref_torch.rms_norm computes them whatever the input's type (x.float()) --
    only for the pin against that function: the restatement the engine is compared with stays fp64 throughout"""
    if oracle_norm:
        v = torch.from_numpy(x).float().pow(2).mean(-1, keepdim=True)
        return w * (x * torch.rsqrt(v + eps).numpy())
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def llama_layers64(x, layers, cos, sin, H, upto=None, eps=1e-5, oracle_norm=False):
    """x (S, D) fp64 input embeddings of ONE sequence at positions 0 .. S - 1; layers: dicts of fp64 arrays ln1, ln2, wq, wk, wv, wo, wg, wu, wd (torch Linear
    layout (out, in)).  Returns (hidden states after the last layer run, [(q, k) after RoPE of every layer run, each (S, H, 64)])."""
    S, D = x.shape
    qk = []
    mask = np.triu(np.ones((S, S), dtype=bool), 1)
    for lw in layers[:upto]:
        h = _rms64(x, lw["ln1"], eps, oracle_norm)
        q = rope64((h @ lw["wq"].T).reshape(S, H, 64), cos, sin)
        k = rope64((h @ lw["wk"].T).reshape(S, H, 64), cos, sin)
        v = (h @ lw["wv"].T).reshape(S, H, 64)
        qk.append((q, k))
        s = np.einsum("ihd,jhd->hij", q, k) * 0.125
        s[:, mask] = -np.inf
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        att = np.einsum("hij,jhd->ihd", p, v).reshape(S, D)
        x = x + att @ lw["wo"].T
        h = _rms64(x, lw["ln2"], eps, oracle_norm)
        g = h @ lw["wg"].T
        x = x + ((g / (1.0 + np.exp(-g))) * (h @ lw["wu"].T)) @ lw["wd"].T
    return x, qk
