"""Shared by tests/test_loudness_push_host.py (SIMT emulator, CPU tensors) and tests/test_turbo_stream_loudness_push_kernels_gpu.py: the cases of the running meter
(include/cbx.h cbx_wave_loudness_push_f32; ops.wave_loudness_push, ops.WaveLoudnessStream) and run_split, which feeds signals to a meter piece by piece.  Not a test
module.

The contract is BITWISE: after every push stats and gain are compared as bit patterns with ops.wave_loudness over each row's concatenation so far, on the same
device; no tolerance is involved.  After the last push the numbers also go through loudness_common.check_stats against the SciPy oracle, with that module's own
tolerances and its gate-margin assertion -- hence the final signals are bursts(25234, 10 + 25234) and bursts(72007, 10 + 72007), which tests/test_loudness_host.py
asserts stay >= 1 LU from both gates.  Prefixes are compared only bitwise, so their margins do not matter.

Splits, at hop = 2400 -- the smallest shapes at which a push can go wrong: one push; [1, 2399, 1, 2400, 4799, 0, 7, rest] (a piece that stays inside the tail, one
that completes a segment exactly, an empty one, one that spans segments with a tail on both sides); pieces of 1000 (K alternates between 0 and 1); pieces of 2400."""
import ctypes

import numpy as np
import torch

import loudness_common as C

HOP = 2400
N_SHORT, N_LONG = 25234, 72007
REST = None


def short():
    return C.bursts(N_SHORT, 10 + N_SHORT)


def long():
    return C.bursts(N_LONG, 10 + N_LONG)


def pieces_of(n, step):
    return [step] * (n // step) + ([n % step] if n % step else [])


SPLITS_ONE = dict(one_push=[REST], ragged=[1, 2399, 1, 2400, 4799, 0, 7, REST], thousands=pieces_of(N_SHORT, 1000), hops=pieces_of(N_SHORT, 2400))
# R = 3: different lengths per push, a row that is empty in some pushes (0, and 2 at its start), a row that ends early (1)
SPLITS_THREE = [[5000, 0, 30000, 1, REST], [10000, REST], [0, 1, 2399, 0, REST]]
TARGETS_THREE = (-30.0, None, -23.0)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def one_shot_energies(ops, rows, device):
    """The E table cbx_wave_loudness_f32 leaves in its workspace for `rows` (views of one buffer): a list of R host arrays of floor(n_r / hop) doubles"""
    base, offs, lens = ops._wave_rows(rows, "one_shot_energies")
    R, f = len(lens), ops.loudness_filter(C.FS)
    ld = -(-max(lens) // f["hop"])
    ws = torch.zeros(max(1, 6 * R * ld), dtype=torch.float64, device=device)
    stats = torch.empty(R, 4, dtype=torch.float64, device=device)
    gain = torch.empty(R, dtype=torch.float32, device=device)
    coef, tg = (ctypes.c_double * 10)(*f["coef"].tolist()), (ctypes.c_double * R)(*[float("nan")] * R)
    rc = ops.lib.cbx_wave_loudness_f32(base, ctypes.addressof(offs), ctypes.addressof(lens), R, ctypes.addressof(coef), f["hop"], ctypes.addressof(tg), 1.0,
                                       stats.data_ptr(), gain.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    assert rc == 0
    return ws, [(4 * R + r) * ld for r in range(R)], [int(n) // f["hop"] for n in lens]


def run_split(ops, signals, splits, targets, mis, device="cpu", sync=lambda: None, seg_cap=4096, oracle=True, ceiling=1.0):
    """Feed signals[r] to ONE ops.WaveLoudnessStream in pieces of splits[r] (REST: what is left; a row whose list is spent gets empty pieces).  Rows of a push are
    views of one NaN-filled buffer at misalignment `mis` (loudness_common.padded_rows).  After EVERY push: stats / gain bitwise equal to ops.wave_loudness over the
    rows' concatenation so far, the padding still NaN, the input tail unchanged.  After the last one: the E table bitwise the one-shot kernel's, and (oracle) the
    numbers against the SciPy oracle.  Returns the list of (stats, gain) host arrays per push."""
    R = len(signals)
    signals = [np.asarray(s, np.float32) for s in signals]
    meter = ops.WaveLoudnessStream(R, device, C.FS, seg_cap)
    done, out = [0] * R, []
    for k in range(max(len(s) for s in splits)):
        lens = []
        for r in range(R):
            want = splits[r][k] if k < len(splits[r]) else 0
            lens.append(len(signals[r]) - done[r] if want is REST else want)
            assert 0 <= lens[r] <= len(signals[r]) - done[r], "the split fits its signal"
        parts = [signals[r][done[r]: done[r] + lens[r]] for r in range(R)]
        buf, rows, spans = C.padded_rows(parts, mis, device)
        tail_in = meter.tail[meter.cur]
        tail_before = tail_in.clone()
        stats, gain = meter.push(rows, list(targets), ceiling)
        sync()
        done = [done[r] + lens[r] for r in range(R)]
        assert meter.n0 == done and meter.tail[1 - meter.cur] is tail_in
        assert np.array_equal(_bits(tail_in), _bits(tail_before)), "the input tail buffer is only read"
        assert np.array_equal(_bits(buf), _bits(C.padded_rows(parts, mis)[0])), "a push writes nothing into the pieces or the padding around them"
        _, so_far, _ = C.padded_rows([signals[r][: done[r]] for r in range(R)], mis, device)
        if any(done):
            ref_stats, ref_gain = ops.wave_loudness(so_far, list(targets), ceiling)
            sync()
            assert np.array_equal(_bits(stats), _bits(ref_stats)), f"push {k}: stats {stats.cpu().tolist()} are not bit for bit the one-shot meter's {ref_stats.cpu().tolist()}"
            assert np.array_equal(_bits(gain), _bits(ref_gain)), f"push {k}: gain {gain.cpu().tolist()} is not bit for bit the one-shot meter's {ref_gain.cpu().tolist()}"
        for r in range(R):  # the tail holds the unfinished segment's samples
            t = done[r] % HOP
            assert np.array_equal(_bits(meter.tail[meter.cur][r, :t]), _bits(torch.from_numpy(signals[r][done[r] - t: done[r]])))
        out.append((stats.cpu().numpy(), gain.cpu().numpy()))
    assert done == [len(s) for s in signals], "the splits spend their signals"
    ws, at, S = one_shot_energies(ops, so_far, device)
    sync()
    for r in range(R):
        assert np.array_equal(_bits(meter.rec[r, 8: 8 + S[r]]), _bits(ws[at[r]: at[r] + S[r]])), f"row {r}: the E table is the one-shot kernel's"
        assert float(meter.rec[r, 5:8].abs().sum()) == 0.0 and float(meter.rec[r, 8 + S[r]:].abs().sum()) == 0.0, "nothing beyond the segments so far is written"
    if oracle:
        C.check_stats(out[-1][0], out[-1][1], signals, targets, ceiling)
    return out


def check_push_refusals(lib, ops, device="cpu", stream=None, sync=lambda: None, run_good=True):
    """Every -22 case of cbx_wave_loudness_push_f32, each with `wave_loudness_push` in cbx_last_error and nothing written -- seg_cap exceeded among them --; then
    (run_good) the good descriptor runs: rc 0 and the one-shot meter's bits"""
    x_host = C.bursts(12000, 3)
    x = torch.from_numpy(x_host).to(device)
    cap = 5
    rec = torch.zeros(1, 8 + cap, dtype=torch.float64, device=device)
    tails = [torch.full((1, HOP), 3.0, device=device) for _ in range(2)]
    stats = torch.full((1, 4), 7.0, dtype=torch.float64, device=device)
    gain = torch.full((1,), 7.0, dtype=torch.float32, device=device)
    ws = torch.zeros(4 * 5, dtype=torch.float64, device=device)
    f = ops.loudness_filter(C.FS)
    coef = (ctypes.c_double * 10)(*f["coef"].tolist())
    bad_coef = (ctypes.c_double * 10)(*(f["coef"].tolist()[:9] + [float("nan")]))
    tg = (ctypes.c_double * 1)(-20.0)
    off, ln, n0 = (ctypes.c_long * 1)(0), (ctypes.c_int * 1)(12000), (ctypes.c_long * 1)(0)
    neg_off, neg_len, neg_n0, late_n0 = (ctypes.c_long * 1)(-1), (ctypes.c_int * 1)(-1), (ctypes.c_long * 1)(-1), (ctypes.c_long * 1)(HOP)
    A = ctypes.addressof
    good = dict(wav=x.data_ptr(), off=A(off), len=A(ln), n0=A(n0), R=1, coef=A(coef), hop=HOP, tg=A(tg), ceiling=1.0, rec=rec.data_ptr(), seg_cap=cap,
                tail_in=tails[0].data_ptr(), tail_out=tails[1].data_ptr(), stats=stats.data_ptr(), gain=gain.data_ptr(), ws=ws.data_ptr(), cap=ws.numel())
    call = lambda d: lib.cbx_wave_loudness_push_f32(d["wav"], d["off"], d["len"], d["n0"], d["R"], d["coef"], d["hop"], d["tg"], d["ceiling"], d["rec"], d["seg_cap"],
                                                    d["tail_in"], d["tail_out"], d["stats"], d["gain"], d["ws"], d["cap"], stream)
    bad = [dict(good, **{k: None}) for k in ("wav", "off", "len", "n0", "coef", "tg", "rec", "tail_in", "tail_out", "stats", "gain", "ws")]
    bad += [dict(good, R=0), dict(good, R=65), dict(good, len=A(neg_len)), dict(good, off=A(neg_off)), dict(good, n0=A(neg_n0)), dict(good, hop=0), dict(good, hop=-5),
            dict(good, coef=A(bad_coef)), dict(good, seg_cap=4), dict(good, n0=A(late_n0)), dict(good, cap=4 * 5 - 1)]   # 5 segments into 4; segments 1 .. 5 into 5
    for d in bad:
        assert call(d) == -22 and b"wave_loudness_push" in lib.cbx_last_error(), d
    sync()
    assert float(stats.min()) == 7.0 and float(gain[0]) == 7.0 and float(ws.abs().max()) == 0.0 and float(rec.abs().max()) == 0.0, "a refusal writes nothing"
    assert all(float(t.min()) == 3.0 and float(t.max()) == 3.0 for t in tails) and np.array_equal(x.cpu().numpy(), x_host), "a refusal writes nothing"
    if run_good:
        assert call(good) == 0
        sync()
        ref_stats, ref_gain = ops.wave_loudness([x], [-20.0])
        sync()
        assert np.array_equal(_bits(stats), _bits(ref_stats)) and np.array_equal(_bits(gain), _bits(ref_gain))
        assert float(tails[0].min()) == 3.0 and float(tails[1][0, 0]) == 3.0, "12 000 samples are five whole segments: no tail is written, the input tail is only read"
