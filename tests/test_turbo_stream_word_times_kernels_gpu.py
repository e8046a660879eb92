"""GPU (-m gpu), kernel level: the two word-timestamp kernels against the NumPy restatements of word_times_common.py.

cbx_attn_text_mass_f32 (ops.attn_text_mass): |err| <= 2e-5 (1 + |ref|) against the fp64 restatement -- the project's tolerance for fp32 attention kernels
(test_softmax_stress_gpu.py).  The kernel's tile sizes, named: TM_QW = 4 queries per wave (rows of 3 / 4 / 5 queries), TM_KT = 64 keys per tile of pass 1 (contexts
of 63 / 64 / 65 and 127 / 128 / 129 keys) and 64 text columns per tile of pass 2 (63 / 64 / 65 columns); K travels as a view of a [row][head][ctx][64] cache.
cbx_align_path_f32 (ops.align_path): spans and frame_tok BIT-EXACT against the fp32 restatement of the recurrence; a wave of the kernel owns 64 columns and the
walk back stages AP_CHUNK = 64 frames at a time, which (64, 65), (65, 64), (130, 33) and (1000, 1024) straddle.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added.  Do not rename this file without extending
_KERNEL_LEVEL_MODULES there."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import word_times_common as W  # noqa: E402

pytestmark = pytest.mark.gpu


def _cols(rows):
    return [[r[i] for r in rows] for i in range(4)]


@pytest.mark.parametrize("case", range(len(W.MASS_CASES)), ids=[c[0].split(":")[0] for c in W.MASS_CASES])
def test_text_mass_is_the_restated_softmax_slice(dev, case):
    """every case of the table: the values, the sentinel outside [q_len) x [t_len), and -- the poison test -- K beyond each row's last visible key filled with NaN
    changes no bit of the result"""
    from chatterbox_amd import ops
    name, H, heads, rows = W.MASS_CASES[case]
    q, k = W.mass_inputs(H, rows, 100 + case)
    ref = W.mass_ref(q, k, heads, *_cols(rows), 0.125, 0.5)
    with torch.cuda.device(dev):
        mass = W.run_mass(ops, dev, q, k, heads, rows, weight=0.5)
        poisoned = W.run_mass(ops, dev, q, k, heads, rows, weight=0.5, poison=True)
        plain = W.run_mass(ops, dev, q, k, heads, rows, weight=0.5, cache_layout=False)
        torch.cuda.synchronize()
    print(f"{name}: worst err / (1 + |ref|) = {W.check_mass(mass, ref, rows):.3g}")
    assert torch.equal(mass, poisoned), "NaN keys nobody sees changed the result"
    assert torch.equal(mass, plain), "the result depends on K's head stride"
    if case == 0:
        assert float(mass[0, 0, 0]) == 0.5, "one query, one key, one text column: p = 1 exactly"


def test_text_mass_poison_beyond_every_query(dev):
    """Query i of a row sees the keys j <= ctx0 + i.  A launch of ONE row per query -- row i holds queries 0 .. i, and every key beyond ctx0 + i is NaN -- gives
    query i the bits it has in the launch of the whole row, where those keys hold numbers: what lies beyond a query's own causal end never reaches its result.
    7 queries: the last wave of the whole row holds 3, so queries share a wave with later ones whose keys they must not see."""
    from chatterbox_amd import ops
    H, heads, nq, c0, t0, tl = 2, [1, 0], 7, 61, 5, 40  # contexts 62 .. 68: the key-tile edge at 64 lies between two queries of one wave
    q, k = W.mass_inputs(H, [(nq, c0, t0, tl)], 77)
    rows = [(i + 1, c0, t0, tl) for i in range(nq)]
    with torch.cuda.device(dev):
        whole = W.run_mass(ops, dev, q, k, heads, [(nq, c0, t0, tl)])
        each = W.run_mass(ops, dev, np.repeat(q, nq, 0), np.repeat(k, nq, 0), heads, rows, poison=True)
        torch.cuda.synchronize()
    for i in range(nq):
        assert torch.equal(each[i, i, :tl], whole[0, i, :tl]), i
    W.check_mass(each, W.mass_ref(np.repeat(q, nq, 0), np.repeat(k, nq, 0), heads, *_cols(rows), 0.125, 1.0), rows)


def test_text_mass_rows_sum_to_weight_times_heads_and_accumulate(dev):
    """The text range equal to the whole context of the FIRST query (one query per row: t0 = 0, t_len = ctx0 + 1): the row sums to weight * n_sel.  Two
    accumulating launches (heads [2], then [0, 2]) equal one restated sum; the first launch overwrites what the buffer held."""
    from chatterbox_amd import ops
    rows = [(1, 69, 0, 70), (1, 0, 0, 1), (1, 63, 0, 64)]
    q, k = W.mass_inputs(3, rows, 5)
    with torch.cuda.device(dev):
        mass = W.run_mass(ops, dev, q, k, [0, 1, 1], rows, weight=0.25)
        got = mass.cpu().numpy().astype(np.float64)
        for z, r in enumerate(rows):
            assert abs(got[z, 0, :r[3]].sum() - 0.75) <= W.MASS_TOL * 1.75, (z, got[z, 0, :r[3]].sum())
        rows2 = [(5, 9, 2, 6), (6, 70, 3, 66)]
        q, k = W.mass_inputs(3, rows2, 6)
        acc = W.run_mass(ops, dev, q, k, [2], rows2, weight=0.5)
        acc = W.run_mass(ops, dev, q, k, [0, 2], rows2, weight=0.5, accumulate=True, mass=acc)
        torch.cuda.synchronize()
    ref = [a + b for a, b in zip(W.mass_ref(q, k, [2], *_cols(rows2), 0.125, 0.5), W.mass_ref(q, k, [0, 2], *_cols(rows2), 0.125, 0.5))]
    W.check_mass(acc, ref, rows2)


def test_text_mass_first_query_offset_and_wide_scores(dev):
    """q0: the row's queries begin inside its q block (the alignment pass: behind the text positions).  Scores spread to about +-80 (scaled q) stay finite and
    within the tolerance."""
    from chatterbox_amd import ops
    rows = [(6, 30, 4, 20), (3, 66, 0, 65)]
    q, k = W.mass_inputs(2, [(r[0] + 5, r[1], r[2], r[3]) for r in rows], 8, spread=27.0)
    q0 = [5, 2]
    qs = np.stack([q[z, q0[z]: q0[z] + max(r[0] for r in rows)] for z in range(2)])
    s = 0.125 * np.einsum("zihd,zjhd->zhij", qs.astype(np.float64), k.astype(np.float64))
    assert 60 < np.abs(s).max() < 130, np.abs(s).max()
    ref = W.mass_ref(qs, k, [1, 0], *_cols(rows), 0.125, 1.0)
    with torch.cuda.device(dev):
        mass = torch.full((2, 8, 70), -7.0, device=dev)
        kt = torch.from_numpy(k).to(dev).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        ops.attn_text_mass(torch.from_numpy(q).to(dev), kt, mass, [1, 0], *_cols(rows), 0.125, q0=q0)
        torch.cuda.synchronize()
    print(f"scores up to {np.abs(s).max():.1f}: worst err / (1 + |ref|) = {W.check_mass(mass, ref, rows):.3g}")


def test_text_mass_refused_descriptors_write_nothing(dev):
    from chatterbox_amd import _lib
    with torch.cuda.device(dev):
        q, k, mass = torch.zeros(1, 4, 2, 64, device=dev), torch.zeros(1, 12, 2, 64, device=dev), torch.full((1, 4, 8), -7.0, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def call(heads=(0,), n_sel=1, q0=(0,), q_len=(4,), ctx0=(8,), t0=(1,), t_len=(8,), nz=1, m_si=8, k_st=128):
            a = [W.c_ints(list(v)) for v in (heads, q0, q_len, ctx0, t0, t_len)]
            return _lib.lib.cbx_attn_text_mass_f32(q.data_ptr(), k.data_ptr(), mass.data_ptr(), a[0], n_sel, 2, a[1], a[2], a[3], a[4], a[5], nz, 512, 128, 1536, k_st, 64,
                                                   32, m_si, 0.125, 1.0, 0, st)
        for bad in (dict(heads=(2,)), dict(n_sel=0), dict(n_sel=17), dict(nz=0), dict(nz=65), dict(q_len=(-1,)), dict(ctx0=(4605,)), dict(t_len=(1025,)),
                    dict(t0=(2,)), dict(q0=(-1,)), dict(m_si=7), dict(k_st=126)):
            assert call(**bad) == -22 and b"attn_text_mass" in _lib.lib.cbx_last_error(), bad
        torch.cuda.synchronize()
        assert bool((mass == -7.0).all()), "a refused call launches nothing"
        assert call() == 0
        torch.cuda.synchronize()
        assert bool((mass == 0.0).sum() == 0) and abs(float(mass[0, 0].sum()) - 8 / 9) < 1e-5, "zero q: uniform rows over 9, 10, 11, 12 visible keys"


PATH_GPU_SHAPES = W.PATH_SHAPES + [(1000, 1024)]


@pytest.mark.parametrize("kind", ["random", "halves"])
def test_align_path_is_bit_exact(dev, kind):
    """every shape of the list alone, then all of them ragged in ONE launch; `halves`: scores quantised to multiples of 0.5, so that ties are common"""
    from chatterbox_amd import ops
    scores = [W.path_scores(n, m, 40 + i, kind) for i, (n, m) in enumerate(PATH_GPU_SHAPES)]
    with torch.cuda.device(dev):
        for s in scores:
            W.check_path(*W.run_path(ops, dev, [s]), [s])
        W.check_path(*W.run_path(ops, dev, scores), scores)


def test_align_path_finds_the_path_it_was_built_around(dev):
    from chatterbox_amd import ops
    shapes = [(70, 9), (64, 64), (300, 130), (5, 1)]
    scores = [W.path_scores(n, m, 0, "diagonal") for n, m in shapes]
    with torch.cuda.device(dev):
        spans, frame_tok = W.run_path(ops, dev, scores)
    W.check_path(spans, frame_tok, scores)
    for z, (n, m) in enumerate(shapes):
        assert np.array_equal(frame_tok[z, :n], W.diagonal_tok(n, m)), (n, m)


def test_align_path_refused_descriptors_write_nothing(dev):
    from chatterbox_amd import _lib
    with torch.cuda.device(dev):
        score = torch.zeros(2, 6, 8, device=dev)
        spans, ft, ws = torch.full((2, 8, 2), -7, dtype=torch.int32, device=dev), torch.full((2, 6), -7, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def call(n=(6, 3), m=(8, 2), nz=2, s_si=8, sp_sb=16, ft_sb=6, ws_cap=512, ws_off=0):
            return _lib.lib.cbx_align_path_f32(score.data_ptr(), 48, s_si, W.c_ints(list(n)), W.c_ints(list(m)), nz, spans.data_ptr(), sp_sb, ft.data_ptr(), ft_sb,
                                               ws.data_ptr() + ws_off, ws_cap, st)
        for bad in (dict(nz=0), dict(nz=65), dict(n=(0, 3)), dict(n=(4097, 3)), dict(m=(0, 2)), dict(m=(1025, 2)), dict(s_si=7), dict(sp_sb=15), dict(ft_sb=5),
                    dict(ws_cap=95), dict(ws_off=4)):
            assert call(**bad) == -22 and b"align_path" in _lib.lib.cbx_last_error(), bad
        torch.cuda.synchronize()
        assert bool((spans == -7).all()) and bool((ft == -7).all()), "a refused call launches nothing"
        assert call() == 0
        torch.cuda.synchronize()
        assert ft[0].tolist() == [0, 0, 0, 0, 0, 0] and ft[1].tolist() == [0, 1, 1, -7, -7, -7], "all-zero scores: a tie stays, -inf does not"
        assert spans[0, 0].tolist() == [0, 6] and spans[0, 1:].flatten().tolist() == [6] * 14 and spans[1, :2].tolist() == [[0, 1], [1, 3]] and bool((spans[1, 2:] == -7).all())
