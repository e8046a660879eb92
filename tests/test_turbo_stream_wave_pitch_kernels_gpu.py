"""GPU (-m gpu), kernel level: cbx_wave_pitch_f32 (ops.wave_pitch), the pitch step, against the fp64 restatement of its definition (wave_pitch_common.py, which
derives the bound): EVERY element of every row within (T + 3) 2^-24 S_j + 2^-23 D_j + 2^-24 |y64|.  Shapes: rows of 0, 1, 7, 479, 480 and 1931 samples (one launch
of six rows) and one of 70000 (several workgroups per row at every step), as views of one NaN-padded allocation, 16-byte aligned and at every 4-byte misalignment;
steps for p = -12, -6, -1, +0.5, +3.3, +6, +12 semitones; output lengths below n / step and above it (the tail reads past the row's end, as the engine's last frame
does).  step = 1 returns the input's bits; an oversized prefilled output stays untouched outside the rows' spans; a refused call launches nothing.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added.  Do not rename this file without extending
_KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import wave_pitch_common as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p", P.SEMITONES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_wave_pitch_is_within_the_bound_of_the_restatement(dev, name, p):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for aligned in (True, False):
            for tail in ("below", "above"):
                worst = P.check_launch(ops, dev, name, p, aligned, tail, sync=torch.cuda.synchronize)
                print(f"{name} p = {p} aligned = {aligned} {tail}: worst error / bound = {worst:.3f}")


def test_the_shapes_are_what_they_claim():
    assert sorted(n for n, _ in P.SETS["A"]) == [0, 1, 7, 479, 480, 1931]
    for p in P.SEMITONES:
        rows = [[0.0] * n for n, _ in P.SETS["B"]]
        assert min(P.out_lens(rows, P.ratio(p), "below")) > 4 * 256, "several workgroups serve the long row"
        for x in [[0.0] * n for n, _ in P.SETS["A"]] + rows:
            lo, hi = P.out_lens([x], P.ratio(p), "below")[0], P.out_lens([x], P.ratio(p), "above")[0]
            assert lo * P.ratio(p) <= len(x) < hi * P.ratio(p)


@pytest.mark.parametrize("name", ["A", "B"])
def test_step_one_returns_the_bits(dev, name):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        for aligned in (True, False):
            P.check_identity(ops, dev, name, aligned, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("p", [-6, 3.3])
def test_nothing_is_written_outside_the_rows(dev, p):
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        P.check_sentinels(ops, dev, p, sync=torch.cuda.synchronize)


def test_refused_descriptors_launch_nothing(dev):
    """Every refusal of the header returns -22 with the entry's name, and nothing is written; the good descriptor then runs and writes its rows only."""
    from chatterbox_amd import _lib, ops
    with torch.cuda.device(dev):
        x = P.signal("uniform", 1920, 9)
        wav = torch.from_numpy(x).to(dev)
        out = torch.full((1500,), 7.0, device=dev)
        good, keep = P.raw_args(wav.data_ptr(), [0, 960], [960, 960], [1.5, 0.75], [600, 600], ops._pitch_table(dev).data_ptr(), out.data_ptr(), [3, 700], 1500,
                                torch.cuda.current_stream().cuda_stream)
        held = P.refused(_lib.lib, good)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call launches nothing"
        assert _lib.lib.cbx_wave_pitch_f32(*good) == 0
        torch.cuda.synchronize()
        o = out.cpu().numpy()
    P.check_bound(o[3:603], x[:960], 1.5, "row 0")
    P.check_bound(o[700:1300], x[960:], 0.75, "row 1")
    assert (o[:3] == 7.0).all() and (o[603:700] == 7.0).all() and (o[1300:] == 7.0).all()
    del held, keep
