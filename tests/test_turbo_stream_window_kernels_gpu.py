"""GPU (-m gpu), kernel level: the HiFT source with a phase carry-in -- cbx_hift_source_carry_f32 (ops.hift_source(cum_in=)) and the stage entry
cbx_hift_f0_source_carry -- and the end-of-round emission cbx_stream_emit_f32 (ops.stream_emit), the launches behind windowed streaming
(synthesize_stream(window=), ChatterboxEngine.vocode_stream, ChatterboxVC.generate_stream), through the C ABI on the MI355X: the source of a window against the
full-length source, the emission against the torch slice / clone / lerp loop it replaces, bit for bit.  The same checks run on the SIMT emulator in
test_stream_window_host.py; the engine- and API-level tests of the windowed stream are in test_stream_window_gpu.py.

WHY THIS FILE NAME: test_host_logic.py::test_every_kernel_entry_point_is_named_by_a_kernel_level_test finds the kernel-level modules by a fixed list of patterns of which
`test_turbo_stream_*` is the only glob, and existing test files are not edited when a feature is added (test_turbo_stream_batch_kernels_gpu.py is the precedent).  Do not
rename this file without extending _KERNEL_LEVEL_MODULES there."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_source_with_phase_carry_equals_the_full_length_source(dev):
    """cbx_hift_source_carry_f32 over frames [w0, T) with cum_in = frame_cum_full[:, :, w0] == samples [480 w0, 480 T) of the full-length source for six w0
    (inside a long voiced run, inside and right after an unvoiced stretch, the last frame); NULL and zero cum_in == cbx_hift_source_f32."""
    import stream_window_common as c
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        c.check_source_carry(ops, dev, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("name", ["first_round_no_tails", "steady_window", "short_tails_finals_closed", "no_fade"])
def test_stream_emit_equals_the_torch_expression(dev, name):
    """One cbx_stream_emit_f32 launch == the per-utterance torch loop (new samples, tail * (1 - ramp) + new * ramp, next tails) over ragged emitted / end / avail:
    the first round (no tails), a steady windowed round, tails shorter than the fade beside final and closed utterances, and fade = 0."""
    import stream_window_common as c
    from chatterbox_amd import ops
    with torch.cuda.device(dev):
        faded = c.check_stream_emit(ops, dev, name, sync=torch.cuda.synchronize)
    assert (faded > 0) == (name in ("steady_window", "short_tails_finals_closed"))


def test_f0_source_with_carry_through_the_c_entry_point_equals_the_python_sequence(dev, B=3, T=20):
    """cbx_hift_f0_source_carry against HiFTEngine.f0_predict + source(cum_in=) (cbx_hift_source_carry_f32), ragged batch, carries hundreds of cycles from 0; a
    NULL carry through the same entry == cbx_hift_f0_source."""
    from chatterbox_amd import synth
    from chatterbox_amd.hift import HiFTEngine
    dev = torch.device(dev)
    eng = HiFTEngine(synth.s3gen_state_dict(0), dev)
    mel = (synth.randn((B, T, 80), seed=9) * 1.5 - 4.0).to(dev)
    phase, noise = synth.rand((B, 9), seed=5) * 6.28 - 3.14, synth.randn((B, 9, 480 * T), seed=6)
    phase[:, 0] = 0
    lens = torch.tensor([T, max(1, T - 7), max(1, T // 2)][:B], dtype=torch.int32, device=dev)
    cum_in = (synth.rand((B, 9), seed=8).double() * 900.0 + 0.37).to(dev)
    eng.decode = lambda mel, s, lens=None, fade=True: s.clone()  # the front half only: inference() hands the source to decode()
    out, scans, calls, inner = {}, {}, [], eng._f0_source_c
    eng._f0_source_c = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    for seam in (False, True):
        eng.c_seam = seam
        out[seam] = eng.inference(mel, phase=phase.to(dev), noise=noise.to(dev), lens=lens, cum_in=cum_in)[1].clone()
        scans[seam] = eng.frame_cum.clone()
    assert len(calls) == 1, "the second pass went through cbx_hift_f0_source_carry"
    assert torch.isfinite(out[True]).all() and out[True].abs().max() > 0
    assert torch.equal(out[True], out[False]), f"max |diff| {(out[True] - out[False]).abs().max().item():.3e}"
    assert torch.equal(scans[True], scans[False]) and torch.equal(scans[True][:, :, 0], cum_in), "the scan starts from the carry and stays readable"
    plain = eng.inference(mel, phase=phase.to(dev), noise=noise.to(dev), lens=lens)[1]
    zero = eng.inference(mel, phase=phase.to(dev), noise=noise.to(dev), lens=lens, cum_in=torch.zeros_like(cum_in))[1]
    assert torch.equal(plain, zero) and not torch.equal(plain, out[True])
