"""CPU (-m "not gpu"): the C ABI of the GPT-2 decode step / token loop (cbx_gpt2_decode_step, cbx_gpt2_loop_*): ctypes layout against the C compiler, and
the step itself on the SIMT emulator (tests/simt) against the launch sequence chatterbox_amd/t3_turbo.py issues from Python, bit for bit."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

CPU = torch.device("cpu")


def test_gpt2_step_ctypes_structs_match_the_c_header(tmp_path):
    """cbx_gpt2_step_t / cbx_gpt2_packed_layer_t: the size and every field offset of the ctypes mirrors equal what gcc gives include/cbx.h."""
    import ctypes
    import shutil
    import subprocess
    from chatterbox_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = {"cbx_gpt2_step_t": _lib.Gpt2Step, "cbx_gpt2_packed_layer_t": _lib.Gpt2PackedLayer, "cbx_gpt2_layer_t": _lib.Gpt2Layer}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cbx.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


def _engine_and_state(B, L=1, d=256, ctx=(20, 33, 7), max_ctx=64, steps=8):
    """A 1-layer, 256-wide T3TurboEngine on the CPU and a decode state in the middle of an utterance: random KV cache up to each row's position,
    random next ids / uniforms, Turbo's sampling parameters in device memory."""
    from chatterbox_amd import synth
    from chatterbox_amd.t3_turbo import START_SPEECH, T3TurboEngine
    eng = T3TurboEngine(synth.t3_turbo_state_dict(L, d, 0), CPU)
    st = eng._get_state(B, max_ctx, steps)
    eng._prepare_tune()
    g = torch.Generator().manual_seed(3)
    pos = torch.tensor(ctx[:B], dtype=torch.int32)
    st["kc"].copy_(torch.randn(st["kc"].shape, generator=g) * 0.5)
    st["vc"].copy_(torch.randn(st["vc"].shape, generator=g) * 0.5)
    st["positions"].copy_(pos)
    st["ctx_lens"].copy_(pos + 1)
    st["next_ids"].copy_(torch.randint(0, START_SPEECH, (B,), generator=g))
    st["uniforms"].copy_(torch.rand(st["uniforms"].shape, generator=g))
    st["samp_dev"].copy_(torch.tensor([0.0, 0.8, 0.0, 0.95, 1.2, 1000.0, -1.0, 0.0]).repeat(B, 1))
    for k in ("seen", "step", "done", "n_generated", "out_tokens"):
        st[k].zero_()
    return eng, st


def _snapshot(st):
    snap = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
    snap.update({("dws", k): v.clone() for k, v in st["dws"].items()})
    return snap


def _restore(st, snap):
    for k, v in snap.items():
        (st["dws"][k[1]] if isinstance(k, tuple) else st[k]).copy_(v)


_KEYS = ("logits", "out_tokens", "n_generated", "next_ids", "positions", "ctx_lens", "kc", "vc", "seen", "step", "done")


@pytest.mark.parametrize("B", [1, 3], ids=["B1_row_path", "B3_packed_path"])
def test_gpt2_decode_step_equals_the_python_launch_sequence_on_the_emulator(emu, B):
    """cbx_gpt2_decode_step (csrc/gpt2_step.hip) against T3TurboEngine._forward + _sample issued launch by launch: identical logits, tokens, sampler
    state and KV cache after two steps -- the row path at B = 1, the packed 16-row-tile path at B = 3."""
    eng, st = _engine_and_state(B)
    assert eng._row(st) == (B == 1) and eng._use_c_step(st)
    snap = _snapshot(st)
    for _ in range(2):
        eng._decode_step(st)
    want = {k: st[k].clone() for k in _KEYS}
    assert torch.isfinite(want["logits"]).all() and float(want["logits"].abs().max()) > 0 and int(want["n_generated"].min()) == 2
    _restore(st, snap)
    for _ in range(2):
        eng._decode_step_c(st)
    for k in _KEYS:
        assert torch.equal(want[k], st[k]), f"cbx_gpt2_decode_step differs from the Python launch sequence in {k}"


@pytest.mark.parametrize("B", [1, 3], ids=["B1_row_path", "B3_packed_path"])
def test_gpt2_token_loop_equals_python_steps_on_the_emulator(emu, B):
    """cbx_gpt2_loop_run of n steps == n Python token steps from the same state; *steps_run reports the steps issued."""
    eng, st = _engine_and_state(B)
    snap = _snapshot(st)
    for _ in range(3):
        eng._decode_step(st)
    want = {k: st[k].clone() for k in _KEYS}
    _restore(st, snap)
    assert eng._run_c_loop(st, 3, 0) == 3
    for k in _KEYS:
        assert torch.equal(want[k], st[k]), f"cbx_gpt2_loop_run differs from the Python steps in {k}"


def test_gpt2_decode_step_refuses_the_seven_launch_form(emu):
    """More than 16 rows (the 7-launch form, which Python keeps replaying itself) are refused with a message."""
    import ctypes
    from chatterbox_amd._lib import Gpt2Layer, Gpt2Step
    layers = (Gpt2Layer * 1)()
    d = Gpt2Step()
    d.n_layers, d.rows, d.dim, d.n_heads, d.vocab, d.layers = 1, 17, 256, 4, 6563, layers
    assert emu.cbx_gpt2_decode_step(ctypes.byref(d), None) != 0
    assert b"16 rows" in emu.cbx_last_error()
