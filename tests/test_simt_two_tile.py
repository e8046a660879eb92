"""CPU twin of tests/test_two_tile_decode_gpu.py on the SIMT emulator (the harness of tests/test_simt_kernels.py): the two-tile GEMV bodies and the decode
attention with its q|k|v fold at 17 and 32 rows against their one-tile runs, so the identity is pinned without a GPU as well."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "simt")):
    if p not in sys.path:
        sys.path.insert(0, p)

import two_tile_common as T  # noqa: E402

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    import build_emu
    if not os.path.exists(build_emu.CLANG):
        pytest.skip("ROCm's clang++ (x86 host compiler of the emulator build) is not installed")
    import harness
    with harness.emulated() as lib:
        yield lib


@pytest.mark.parametrize("rows,K,N", ((17, 256, 48), (32, 512, 32)))
@pytest.mark.parametrize("form", T.FORMS)
def test_gemv_two_tile_bodies_on_the_emulator(emu, form, rows, K, N):
    T.check_gemv_two_tile(CPU, form, rows, K, N)


@pytest.mark.parametrize("fold", (False, True))
@pytest.mark.parametrize("rows,ctx", ((17, 63), (32, 64), (32, 200)))
def test_decode_attention_fold_above_16_rows_on_the_emulator(emu, rows, ctx, fold):
    T.check_attn_two_tile(CPU, rows, ctx, fold)
