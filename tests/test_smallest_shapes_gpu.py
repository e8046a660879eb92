"""GPU (-m gpu), kernel level: the software-pipelined kernels -- gemm_planes.hip (every tile form of test_planes_gpu.TILES), attention_planes.hip (versions 0 .. 6),
gemm_split.hip and the loaders of gemm_f32.hip -- at the smallest shapes they accept, where their prologues and drains run: K walks of 1 .. 3 K tiles against rings of
2 .. 4 LDS stages, the `nk < PKT` arm of the deferred-epilogue forms, M = 1 .. 63, a single part-filled tile, fewer tiles than workgroups, key sequences below one KV
tile and not a multiple of 8, two and three KV tiles against the three-stage ring.  These are the shapes of short utterances and short streaming rounds on the default
(precision 16) path.  Bodies, shapes, references and tolerances: smallest_shapes_common.py; tests/test_simt_kernels.py (_SMALLSHAPE) runs a reduced matrix of the same
bodies on the SIMT emulator, plain, under CBX_EMU_DMA=deferred (counted waits) and under CBX_EMU_SCHED=random (barriers).

(nk, tiles per workgroup) pairs per tile form, from smallest_shapes_common.walk (each body prints its own SMALLSHAPE-COVER line; profiles/smallest_shapes_tests.log):
  * Linear, persist = 0: one tile per workgroup, nk = 1, 2, 3, 4, 6 on the BK = 32 forms and 1, 2, 3 on the BK = 64 forms (K = 64, 128, 192).  persist = 2:
      forms 1, 2, 13, 16                                   (1,1) (2,1) (3,1) (4,2) (6,8)
      forms 3, 4, 12, 14, 17, 22, 24, 25, 33, 34, 37       (1,1) (2,1) (3,1) (4,1) (6,5)
      forms 9, 43                                          (1,1) (2,1) (3,1) (4,3) (6,13)
      form 10                                              (1,1) (2,1) (3,1) (4,2) (6,5)
      forms 11, 15, 18, 19, 23, 26, 27, 28, 36             (1,1) (2,1) (3,1) (4,1) (6,3)
      forms 5, 6 (BK = 64)                                 (1,1) (2,2) (3,8)
      forms 7, 8, 21, 31, 32, 35, 41, 42 (BK = 64)         (1,1) (2,1) (3,5)
      forms 44, 45 (BK = 64), form 0 at K % 64 == 0        (1,1) (2,3) (3,13)
    (form 0 at K = 32 and 96 is form 9's kernel).  Short walks ON a tile walk also come from the conv (nk = 3 or 6, 4 - 5 tiles per workgroup at persist = 2) and
    from the transposed column range (nk = 1, 2; 2 - 3 tiles per workgroup);
  * deferred epilogue (41, 42), both df_kinds: (nk, tiles per workgroup) = (1, 8), (2, 8), (3, 8) at 300 x 640, persist = 2 -- every tile but a workgroup's first
    takes the `nk < PKT` arm with 3, 2 and 1 K-tile-less slots -- and (1, 1), (2, 1), (3, 1) at 65 x 512, persist = 0 (everything drains);
  * LayerNorm epilogue: nk = 1, 2, 3 against its three stages, 1 .. 3 row tiles, on one or two workgroups.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import smallest_shapes_common as S  # noqa: E402
from test_planes_gpu import TILES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("persist", [0, 2])
@pytest.mark.parametrize("tile", TILES)
def test_gemm_planes_linear_smallest(dev, tile, persist):
    ran = S.check_linear_tile(dev, tile, persist)
    bk = 64 if tile == 0 else S.FORMS[tile][2]
    assert {nk for nk, _ in ran} >= ({1, 2, 3} if bk == 64 and tile else {1, 2, 3, 4, 6} if tile else {1, 2, 3}), ran


@pytest.mark.parametrize("persist,M,N", [(2, 300, 640), (0, 65, 512)])
@pytest.mark.parametrize("tile,plain", [(41, 32), (42, 35)])
def test_gemm_planes_deferred_epilogue_smallest(dev, tile, plain, persist, M, N):
    ran = S.check_deferred_epilogue(dev, tile, plain, persist, M, N)
    assert {nk for nk, _ in ran} == {1, 2, 3} and all((tpw > 1) == (persist == 2) for _, tpw in ran), ran  # nk < PKT = 4: the K-tile-less arm runs wherever a workgroup walks on


@pytest.mark.parametrize("persist", [0, 2])
@pytest.mark.parametrize("K", S.LN_KS)
def test_gemm_planes_layernorm_epilogue_smallest(dev, K, persist):
    S.check_layernorm_epilogue(dev, K, persist)


@pytest.mark.parametrize("persist", [0, 2])
@pytest.mark.parametrize("tile", S.CONV_FORMS)
def test_gemm_planes_conv_smallest(dev, tile, persist):
    S.check_conv_tile(dev, tile, persist)


@pytest.mark.parametrize("persist", [0, 2])
@pytest.mark.parametrize("tile", S.PT_FORMS)
def test_gemm_planes_transposed_smallest(dev, tile, persist):
    S.check_transposed_tile(dev, tile, persist)


@pytest.mark.parametrize("version", range(7))
def test_flash_attn_planes_smallest(dev, version):
    S.check_attention(dev, version)


def test_exact_gemm_smallest(dev):
    S.check_f32_linear(dev, 1, S.F32_P1_M, S.F32_P1_N, S.F32_P1_K)


@pytest.mark.parametrize("prec", [3, 6, 16])
def test_split_gemm_smallest(dev, prec):
    S.check_f32_linear(dev, prec, S.F32_SPLIT_M, S.F32_SPLIT_N, S.F32_SPLIT_K)


def test_split_gemm_layernorm_fold_smallest(dev):
    S.check_f32_layernorm_fold(dev)


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("prec", [1, 16])
def test_gemm_refuses_k_not_a_multiple_of_4(dev, prec, M):
    S.check_k_multiple_of_4_contract(dev, prec, M)
