"""GPU (-m gpu): the packed five-launch decode layer on two row tiles (17 .. 32 rows), bit for bit against its one-tile launches (bodies:
tests/two_tile_common.py; the kernel bodies also run on the emulator, tests/test_simt_two_tile.py).

Kernel level: every v2 GEMV form and the decode attention, two-tile launch against the 16-row launches of the same geometry, poisoned pad rows.  Engine:
T3Engine.generate(two_tile=True) of 9 and 16 utterances against the same utterances in batches of at most 8 -- logits of every step and ids, eagerly, from the
captured graph and through the library's token loop.  Schedule: synthesize_pipelined(t3_pair=True) against t3_pair=False.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import two_tile_common as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", T.NS)
@pytest.mark.parametrize("K", T.KS)
@pytest.mark.parametrize("rows", T.ROWS)
@pytest.mark.parametrize("form", T.FORMS)
def test_gemv_two_tile_equals_its_one_tile_launches(dev, form, rows, K, N):
    T.check_gemv_two_tile(dev, form, rows, K, N)


@pytest.mark.parametrize("fold", (False, True))
@pytest.mark.parametrize("ctx", T.ATTN_CTX)
@pytest.mark.parametrize("rows", T.ATTN_ROWS)
def test_decode_attention_above_16_rows_equals_its_16_row_launches(dev, rows, ctx, fold):
    T.check_attn_two_tile(dev, rows, ctx, fold)


@pytest.mark.parametrize("mode", T.ENG_MODES)
@pytest.mark.parametrize("B", (9, 16))
def test_engine_two_tile_logits_equal_batches_of_at_most_8(dev, B, mode):
    T.check_engine_two_tile(dev, B, mode)


def test_pipelined_schedule_pairs_jobs_without_changing_a_result(dev):
    T.check_schedule_pairs(dev)
