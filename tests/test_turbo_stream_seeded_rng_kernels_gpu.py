"""GPU (-m gpu), kernel level: cbx_rng_fill_f32 (ops.rng_fill), the counter-based RNG behind per-request seeds, against the NumPy Philox4x32-10 restatement
of seeded_rng_common.py -- known answer, both distributions, ragged rows, slices at any col0, the counter carry, substreams, stream ids, moments."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import seeded_rng_common as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_NORMAL = 1e-5  # |n| <= 5.77; the fp32 angle 2 pi u2 is off by <= 2^-22 (1.4e-6), plus a few ulp of logf / sqrtf / sincosf (derivation: test_seeded_rng_host.py)
KEYS = [(0, 0, 0), (12345, 2, 1), (2 ** 63 + 7, 8, 3)]


def _fill(dev, keys, n, col0=0, normal=False, pad=0):
    from chatterbox_amd import ops
    out = torch.full((len(keys), n + pad), float("nan"), device=dev)
    ops.rng_fill(out, R.key_tensor(keys, dev), n=n, col0=col0, normal=normal)
    return out


def _check(dev, keys, n, col0, normal, pad=3):
    out = _fill(dev, keys, n, col0, normal, pad)
    assert out[:, n:].isnan().all(), "columns [n, ld_out) must not be written"
    got, want = out[:, :n].double().cpu().numpy(), R.fill(keys, col0, n, normal)
    err = float(np.abs(got - want).max())
    print(f"rows={len(keys)} n={n} col0={col0} {'normal' if normal else 'uniform'}: max |err| {err:.3e}")
    if normal:
        assert np.isfinite(got).all() and err <= TOL_NORMAL, f"normals: max |err| {err:.3e}"
    else:
        assert np.array_equal(got, want), "uniforms are bit-equal to (x >> 8) * 2^-24"
    return out[:, :n]


def test_rng_fill_known_answer(dev):
    """Seed 0, stream 0, substream 0, columns 0 .. 3: the first known-answer block of Philox4x32-10, as (x >> 8) * 2^-24."""
    want = torch.tensor([(w >> 8) * 2.0 ** -24 for w in R.KAT[0][2]], dtype=torch.float64)
    got = _fill(dev, [(0, 0, 0)], 4)
    assert torch.equal(got[0].double().cpu(), want)


@pytest.mark.parametrize("n", [1, 5, 4101])
@pytest.mark.parametrize("normal", [False, True], ids=["uniform", "normal"])
def test_rng_fill_equals_the_restatement(dev, n, normal):
    """Three rows (seeds 0, 12345, 2^63 + 7), ld_out = n + 3 with NaN padding: 4101 columns are 1026 blocks -- five workgroups per row, a ragged last block."""
    _check(dev, KEYS, n, 0, normal)


@pytest.mark.parametrize("normal", [False, True], ids=["uniform", "normal"])
def test_rng_fill_slices_equal_the_long_fill(dev, normal):
    """col0 in {0, 1, 6, 4099}, n = 37: torch.equal to columns [col0, col0 + 37) of ONE fill of 4200 columns (vector stores there, scalar head / tail here)."""
    full = _fill(dev, KEYS, 4200, 0, normal)
    for col0 in (0, 1, 6, 4099):
        part = _fill(dev, KEYS, 37, col0, normal, pad=1)
        assert torch.equal(part[:, :37], full[:, col0: col0 + 37]), f"col0={col0}"
        assert part[:, 37:].isnan().all()


@pytest.mark.parametrize("normal", [False, True], ids=["uniform", "normal"])
def test_rng_fill_counter_carry(dev, normal):
    """col0 = 2^34 + 3, n = 9: block indices 2^32 .. 2^32 + 2 -- the counter's second word."""
    _check(dev, KEYS, 9, 2 ** 34 + 3, normal)
    lo = _fill(dev, KEYS, 9, 3, normal)
    hi = _fill(dev, KEYS, 9, 2 ** 34 + 3, normal)
    assert not torch.equal(lo, hi), "the high counter word must take part"


def test_rng_fill_substreams_and_stream_ids(dev):
    """Nine rows that share a seed and differ in substream only (the vocoder noise's harmonics): all distinct, each equal to the restatement; two rows that differ
    in stream id only: distinct."""
    keys = [(987654321, h, 3) for h in range(9)]
    for normal in (False, True):
        out = _check(dev, keys, 257, 0, normal)
        assert len({tuple(r.tolist()) for r in out.cpu()}) == 9
    two = _check(dev, [(55, 0, 0), (55, 0, 1)], 64, 0, False)
    assert not torch.equal(two[0], two[1])


def test_rng_fill_normal_moments(dev):
    """2^20 normals of one key (seed 2024, stream 1; the restatement's own sample passes: mean 5.2e-4, var - 1 1.0e-3): 5-sigma bounds |mean| <= 5 / sqrt(n) = 4.9e-3
    and |var - 1| <= 5 sqrt(2 / n) = 6.9e-3; and the uniforms lie in [0, 1)."""
    n = 1 << 20
    x = _fill(dev, [(2024, 0, 1)], n, normal=True)[0].double()
    mean, var = float(x.mean()), float(x.var(unbiased=False))
    print(f"n = 2^20: mean {mean:.3e} (bound {5 / n ** 0.5:.1e}), var - 1 {var - 1:.3e} (bound {5 * (2 / n) ** 0.5:.1e}), max |x| {float(x.abs().max()):.3f}")
    assert abs(mean) <= 5 / n ** 0.5 and abs(var - 1) <= 5 * (2 / n) ** 0.5 and float(x.abs().max()) <= 5.78
    u = _fill(dev, [(2024, 0, 0)], n)[0]
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
