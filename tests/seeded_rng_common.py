"""Shared by the seeded-RNG tests (not a test module): a NumPy Philox4x32-10 written from the published algorithm (Salmon, Moraes, Dror, Shaw, SC'11) with
the addressing of cbx_rng_fill_f32 (include/cbx.h), the uniform and Box-Muller maps evaluated in float64."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# counter words / key words -> output words: checked on the CPU with exactly this construction
KAT = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (values < 2^32) of one shape, key: two ints -> four uint64 arrays, the output words."""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def words(seed, substream, stream, col0, n):
    """The 32-bit words of absolute columns [col0, col0 + n) of key (seed, substream, stream), and for each column its partner word of the Box-Muller pair:
    (x, xa, xb, odd) uint64 / bool arrays of length n (xa, xb: the even and the odd word of the column's pair)."""
    j = np.arange(col0, col0 + n, dtype=object)  # Python ints: col0 may be near 2^64
    blk = [int(v) >> 2 for v in j]
    lo = np.array([b & MASK for b in blk], dtype=np.uint64)
    hi = np.array([b >> 32 for b in blk], dtype=np.uint64)
    w = np.array([int(v) & 3 for v in j])
    out = philox4x32_10((lo, hi, np.full(n, substream, dtype=np.uint64), np.full(n, stream, dtype=np.uint64)), (seed & MASK, seed >> 32))
    o = np.stack(out)  # (4, n)
    idx = np.arange(n)
    return o[w, idx], o[w & 2, idx], o[(w & 2) + 1, idx], (w & 1).astype(bool)


def uniform(seed, substream, stream, col0, n):
    """float64 (exactly representable in fp32): (x >> 8) * 2^-24"""
    x = words(seed, substream, stream, col0, n)[0]
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normal(seed, substream, stream, col0, n):
    """Box-Muller in float64: u1 = ((xa >> 8) + 1) 2^-24, u2 = (xb >> 8) 2^-24, r = sqrt(-2 ln u1); even word r cos(2 pi u2), odd word r sin(2 pi u2)"""
    _, xa, xb, odd = words(seed, substream, stream, col0, n)
    u1 = ((xa >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (xb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.where(odd, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2))


def fill(keys, col0, n, normal_dist):
    """Reference of one cbx_rng_fill_f32 call: keys = [(seed, substream, stream), ...] -> (rows, n) float64"""
    f = normal if normal_dist else uniform
    return np.stack([f(s, sub, st, col0, n) for s, sub, st in keys])


def key_tensor(keys, device="cpu"):
    """(rows, 4) int32 tensor of [(seed, substream, stream), ...] in the layout of cbx_rng_fill_f32"""
    import torch
    k = np.array([[s & MASK, s >> 32, sub, st] for s, sub, st in keys], dtype=np.uint32)
    return torch.from_numpy(k.view(np.int32)).to(device)
