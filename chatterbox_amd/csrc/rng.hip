// Counter-based device RNG (cbx_rng_fill_f32, include/cbx.h): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11).  Every float is a pure function of (the row's four key words, its absolute column), so a request's draws do not depend on the batch it runs in, on
// its row, on padding or on the order of calls -- what a sequential torch.Generator cannot give.  It replaces, for a request that carries a seed, the draw
// inside torch.multinomial (t3.py:360,430,455), torch.randn_like of the CFM noise (flow_matching.py:63,216) and the phase / noise draws of SineGen and
// SourceModuleHnNSF (hifigan.py:212-213,226,282).
//
// One thread computes ONE Philox block (four 32-bit words = four columns) and stores it as one 16-byte vector where the block is whole and its address aligned,
// word by word at a ragged head or tail.  The kernel only writes: plain stores (a bulk producer like the flow's kernels, which lose with write-through stores,
// cbx_common.h).  Ten rounds are 20 32x32->64 multiplies per 16 bytes; the normal form adds two logf, two sqrtf and two sincosf.
#include <math.h>

#include "cbx_common.h"

namespace {

struct philox4 {
    unsigned x[4];
};

__device__ __forceinline__ philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return philox4{{c0, c1, c2, c3}};
}

// Box-Muller on the word pair (xa, xb): u1 in (0, 1], u2 in [0, 1), both exact in fp32; |result| <= sqrt(48 ln 2) = 5.77
__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& even, float& odd) {
    const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(xb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    even = r * c;
    odd = r * s;
}

// grid (ceil(blocks / 256), rows): thread t of a row owns Philox block blk0 + t, i.e. absolute columns [4 (blk0 + t), 4 (blk0 + t) + 4) cut to [col0, col0 + n)
__global__ __launch_bounds__(256) void rng_fill_kernel(float* __restrict__ out, long ld_out, const unsigned* __restrict__ keys, long n,
                                                       unsigned long long col0, unsigned long long blk0, unsigned long long n_blk, int normal) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_blk) return;
    const unsigned long long blk = blk0 + t;
    const unsigned* key = keys + 4 * (long)blockIdx.y;
    const philox4 p = philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), key[2], key[3], key[0], key[1]);
    f32x4 v;
    if (normal) {
        float a, b, c, d;
        box_muller(p.x[0], p.x[1], a, b);
        box_muller(p.x[2], p.x[3], c, d);
        v = f32x4{a, b, c, d};
    } else {
        v = f32x4{(float)(p.x[0] >> 8) * 0x1p-24f, (float)(p.x[1] >> 8) * 0x1p-24f, (float)(p.x[2] >> 8) * 0x1p-24f, (float)(p.x[3] >> 8) * 0x1p-24f};
    }
    // columns of the row this block covers: [lo, hi) of [0, n), relative to col0 (j may be negative only in the first block, past n only in the last)
    const long long j = (long long)(4 * blk - col0);  // 4 * blk >= 4 * blk0 > col0 - 4, so the difference fits (wraps consistently when col0 is near 2^64)
    float* row = out + (long)blockIdx.y * ld_out;
    if (j >= 0 && j + 4 <= n && ((uintptr_t)(row + j) & 15) == 0) {
        *reinterpret_cast<f32x4*>(row + j) = v;
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (j + w >= 0 && j + w < n) row[j + w] = v[w];
    }
}

}  // namespace

extern "C" int cbx_rng_fill_f32(float* out, long ld_out, const unsigned* keys, int rows, long n, unsigned long long col0, int dist, void* stream) {
    CBX_REQUIRE(out && keys, "rng_fill: null pointer");
    CBX_REQUIRE(rows >= 0 && rows <= 65535 && n >= 0 && ld_out >= n, "rng_fill: bad shape (rows %d, n %ld, ld_out %ld)", rows, n, ld_out);
    CBX_REQUIRE(dist == CBX_RNG_UNIFORM || dist == CBX_RNG_NORMAL, "rng_fill: unknown distribution %d", dist);
    CBX_REQUIRE((unsigned long long)n <= ~0ull - col0, "rng_fill: col0 + n exceeds 2^64");
    if (rows == 0 || n == 0) return 0;
    const unsigned long long blk0 = col0 >> 2, n_blk = ((col0 + (unsigned long long)n - 1) >> 2) - blk0 + 1;
    const unsigned long long gx = (n_blk + 255) / 256;
    CBX_REQUIRE(gx <= 0x7fffffffull, "rng_fill: n too large for one launch");
    hipLaunchKernelGGL(rng_fill_kernel, dim3((unsigned)gx, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, out, ld_out, keys, n, col0, blk0, n_blk,
                       dist == CBX_RNG_NORMAL);
    return cbx_check_launch("rng_fill");
}
