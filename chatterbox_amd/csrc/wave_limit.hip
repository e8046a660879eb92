// True-peak limiter (cbx_wave_limit_f32, include/cbx.h): the waveforms of a batch held under a dBTP ceiling -- the peak of the band-limited signal BETWEEN the
// samples, which every D/A converter and our own sample_rate= conversion reconstruct -- behind the vocoder and the loudness step, ahead of the only copy to the
// host.  The reference has no counterpart: it returns the vocoder's output as it is (tts.py:272, mtl_tts.py:352, tts_turbo.py:320, vc.py:104).
//
// Rows: R <= 64 waveforms `wav + off[r]` of n[r] samples, as cbx_wave_gain_f32 takes them; offsets, lengths and ceilings travel to the kernel by value (1.5 KiB of
// kernel arguments), so a call needs no upload.  Per row: u = x gamma (one fp32 multiply), y = u oversampled U times by the phase table (fmaf, taps ascending),
// m[i] = max(|u[i]|, |y[U i .. U i + U - 1]|), c[i] = C / m[i] where m[i] > C (else 1), a = the minimum of c over i +- H, g[i] = min(1 - sum_k w_k (1 - a[i + k]),
// c[i]), out = u g.  Every output depends on inputs within 2 H + T samples of it: the chain is local.
//
// One workgroup of 256 threads owns a tile of 1024 outputs of one row.  It stages u over tile +- 2 H plus the filter's reach in LDS (16-byte loads counted from the
// 16-byte boundary at or below the span's first sample inside the row, 4-byte loads at the ragged ends, zeros outside the row), computes m and c over tile +- 2 H,
// takes the sliding minimum by doubling passes in LDS (min over windows of 1, 2, 4, .. 2^k <= 2 H + 1 samples, then two overlapping windows: exact whatever the
// order), forms 1 - a once, and runs the smoothing sum in the order of the definition.  The tile's outputs pass through LDS and leave as 16-byte stores counted
// from the 16-byte boundary at or below the tile's first output, 4-byte stores at the ragged ends.  A tile whose c is 1 everywhere skips minimum and sum: every
// term of the sum is exactly 0 there, so g = 1 and out = u either way.  Each value is a function of the row's samples alone -- not of the tile it falls into, the
// grid or the row's alignment --, so the result is bit for bit the same however the rows are laid out.
//
// Stats: every tile leaves {true peak, min g, samples with g < 1, samples with m > C} in the workspace (a fixed LDS tree; max, min and integer counts are exact in
// any order); a second launch, one workgroup per row, folds the tiles and writes the row's four doubles.  No floating-point atomics, plain C++ and vector stores.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int LM_TILE = 1024;                        // outputs of one workgroup: 256 threads x 4
constexpr int LM_HMAX = 480;                         // the largest look-ahead
constexpr int LM_TAB = 1024;                         // floats of the phase table, U T
constexpr int LM_LEAD = 10;                          // hl / U: samples above i that y[U i + p] reads
constexpr int LM_NC = LM_TILE + 4 * LM_HMAX;         // c over tile +- 2 H
constexpr int LM_SPAN = LM_NC + LM_TAB + 16;         // u over that, plus the filter's reach and the alignment slack
constexpr int LM_WIN = 2 * LM_HMAX + 1;

struct lm_rows_t : cbx_wave_rows_t {
    long out_off[CBX_WAVE_MAX_ROWS];  // first output of the row, floats from `out`
    float ceil[CBX_WAVE_MAX_ROWS];    // (float)C; NaN: the row is not limited
};

// sample i of the row times the pre-gain, zero outside [0, n)
__device__ __forceinline__ float lm_u(const float* p, long n, float gam, long i) { return (i >= 0 && i < n) ? p[i] * gam : 0.0f; }

// m of one sample: x points at u[i] in LDS, tabs at the phase table (row stride ts).  UU / TT > 0: the product's table (U = 4, T = 21) with both loops unrolled, so
// the 21 samples are read once for the four phases; 0: any table, run-time trip counts.  The same fmaf chain in the same order either way: the same bits.
template <int UU, int TT>
__device__ __forceinline__ float lm_peak(const float* x, const float* tabs, int U, int T, int ts, int& nan) {
    float m = fabsf(x[0]);
    nan = !(x[0] == x[0]);
    if constexpr (UU > 0) {
#pragma unroll
        for (int ph = 0; ph < UU; ++ph) {
            const float* t = tabs + ph * (TT | 1);
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < TT; ++j) acc = fmaf(t[j], x[LM_LEAD - j], acc);
            m = fmaxf(m, fabsf(acc));
            nan |= !(acc == acc);
        }
    } else {
        for (int ph = 0; ph < U; ++ph) {
            const float* t = tabs + ph * ts;
            float acc = 0.0f;
            for (int j = 0; j < T; ++j) acc = fmaf(t[j], x[LM_LEAD - j], acc);
            m = fmaxf(m, fabsf(acc));
            nan |= !(acc == acc);
        }
    }
    return m;
}

// grid (ceil(max n / 1024), R / C) x 256: signal g = rows [g C, g C + C) of one length, the channels of one signal (C = 1: row g, cbx_wave_limit_f32).  The
// channels are staged one after the other through s_u: each gives its m, the maximum over the channels so far waits in s_a (NaN where one of them is), and the
// tile's own u of all channels but the last waits in s_keep; c, the minimum and g are formed ONCE, every channel's tile is multiplied by the same g.
// ws: 4 doubles per (signal, tile) at (g ld + x) * 4
template <int C>
__global__ __launch_bounds__(256) void wave_limit_kernel(const float* __restrict__ wav, lm_rows_t rows, const float* __restrict__ gain, const float* __restrict__ tab,
                                                         int U, int T, const float* __restrict__ win, int H, float* __restrict__ out, double* __restrict__ ws, long ld) {
    __shared__ float s_u[LM_SPAN];
    __shared__ float s_a[LM_NC], s_b[LM_NC];
    __shared__ float s_tab[LM_TAB + 8];
    __shared__ float s_w[LM_WIN + 3];
    __shared__ float s_o[C * LM_TILE];
    __shared__ float s_keep[C > 1 ? (C - 1) * LM_TILE : 1];
    __shared__ float s_pk[256], s_mg[256];
    __shared__ int s_bad[256], s_ng[256], s_nm[256], s_any;
    const int sg = blockIdx.y, r = sg * C, tid = threadIdx.x;
    const long n = rows.n[r], t0 = (long)blockIdx.x * LM_TILE;
    if (t0 >= n) return;  // (uniform over the workgroup, ahead of its barriers)
    const int nt = n - t0 < LM_TILE ? (int)(n - t0) : LM_TILE;
    const float gam = gain ? gain[sg] : 1.0f;
    const float CL = rows.ceil[r];
    const int below = T > LM_LEAD + 1 ? T - (LM_LEAD + 1) : 0;  // samples below i that y[U i + p] reads
    const int nc = LM_TILE + 4 * H, na = LM_TILE + 2 * H;
    const int ts = T | 1;  // (an odd row stride: the phases of a wave's lanes fall on different banks)
    const bool product = U == 4 && T == 21;  // (uniform)
    // the span of u: [t0 - 2 H - below, t0 + 1024 + 2 H + LM_LEAD], begun at most three samples lower, where p + ks is a 16-byte boundary
    const long k_lo = t0 - 2 * H - below;
    long ks = 0;
    float pk = 0.0f;
    int bad = 0, nm = 0, any = 0;
    for (int ch = 0; ch < C; ++ch) {
        if (ch > 0) __syncthreads();  // (the last channel's m pass has read s_u)
        const float* p = wav + rows.off[r + ch];
        ks = k_lo - ((k_lo + (long)(((uintptr_t)p >> 2) & 3)) & 3);
        const int span = (int)(t0 + LM_TILE + 2 * H + LM_LEAD + 1 - ks);
        for (int q = tid; 4 * q < span; q += 256) {
            const long k = ks + 4 * q;
            float v[4];
            if (k >= 0 && k + 4 <= n) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(p + k);
                v[0] = t[0] * gam, v[1] = t[1] * gam, v[2] = t[2] * gam, v[3] = t[3] * gam;
            } else {
                for (int e = 0; e < 4; ++e) v[e] = lm_u(p, n, gam, k + e);
            }
            for (int e = 0; e < 4; ++e) s_u[4 * q + e] = v[e];
        }
        if (ch == 0) {
            for (int i = tid; i < U * T; i += 256) s_tab[(i / T) * ts + i % T] = tab[i];
            for (int i = tid; i <= 2 * H; i += 256) s_w[i] = win[i];
            if (tid == 0) s_any = 0;
        }
        __syncthreads();
        // m and c over tile +- 2 H; the tile's own samples also feed the stats
        for (int q = tid; q < nc; q += 256) {
            const long i = t0 - 2 * H + q;
            float c = ch < C - 1 ? 0.0f : 1.0f;  // (ahead of the last channel s_a holds m so far, 0 outside the row)
            if (i >= 0 && i < n) {
                const float* x = s_u + (i - ks);
                int nan;
                float m = product ? lm_peak<4, 21>(x, s_tab, U, T, ts, nan) : lm_peak<0, 0>(x, s_tab, U, T, ts, nan);
                if (ch > 0) {  // (s_a[q] is this thread's own store of the channel before)
                    const float prev = s_a[q];
                    nan |= !(prev == prev);
                    m = fmaxf(m, prev);
                }
                if (ch < C - 1) {
                    c = nan ? NAN : m;
                } else {
                    const bool over = !nan && m > CL;  // (a NaN ceiling compares false: the row is not limited)
                    if (over && m < INFINITY) c = CL / m, any = 1;
                    if (i >= t0 && i < t0 + nt) pk = fmaxf(pk, m), bad |= nan, nm += over;
                }
            }
            s_a[q] = c;
        }
        if (ch < C - 1)
            for (int e = 0; e < 4; ++e) {
                const int o = e * 256 + tid;
                if (o < nt) s_keep[ch * LM_TILE + o] = s_u[t0 - ks + o];
            }
    }
    if (any) s_any = 1;  // (every writer stores the same value)
    __syncthreads();
    const bool limit = s_any != 0;  // (uniform over the workgroup)
    float cr[4];
    for (int e = 0; e < 4; ++e) cr[e] = s_a[2 * H + e * 256 + tid];  // c of this thread's four outputs
    float mg = 1.0f;
    int ng = 0;
    if (limit) {
        // the sliding minimum: after the pass of `half`, cur[q] = min c[q .. q + 2 half - 1]
        float *cur = s_a, *nxt = s_b;
        const int W = 2 * H + 1;
        int len = 1;
        for (; 2 * len <= W; len *= 2) {
            __syncthreads();
            for (int q = tid; q + 2 * len <= nc; q += 256) nxt[q] = fminf(cur[q], cur[q + len]);
            float* sw = cur;
            cur = nxt, nxt = sw;
        }
        __syncthreads();
        // a over tile +- H, kept as 1 - a: a[i] = min c[i - H .. i + H] = min of two windows of `len` samples
        for (int q = tid; q < na; q += 256) nxt[q] = 1.0f - fminf(cur[q], cur[q + W - len]);
        __syncthreads();
        for (int e = 0; e < 4; ++e) {
            const int o = e * 256 + tid;
            if (o >= nt) break;
            const float* d = nxt + o;  // 1 - a[i + k] at d[k + H]
            float s = 0.0f;
            for (int k = 0; k < W; ++k) s = fmaf(s_w[k], d[k], s);
            const float g = fminf(1.0f - s, cr[e]);
            for (int ch = 0; ch < C - 1; ++ch) s_o[ch * LM_TILE + o] = s_keep[ch * LM_TILE + o] * g;
            s_o[(C - 1) * LM_TILE + o] = s_u[t0 - ks + o] * g;
            mg = fminf(mg, g), ng += g < 1.0f;
        }
    } else {
        for (int e = 0; e < 4; ++e) {
            const int o = e * 256 + tid;
            if (o < nt) {
                for (int ch = 0; ch < C - 1; ++ch) s_o[ch * LM_TILE + o] = s_keep[ch * LM_TILE + o];
                s_o[(C - 1) * LM_TILE + o] = s_u[t0 - ks + o];
            }
        }
    }
    s_pk[tid] = pk, s_mg[tid] = mg, s_bad[tid] = bad, s_ng[tid] = ng, s_nm[tid] = nm;
    __syncthreads();
    if (out) {  // quads counted from the 16-byte boundary at or below the tile's first output
        for (int ch = 0; ch < C; ++ch) {
            float* po = out + rows.out_off[r + ch] + t0;
            const float* so = s_o + ch * LM_TILE;
            const int mis = (int)(((uintptr_t)po >> 2) & 3);
            for (int q = tid; 4 * q - mis < nt; q += 256) {
                const int o0 = 4 * q - mis;  // (-3 .. -1 in the first quad of a misaligned tile)
                if (o0 >= 0 && o0 + 4 <= nt) {
                    *reinterpret_cast<f32x4*>(po + o0) = f32x4{so[o0], so[o0 + 1], so[o0 + 2], so[o0 + 3]};
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (o0 + e >= 0 && o0 + e < nt) po[o0 + e] = so[o0 + e];
                }
            }
        }
    }
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            s_pk[tid] = fmaxf(s_pk[tid], s_pk[tid + s]), s_mg[tid] = fminf(s_mg[tid], s_mg[tid + s]);
            s_bad[tid] |= s_bad[tid + s], s_ng[tid] += s_ng[tid + s], s_nm[tid] += s_nm[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* w = ws + ((long)sg * ld + blockIdx.x) * 4;
        w[0] = s_bad[0] ? (double)NAN : (double)s_pk[0], w[1] = (double)s_mg[0], w[2] = (double)s_ng[0], w[3] = (double)s_nm[0];
    }
}

// grid (R / C) x 256: the tiles of signal r (rows [r C, r C + C)) folded into its four doubles (an empty one: {0, 1, 0, 0})
__global__ __launch_bounds__(256) void wave_limit_finish_kernel(lm_rows_t rows, int C, const double* __restrict__ ws, long ld, double* __restrict__ stats) {
    __shared__ double s_pk[256], s_mg[256], s_ng[256], s_nm[256];
    __shared__ int s_bad[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long nt = ((long)rows.n[r * C] + LM_TILE - 1) / LM_TILE;
    double pk = 0.0, mg = 1.0, ng = 0.0, nm = 0.0;
    int bad = 0;
    for (long x = tid; x < nt; x += 256) {
        const double* w = ws + ((long)r * ld + x) * 4;
        bad |= !(w[0] == w[0]);
        pk = fmax(pk, w[0]), mg = fmin(mg, w[1]), ng += w[2], nm += w[3];
    }
    s_pk[tid] = pk, s_mg[tid] = mg, s_ng[tid] = ng, s_nm[tid] = nm, s_bad[tid] = bad;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            s_pk[tid] = fmax(s_pk[tid], s_pk[tid + s]), s_mg[tid] = fmin(s_mg[tid], s_mg[tid + s]);
            s_ng[tid] += s_ng[tid + s], s_nm[tid] += s_nm[tid + s], s_bad[tid] |= s_bad[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) stats[4 * r] = s_bad[0] ? (double)NAN : s_pk[0], stats[4 * r + 1] = s_mg[0], stats[4 * r + 2] = s_ng[0], stats[4 * r + 3] = s_nm[0];
}

}  // namespace

// The limiter behind cbx_wave_limit_f32 (C = 1, who = "wave_limit") and cbx_wave_limit_ch_f32 (wave_stereo.hip, which has checked C and the groups' lengths):
// gain, ceiling and stats have R / C entries, one per signal of C rows; out_off has R.
int cbx_wave_limit_run(const char* who, const float* wav, const long* row_off, const int* row_len, int R, int C, const float* gain, const double* ceiling,
                       const float* tab, int U, int T, const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap,
                       void* stream) {
    CBX_REQUIRE(wav && row_off && row_len && ceiling && tab && win && stats && ws, "%s: null pointer", who);
    CBX_REQUIRE(!out || out_off, "%s: null pointer (out_off may be NULL only with out)", who);
    int rc = cbx_wave_count(who, row_off, row_len, R);
    if (rc) return rc;
    CBX_REQUIRE(U >= 1 && U <= 8, "%s: U = %d outside [1, 8]", who, U);
    CBX_REQUIRE(T >= 1 && U * (long)T <= LM_TAB, "%s: T = %d: a table of U T = %ld floats (1 .. %d)", who, T, U * (long)T, LM_TAB);
    CBX_REQUIRE(H >= 1 && H <= LM_HMAX, "%s: H = %d outside [1, %d]", who, H, LM_HMAX);
    lm_rows_t rows = {};  // (entries behind R stay zero: the grids end at R, no kernel reads them)
    cbx_wave_span_t sp, to;
    if ((rc = cbx_wave_rows(who, row_off, row_len, R, &rows, &sp))) return rc;
    long cnt[CBX_WAVE_MAX_ROWS];
    for (int r = 0; r < R; ++r) {
        const double c = ceiling[r / C];
        CBX_REQUIRE(!(c == c) || (c > 0.0 && c < INFINITY), "%s: row %d has the ceiling %g (a positive finite number, or NaN for a row that is not limited)", who, r, c);
        rows.ceil[r] = (float)c;
        CBX_REQUIRE(!(c == c) || (rows.ceil[r] > 0.0f && rows.ceil[r] < INFINITY), "%s: row %d has the ceiling %g, which is no positive finite float", who, r, c);
        if (out) rows.out_off[r] = out_off[r];
        cnt[r] = row_len[r];
    }
    if (out && (rc = cbx_wave_packed(who, out_off, cnt, R, out_cap, nullptr, &to))) return rc;  // (the rows' own layout: no sum)
    const long n_max = sp.n_max;
    if (out)
        for (int a = 0; a < R; ++a)
            for (int b = 0; b < R; ++b) {
                const uintptr_t w0 = (uintptr_t)(wav + row_off[a]), w1 = (uintptr_t)(wav + row_off[a] + row_len[a]);
                const uintptr_t o0 = (uintptr_t)(out + out_off[b]), o1 = (uintptr_t)(out + out_off[b] + row_len[b]);
                CBX_REQUIRE(!(row_len[a] > 0 && row_len[b] > 0 && w0 < o1 && o0 < w1), "%s: out row %d overlaps wav row %d (the limiter does not run in place)", who, b, a);
            }
    const long ld = (n_max + LM_TILE - 1) / LM_TILE;
    const int S = R / C;
    CBX_REQUIRE(ws_cap >= 4l * S * ld, "%s: workspace of %ld doubles, %d rows of %ld tiles need %ld", who, ws_cap, S, ld, 4l * S * ld);
    if (ld > 0) {
        const auto kernel = C == 2 ? wave_limit_kernel<2> : wave_limit_kernel<1>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)ld, (unsigned)S), dim3(256), 0, (hipStream_t)stream, wav, rows, gain, tab, U, T, win, H, out, ws, ld);
        const int e = cbx_check_launch(who);
        if (e) return e;
    }
    hipLaunchKernelGGL(wave_limit_finish_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, rows, C, (const double*)ws, ld, stats);
    return cbx_check_launch(who);
}

extern "C" int cbx_wave_limit_f32(const float* wav, const long* row_off, const int* row_len, int R, const float* gain, const double* ceiling, const float* tab, int U,
                                  int T, const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap,
                                  void* stream) {
    return cbx_wave_limit_run("wave_limit", wav, row_off, row_len, R, 1, gain, ceiling, tab, U, T, win, H, out, out_off, out_cap, stats, ws, ws_cap, stream);
}
