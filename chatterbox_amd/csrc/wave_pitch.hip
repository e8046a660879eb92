// Pitch control (cbx_wave_pitch_f32, include/cbx.h): the cut waveforms of a batch read back at an arbitrary REAL step -- `step` source samples per output sample --
// in ONE launch, behind the vocoder and ahead of the loudness step, the pauses, the join, the format launch and the only copy to the host.  The reference has no
// such step (models/s3gen/s3gen.py:289 vocodes the flow's mel as it is; tts.py:272, mtl_tts.py:352, tts_turbo.py:320, vc.py:104 return what the vocoder gives).
// The engine stretches the mel by the pitch ratio r = 2^(p / 12) (cbx_mel_time_scale_f32), the vocoder runs on the stretched mel, and this kernel reads the
// result at step = r: the duration of the unpitched call, every frequency -- the formants too -- multiplied by r.  cbx_wave_format_f32 cannot serve: it is rational
// polyphase with U <= 147, and 2^(1/12) is irrational.
//
// Rows: R <= 64 pieces `wav + off[r]` of len[r] samples, as cbx_wave_format_f32 takes them; every per-row number travels to the kernel by value (3 KiB of kernel
// arguments), so a call needs no upload.  tab[k] = h(k / L), k = 0 .. Z L + 1, the fp32 table of the host's fp64 Kaiser-windowed sinc (Z zero crossings per side, L
// steps per crossing).  Output j of a row: x = j step in fp64, c = min(1, 1 / step); for i ascending over max(0, ceil(x - Z / c)) .. min(n - 1, floor(x + Z / c)):
// u = |x - i| c L in fp64 (a tap with u >= Z L is skipped), k = (long)u, a = (float)(u - k), w = fmaf(a, tab[k + 1] - tab[k], tab[k]), acc = fmaf(w, wav[i], acc)
// from 0; y[j] = (float)c acc.
//
// One workgroup per (256 outputs, row), one output per thread.  The table (16 KiB at Z = 16, L = 256) and the tile's input span -- at most 255 step + 2 Z / c + 8
// <= 584 floats there; samples outside [0, n) are zeros -- are staged in LDS.  The span begins where the row's pointer is 16-byte aligned: quads inside the row are
// one 16-byte load whatever the row's own alignment, the ragged ends 4-byte loads.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WP_TILE = 256;
constexpr int WP_SPAN = 640;    // LDS floats of a tile's input span (the entry checks ceil(255 step + 2 Z / c) + 8 against it)
constexpr int WP_TAB = 4098;    // LDS floats of the table: Z L + 2 <= 4098

struct wp_rows_t : cbx_wave_rows_t {       // (3 KiB with the core)
    long out_off[CBX_WAVE_MAX_ROWS];  // first output of the row, floats from `out`
    double step[CBX_WAVE_MAX_ROWS];   // source samples per output sample
    double c[CBX_WAVE_MAX_ROWS];      // min(1, 1 / step): the filter's cutoff, relative to the source's Nyquist rate, and its gain
    double half[CBX_WAVE_MAX_ROWS];   // Z / c: the filter's reach to either side, in source samples
    int cnt[CBX_WAVE_MAX_ROWS];       // N: outputs of the row
};

// the first / last source sample output j may read: max(0, ceil(j step - half)) / min(n - 1, floor(j step + half)); x is a statement of its own, so that the
// tile's span and every thread's taps come from the same fp64 product
__device__ __forceinline__ long wp_first(long j, double step, double half) {
    const double x = (double)j * step;
    const double lo = ceil(x - half);
    return lo > 0.0 ? (long)lo : 0;
}
__device__ __forceinline__ long wp_last(long j, double step, double half, long n) {
    const double x = (double)j * step;
    const double hi = floor(x + half);
    return hi < (double)(n - 1) ? (long)hi : n - 1;
}

// grid (ceil(max cnt / 256), R) x 256
__global__ __launch_bounds__(256) void wave_pitch_kernel(const float* __restrict__ wav, wp_rows_t rows, const float* __restrict__ tab, int ZL, double Ld,
                                                         float* __restrict__ out) {
    __shared__ float s_x[WP_SPAN];
    __shared__ float s_tab[WP_TAB];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long n = rows.n[r], cnt = rows.cnt[r];
    const long jb = (long)blockIdx.x * WP_TILE;
    if (jb >= cnt) return;  // (uniform over the workgroup, ahead of its barrier)
    const int nt = cnt - jb < WP_TILE ? (int)(cnt - jb) : WP_TILE;
    const double step = rows.step[r], c = rows.c[r], half = rows.half[r];
    const float* row = wav + rows.off[r];
    const long i_lo = wp_first(jb, step, half), i_hi = wp_last(jb + nt - 1, step, half, n);
    // the span begins at most three samples below i_lo, where row + ks is a 16-byte boundary
    const long mis = (i_lo + (long)(((uintptr_t)row >> 2) & 3)) & 3;
    const long ks = i_lo - mis;
    const int span = (int)(i_hi - ks + 1);  // (<= 0: no output of the tile reads a sample)
    for (int q = tid; 4 * q < span; q += WP_TILE) {
        const long k = ks + 4 * q;
        float v[4];
        if (k >= 0 && k + 4 <= n) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(row + k);
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
            for (int e = 0; e < 4; ++e) v[e] = (k + e >= 0 && k + e < n) ? row[k + e] : 0.0f;
        }
        for (int e = 0; e < 4; ++e) s_x[4 * q + e] = v[e];
    }
    const int nh = ZL + 2;
    if (((uintptr_t)tab & 15) == 0) {
        for (int q = tid; 4 * q < nh; q += WP_TILE) {
            if (4 * q + 4 <= nh) {
                *reinterpret_cast<f32x4*>(s_tab + 4 * q) = *reinterpret_cast<const f32x4*>(tab + 4 * q);
            } else {
                for (int e = 4 * q; e < nh; ++e) s_tab[e] = tab[e];
            }
        }
    } else {
        for (int e = tid; e < nh; e += WP_TILE) s_tab[e] = tab[e];
    }
    __syncthreads();
    if (tid >= nt) return;
    const long j = jb + tid;
    const double x = (double)j * step;
    const long lo = wp_first(j, step, half), hi = wp_last(j, step, half, n);
    const double top = (double)ZL;
    float acc = 0.0f;
    for (long i = lo; i <= hi; ++i) {
        const double u = fabs(x - (double)i) * c * Ld;
        if (u >= top) continue;
        const long k = (long)u;
        const float a = (float)(u - (double)k);
        const float w = __builtin_fmaf(a, s_tab[k + 1] - s_tab[k], s_tab[k]);
        acc = __builtin_fmaf(w, s_x[i - ks], acc);
    }
    out[rows.out_off[r] + j] = (float)c * acc;
}

}  // namespace

extern "C" int cbx_wave_pitch_f32(const float* wav, const long* row_off, const int* row_len, const double* step, const int* out_len, int R, const float* tab, int Z,
                                  int L, float* out, const long* out_off, long out_cap, void* stream) {
    CBX_REQUIRE(wav && row_off && row_len && step && out_len && tab && out && out_off, "wave_pitch: null pointer");
    int rc = cbx_wave_count("wave_pitch", row_off, row_len, R);
    if (rc) return rc;
    CBX_REQUIRE(Z >= 1 && L >= 1 && (long)Z * L + 2 <= WP_TAB, "wave_pitch: a table of Z = %d crossings of L = %d steps (Z, L >= 1, Z L + 2 <= %d)", Z, L, WP_TAB);
    wp_rows_t rows = {};     // (entries behind R stay zero: the grid ends at R, the kernel does not read them)
    cbx_wave_span_t in, to;  // the rows span [lo, hi) of wav, their outputs [lo, hi) of out
    if ((rc = cbx_wave_rows("wave_pitch", row_off, row_len, R, &rows, &in))) return rc;
    long cnt[CBX_WAVE_MAX_ROWS];
    for (int r = 0; r < R; ++r) {
        const double s = step[r];
        CBX_REQUIRE(s >= 0.5 && s <= 2.0, "wave_pitch: row %d has step %g (a finite number in [0.5, 2])", r, s);  // (NaN fails both comparisons)
        const double c = s > 1.0 ? 1.0 / s : 1.0, half = (double)Z / c;
        CBX_REQUIRE(ceil((WP_TILE - 1) * s + 2.0 * half) + 8.0 <= WP_SPAN, "wave_pitch: Z = %d at step %g does not fit the kernel's LDS", Z, s);
        rows.out_off[r] = out_off[r], rows.step[r] = s, rows.c[r] = c, rows.half[r] = half, rows.cnt[r] = out_len[r];
        cnt[r] = out_len[r];
    }
    if ((rc = cbx_wave_packed("wave_pitch", out_off, cnt, R, out_cap, "samples", &to))) return rc;
    if ((rc = cbx_wave_apart("wave_pitch", wav, in, out, to, "an output reads samples on either side of its position"))) return rc;
    const long cnt_max = to.n_max;
    if (cnt_max == 0) return 0;
    hipLaunchKernelGGL(wave_pitch_kernel, dim3((unsigned)((cnt_max + WP_TILE - 1) / WP_TILE), (unsigned)R), dim3(WP_TILE), 0, (hipStream_t)stream, wav, rows,
                       tab, Z * L, (double)L, out);
    return cbx_check_launch("wave_pitch");
}
