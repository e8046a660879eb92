// Music bed (cbx_wave_duck_f32 / cbx_wave_duck_level_f32, include/cbx.h): the finished speech of a programme laid over a background -- music, room tone --
// that is pulled down while someone talks ("ducking"), behind the mix / join and ahead of the loudness step, the limiter and the only copy to the host, so that
// the level and the ceiling hold for the SUM.  The reference has no counterpart: it returns one utterance of one voice as the vocoder left it (tts.py:272,
// mtl_tts.py:352, tts_turbo.py:320).
//
// Rows: R <= 64 speech rows `speech + s_off[r]` of n[r] samples and bed sources `bed + b_off[r]` of nb[r] samples; offsets and lengths travel to the kernels by
// value (2 KiB of kernel arguments), the control numbers are one set per call.  The output row has N = lead + n + tail samples.
//
// Three launches:
//   frames: one WAVE per control frame of 240 output samples: lane l takes the quad l counted from the 16-byte boundary at or below the frame's first speech
//     sample (a 16-byte load inside the row, 4-byte loads at the ragged ends), the wave maximum of |s'| and the NaN flag go through wave_max (cbx_xor_lane
//     butterflies), lane 0 stores the activity (1.0f / 0.0f) in the workspace.  A comparison of exact values: the same decision in every implementation.
//   apply: one workgroup of 256 threads owns 1024 outputs of one row.  It stages the activity of the frames it needs (the tile's frames +- 1 +- S and the hold's
//     pre / post) in LDS, forms A (the hold), 1 - t and G for its <= 7 frames in the order of the definition (fmaf over k ascending from 0), then streams speech
//     and bed: quads counted from the 16-byte boundary at or below the tile's first output, 16-byte stores (and loads where the source address allows), 4-byte
//     accesses at the ragged ends; a quad that meets the loop seam is read sample by sample.  Each value is a function of the row's samples alone -- not of the
//     tile, the grid or the rows' alignment.
//   fold: one workgroup per row folds the tiles' {max |out|, NaN flag, frames with A that begin in the tile} into the row's four doubles (max and integer counts
//     are exact in any order).  No floating-point atomics, plain C++ and vector stores.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int DK_TILE = 1024;                     // outputs of one workgroup: 256 threads x 4
constexpr int DK_Q = 240;                         // samples of a control frame (10 ms at 24 kHz)
constexpr int DK_HOLD_MAX = 200;                  // the largest pre / post, frames
constexpr int DK_S_MAX = 100;                     // the largest smoothing half-width, frames
constexpr int DK_FADE_MAX = 24000;                // the largest xf / fi / fo, samples
constexpr int DK_NG = 8;                          // frames of G one tile reads: (1023 + 239) / 240 + 2 = 7
constexpr int DK_ND = DK_NG + 2 * DK_S_MAX;       // 1 - t over those +- S
constexpr int DK_NA = DK_ND + 2 * DK_HOLD_MAX;    // the activity over those, post below and pre above

struct dk_rows_t : cbx_wave_rows_t {  // (the core: the speech rows)
    long b_off[CBX_WAVE_MAX_ROWS];    // first sample of the bed source, floats from `bed`
    int nb[CBX_WAVE_MAX_ROWS];        // its length
    long out_off[CBX_WAVE_MAX_ROWS];  // first output of the row, floats from `out`
};

struct dk_plan_t {
    long lead, tail;
    float thr, duck;
    int pre, post, S, loop, xf, fi, fo;
};

__device__ __forceinline__ long dk_floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// bed'(i) of the definition for a row with nb > 0; P = nb - xf
__device__ __forceinline__ float dk_bed(const float* b, long nb, int loop, long P, int xf, const float* ramp, long i) {
    if (!loop) return i < nb ? b[i] : 0.0f;
    const long k = i / P, r = i - k * P;
    if (k > 0 && r < xf) return fmaf(ramp[r], b[r] - b[P + r], b[P + r]);
    return b[r];
}

// grid (ceil(max F / 4), R) x 256: wave w of workgroup (x, r) owns control frame 4 x + w of row r.  act[r ldf + f] = 1.0f where the frame is active, else 0.0f
__global__ __launch_bounds__(256) void wave_duck_frames_kernel(const float* __restrict__ speech, dk_rows_t rows, dk_plan_t pl, float* __restrict__ act, long ldf) {
    const int r = blockIdx.y, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + (long)(threadIdx.x >> 6);
    const long n = rows.n[r], N = pl.lead + n + pl.tail;
    if (f * DK_Q >= N) return;  // (wave-uniform)
    long a = f * DK_Q - pl.lead, b = a + DK_Q;  // the frame's speech samples [a, b), cut to the row
    a = a < 0 ? 0 : a, b = b > n ? n : b;
    float m = 0.0f, bad = 0.0f;
    if (a < b) {
        const float* p = speech + rows.off[r];
        const long k = a - (long)(((uintptr_t)(p + a) >> 2) & 3) + 4 * lane;  // quads counted from the 16-byte boundary at or below p + a: at most 61
        if (k < b) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (k >= a && k + 4 <= b) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(p + k);
                v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
            } else {
                for (int e = 0; e < 4; ++e)
                    if (k + e >= a && k + e < b) v[e] = p[k + e];
            }
            for (int e = 0; e < 4; ++e) {
                m = fmaxf(m, fabsf(v[e]));  // (fmaxf drops a NaN: the flag carries it)
                if (!(v[e] == v[e])) bad = 1.0f;
            }
        }
    }
    m = wave_max(m), bad = wave_max(bad);
    if (lane == 0) act[(long)r * ldf + f] = (bad > 0.0f || m > pl.thr) ? 1.0f : 0.0f;  // !(p <= thr), p NaN where the frame holds one
}

// grid (ceil(max N / 1024), R) x 256.  tiles: 4 floats per (row, tile) at (r ldt + x) * 4: {max |out|, NaN flag, frames with A that begin in the tile, 0}
__global__ __launch_bounds__(256) void wave_duck_apply_kernel(const float* __restrict__ speech, const float* __restrict__ bed, dk_rows_t rows, dk_plan_t pl,
                                                              const float* __restrict__ gain, const float* __restrict__ win, const float* __restrict__ ramp,
                                                              const float* __restrict__ act, long ldf, float* __restrict__ out, float* __restrict__ tiles, long ldt) {
#pragma clang fp contract(off)
    __shared__ float s_act[DK_NA], s_d[DK_ND], s_G[DK_NG], s_w[2 * DK_S_MAX + 1];
    __shared__ float s_pk[256];
    __shared__ int s_bad[256], s_cnt[256];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long n = rows.n[r], nb = rows.nb[r], N = pl.lead + n + pl.tail, t0 = (long)blockIdx.x * DK_TILE;
    if (t0 >= N) return;  // (uniform over the workgroup, ahead of its barriers)
    const int nt = N - t0 < DK_TILE ? (int)(N - t0) : DK_TILE;
    const long F = (N + DK_Q - 1) / DK_Q;
    const int S = pl.S, hold = pl.pre + pl.post;
    // sample i reads G[f0] and G[f0 + 1], f0 = floor((i - 120) / 240), both clamped to [0, F): the frames [ga, gb] of G, at most 7
    const long fa = dk_floor_div(t0 - DK_Q / 2, DK_Q), fb = dk_floor_div(t0 + nt - 1 - DK_Q / 2, DK_Q) + 1;
    const long ga = fa < 0 ? 0 : fa, gb = fb > F - 1 ? F - 1 : fb;
    const int ng = (int)(gb - ga + 1), nd = ng + 2 * S, na = nd + hold;
    for (int q = tid; q < na; q += 256) {  // the activity of frames ga - S - post .. gb + S + pre; frames outside [0, F) are inactive
        const long j = ga - S - pl.post + q;
        s_act[q] = (j >= 0 && j < F) ? act[(long)r * ldf + j] : 0.0f;
    }
    for (int i = tid; i <= 2 * S; i += 256) s_w[i] = win[i];
    __syncthreads();
    int cnt = 0;
    for (int q = tid; q < nd; q += 256) {  // 1 - t of frames ga - S .. gb + S: A[f] = the OR of act[f - post .. f + pre]; t = 1 outside [0, F)
        const long f = ga - S + q;
        float d1 = 0.0f;
        if (f >= 0 && f < F) {
            bool A = false;
            for (int j = 0; j <= hold; ++j) A = A || s_act[q + j] != 0.0f;
            if (A) {
                d1 = 1.0f - pl.duck;
                cnt += f * DK_Q >= t0 && f * DK_Q < t0 + nt;  // (a frame is counted by the tile its first sample falls into)
            }
        }
        s_d[q] = d1;
    }
    __syncthreads();
    if (tid < ng) {  // G[ga + tid] = 1 - sum_k w_k (1 - t[f + k]), k ascending, fmaf from 0
        float s = 0.0f;
        for (int k = 0; k <= 2 * S; ++k) s = fmaf(s_w[k], s_d[tid + k], s);
        s_G[tid] = 1.0f - s;
    }
    __syncthreads();
    const float L = gain ? gain[r] : 1.0f;
    const float* ps = speech + rows.off[r];
    const float* pb = bed + rows.b_off[r];  // (not read when nb == 0)
    const long end = nb == 0 ? 0 : (pl.loop ? N : (N < nb ? N : nb));
    const long P = nb - pl.xf;  // (> xf for a looped row: the entry checks it)
    const float fi1 = (float)(pl.fi + 1), fo1 = (float)(pl.fo + 1);
    float* po = out + rows.out_off[r] + t0;
    const int mis = (int)(((uintptr_t)po >> 2) & 3);
    float pk = 0.0f;
    int bad = 0;
    for (int q = tid; 4 * q - mis < nt; q += 256) {  // quads counted from the 16-byte boundary at or below the tile's first output
        const int o0 = 4 * q - mis;                  // (-3 .. -1 in the first quad of a misaligned tile)
        const long i0 = t0 + o0, j0 = i0 - pl.lead;
        const bool whole = o0 >= 0 && o0 + 4 <= nt;
        float sv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, bv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, y[4];
        if (j0 >= 0 && j0 + 4 <= n && ((uintptr_t)(ps + j0) & 15) == 0) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(ps + j0);
            sv[0] = t[0], sv[1] = t[1], sv[2] = t[2], sv[3] = t[3];
        } else {
            for (int e = 0; e < 4; ++e)
                if (o0 + e >= 0 && o0 + e < nt && j0 + e >= 0 && j0 + e < n) sv[e] = ps[j0 + e];
        }
        if (nb > 0 && i0 + 4 > 0 && i0 < end) {
            // a plain run of four source samples: inside the source without a loop; with one, inside one period and outside the cross-fade
            long src = -1;
            if (whole && !pl.loop && i0 + 4 <= nb) src = i0;
            if (whole && pl.loop) {
                const long k = i0 / P, rr = i0 - k * P;
                if (rr + 4 <= P && (k == 0 || rr >= pl.xf)) src = rr;
            }
            if (src >= 0 && ((uintptr_t)(pb + src) & 15) == 0) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(pb + src);
                bv[0] = t[0], bv[1] = t[1], bv[2] = t[2], bv[3] = t[3];
            } else {
                for (int e = 0; e < 4; ++e)
                    if (o0 + e >= 0 && o0 + e < nt && i0 + e < end) bv[e] = dk_bed(pb, nb, pl.loop, P, pl.xf, ramp, i0 + e);
            }
        }
        for (int e = 0; e < 4; ++e) {
            const long i = i0 + e;
            y[e] = 0.0f;
            if (o0 + e < 0 || o0 + e >= nt) continue;
            const long j = i - DK_Q / 2, f0 = dk_floor_div(j, DK_Q);
            const float a = (float)(j - f0 * DK_Q) / 240.0f;
            const long lo = f0 < 0 ? 0 : (f0 > F - 1 ? F - 1 : f0), hi = f0 + 1 > F - 1 ? F - 1 : f0 + 1;  // G[-1] = G[0], G[F] = G[F - 1]
            const float Gl = s_G[lo - ga], Gh = s_G[hi - ga];
            const float g = fmaf(a, Gh - Gl, Gl);
            float env = 0.0f;
            if (i < end) {
                const float up = i < pl.fi ? (float)(i + 1) / fi1 : 1.0f;
                const float dn = end - 1 - i < pl.fo ? (float)(end - i) / fo1 : 1.0f;
                env = up * dn;
            }
            y[e] = fmaf((bv[e] * env) * g, L, sv[e]);
            pk = fmaxf(pk, fabsf(y[e]));
            bad |= !(y[e] == y[e]);
        }
        if (whole) {
            *reinterpret_cast<f32x4*>(po + o0) = f32x4{y[0], y[1], y[2], y[3]};
        } else {
            for (int e = 0; e < 4; ++e)
                if (o0 + e >= 0 && o0 + e < nt) po[o0 + e] = y[e];
        }
    }
    s_pk[tid] = pk, s_bad[tid] = bad, s_cnt[tid] = cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_pk[tid] = fmaxf(s_pk[tid], s_pk[tid + s]), s_bad[tid] |= s_bad[tid + s], s_cnt[tid] += s_cnt[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        float* w = tiles + ((long)r * ldt + blockIdx.x) * 4;
        w[0] = s_pk[0], w[1] = (float)s_bad[0], w[2] = (float)s_cnt[0], w[3] = 0.0f;
    }
}

// grid R x 256: the tiles of row r folded into its four doubles {L as applied, frames with A, F, max |out| (NaN: the row holds one)}; an empty row: {L, 0, 0, 0}
__global__ __launch_bounds__(256) void wave_duck_fold_kernel(dk_rows_t rows, dk_plan_t pl, const float* __restrict__ gain, const float* __restrict__ tiles, long ldt,
                                                             double* __restrict__ stats) {
    __shared__ float s_pk[256];
    __shared__ int s_bad[256];
    __shared__ long s_cnt[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long N = pl.lead + rows.n[r] + pl.tail, nt = (N + DK_TILE - 1) / DK_TILE;
    float pk = 0.0f;
    int bad = 0;
    long cnt = 0;
    for (long x = tid; x < nt; x += 256) {
        const float* w = tiles + ((long)r * ldt + x) * 4;
        pk = fmaxf(pk, w[0]), bad |= w[1] != 0.0f, cnt += (long)w[2];
    }
    s_pk[tid] = pk, s_bad[tid] = bad, s_cnt[tid] = cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_pk[tid] = fmaxf(s_pk[tid], s_pk[tid + s]), s_bad[tid] |= s_bad[tid + s], s_cnt[tid] += s_cnt[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        double* o = stats + 4 * r;
        o[0] = (double)(gain ? gain[r] : 1.0f), o[1] = (double)s_cnt[0], o[2] = (double)((N + DK_Q - 1) / DK_Q), o[3] = s_bad[0] ? (double)NAN : (double)s_pk[0];
    }
}

struct dk_level_t {
    double level[CBX_WAVE_MAX_ROWS];
};

// one workgroup of 64 threads: gain[r] = (float)10^((Ls + level_r - Lb) / 20) in fp64; a level alone where a loudness is not finite
__global__ __launch_bounds__(64) void wave_duck_level_kernel(const double* __restrict__ stats_s, const double* __restrict__ stats_b, dk_level_t lv, int R,
                                                             float* __restrict__ gain) {
    const int r = threadIdx.x;
    if (r >= R) return;
    const double Ls = stats_s[4 * r], Lb = stats_b[4 * r];
    const bool both = Ls - Ls == 0.0 && Lb - Lb == 0.0;  // (finite: x - x is NaN for an infinity or a NaN)
    gain[r] = (float)pow(10.0, (both ? Ls + lv.level[r] - Lb : lv.level[r]) / 20.0);
}

}  // namespace

extern "C" int cbx_wave_duck_f32(const float* speech, const long* s_off, const int* s_len, const float* bed, const long* b_off, const int* b_len, int R,
                                 const float* gain, long lead, long tail, double threshold, double duck, int pre, int post, int S, const float* win, int loop, int xf,
                                 const float* ramp, int fi, int fo, float* out, const long* out_off, long out_cap, double* stats, float* ws, long ws_cap,
                                 void* stream) {
    CBX_REQUIRE(speech && s_off && s_len && b_off && b_len && win && out && out_off && stats && ws, "wave_duck: null pointer");
    dk_rows_t rows = {};  // (entries behind R stay zero: the grids end at R, no kernel reads them)
    cbx_wave_span_t sp, bsp, to;
    int rc = cbx_wave_rows("wave_duck", s_off, s_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(lead >= 0 && tail >= 0 && lead <= 0x7fffffffl && tail <= 0x7fffffffl, "wave_duck: lead = %ld, tail = %ld (samples of bed alone, >= 0)", lead, tail);
    dk_plan_t pl = {};
    pl.lead = lead, pl.tail = tail, pl.thr = (float)threshold, pl.duck = (float)duck;
    pl.pre = pre, pl.post = post, pl.S = S, pl.loop = loop, pl.xf = xf, pl.fi = fi, pl.fo = fo;
    CBX_REQUIRE(threshold > 0.0 && threshold < INFINITY && pl.thr > 0.0f && pl.thr < INFINITY, "wave_duck: the threshold %g is no positive finite float", threshold);
    CBX_REQUIRE(duck > 0.0 && duck <= 1.0 && pl.duck > 0.0f, "wave_duck: the ducked gain %g outside (0, 1]", duck);
    CBX_REQUIRE(pre >= 0 && pre <= DK_HOLD_MAX && post >= 0 && post <= DK_HOLD_MAX, "wave_duck: pre = %d, post = %d outside [0, %d] frames", pre, post, DK_HOLD_MAX);
    CBX_REQUIRE(S >= 1 && S <= DK_S_MAX, "wave_duck: S = %d outside [1, %d]", S, DK_S_MAX);
    CBX_REQUIRE(loop == 0 || loop == 1, "wave_duck: loop = %d outside {0, 1}", loop);
    CBX_REQUIRE(xf >= 0 && xf <= DK_FADE_MAX && fi >= 0 && fi <= DK_FADE_MAX && fo >= 0 && fo <= DK_FADE_MAX, "wave_duck: xf = %d, fi = %d, fo = %d outside [0, %d] samples",
                xf, fi, fo, DK_FADE_MAX);
    CBX_REQUIRE(!(loop && xf > 0) || ramp, "wave_duck: a cross-fade of %d samples without a ramp", xf);
    bsp = cbx_wave_span_t{0, 0, -1, 0};
    long cnt[CBX_WAVE_MAX_ROWS];
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(b_len[r] >= 0 && b_off[r] >= 0, "wave_duck: bed row %d has length %d at offset %ld", r, b_len[r], b_off[r]);
        CBX_REQUIRE(!(loop && b_len[r] > 0 && b_len[r] <= 2 * xf), "wave_duck: bed row %d of %d samples cannot loop with a cross-fade of %d (more than 2 xf)", r, b_len[r], xf);
        rows.b_off[r] = b_off[r], rows.nb[r] = b_len[r], rows.out_off[r] = out_off[r];
        cbx_wave_span_add(&bsp, b_off[r], b_len[r]);
        cnt[r] = lead + s_len[r] + tail;
        CBX_REQUIRE(cnt[r] <= 0x7fffffffl, "wave_duck: row %d has %ld outputs, too many for one launch", r, cnt[r]);
    }
    CBX_REQUIRE(bed || bsp.lo < 0, "wave_duck: null pointer (bed may be NULL only when every bed row is empty)");
    if ((rc = cbx_wave_packed("wave_duck", out_off, cnt, R, out_cap, nullptr, &to))) return rc;  // (the rows' own layout: no sum)
    for (int a = 0; a < R; ++a)
        for (int b = 0; b < R; ++b) {
            const uintptr_t o0 = (uintptr_t)(out + out_off[b]), o1 = (uintptr_t)(out + out_off[b] + cnt[b]);
            const uintptr_t w0 = (uintptr_t)(speech + s_off[a]), w1 = (uintptr_t)(speech + s_off[a] + s_len[a]);
            CBX_REQUIRE(!(s_len[a] > 0 && cnt[b] > 0 && w0 < o1 && o0 < w1), "wave_duck: out row %d overlaps speech row %d (the step does not run in place)", b, a);
            const uintptr_t b0 = (uintptr_t)(bed + b_off[a]), b1 = (uintptr_t)(bed + b_off[a] + b_len[a]);
            CBX_REQUIRE(!(b_len[a] > 0 && cnt[b] > 0 && b0 < o1 && o0 < b1), "wave_duck: out row %d overlaps bed row %d (the step does not run in place)", b, a);
        }
    const long n_max = to.n_max, ldf = (n_max + DK_Q - 1) / DK_Q, ldt = (n_max + DK_TILE - 1) / DK_TILE;
    CBX_REQUIRE(ws_cap >= R * (ldf + 4 * ldt), "wave_duck: workspace of %ld floats, %d rows of %ld frames and %ld tiles need %ld", ws_cap, R, ldf, ldt, R * (ldf + 4 * ldt));
    float* act = ws;
    float* tiles = ws + R * ldf;
    if (n_max > 0) {
        hipLaunchKernelGGL(wave_duck_frames_kernel, dim3((unsigned)((ldf + 3) / 4), (unsigned)R), dim3(256), 0, (hipStream_t)stream, speech, rows, pl, act, ldf);
        int e = cbx_check_launch("wave_duck");
        if (e) return e;
        hipLaunchKernelGGL(wave_duck_apply_kernel, dim3((unsigned)ldt, (unsigned)R), dim3(256), 0, (hipStream_t)stream, speech, bed, rows, pl, gain, win, ramp,
                           (const float*)act, ldf, out, tiles, ldt);
        if ((e = cbx_check_launch("wave_duck"))) return e;
    }
    hipLaunchKernelGGL(wave_duck_fold_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, rows, pl, gain, (const float*)tiles, ldt, stats);
    return cbx_check_launch("wave_duck");
}

extern "C" int cbx_wave_duck_level_f32(const double* stats_speech, const double* stats_bed, const double* level, int R, float* gain, void* stream) {
    CBX_REQUIRE(stats_speech && stats_bed && level && gain, "wave_duck_level: null pointer");
    CBX_REQUIRE(R >= 1 && R <= CBX_WAVE_MAX_ROWS, "wave_duck_level: R = %d outside [1, %d]", R, CBX_WAVE_MAX_ROWS);
    dk_level_t lv = {};
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(level[r] - level[r] == 0.0 && fabs(level[r]) <= 200.0, "wave_duck_level: row %d has the level %g (a finite number of LU within +- 200)", r, level[r]);
        lv.level[r] = level[r];
    }
    hipLaunchKernelGGL(wave_duck_level_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats_speech, stats_bed, lv, R, gain);
    return cbx_check_launch("wave_duck_level");
}
