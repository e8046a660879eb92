// Stereo dialogue (cbx_wave_pan_mix_f32, cbx_wave_loudness_ch_f32, cbx_wave_limit_ch_f32, include/cbx.h): the turns of a conversation summed into TWO planes, each
// voice at a place of its own between left and right, then metered and limited as ONE two-channel signal.  The reference has no counterpart: it returns one mono
// utterance of one voice (tts.py:272, mtl_tts.py:352, tts_turbo.py:320).
//
// The panned mix is cbx_wave_mix_f32's kernel (wave_mix.hip) with two sets of sums: the rows' descriptor, the tile (WP_TILE = 4096 outputs per workgroup of 256
// threads, counted from the 16-byte boundary at or below `out`), the row loop in ASCENDING r and the balance gain / fade-in / fade-out multiplies are the mono
// entry's; then one rounded multiply by the row's left and right gain and one rounded add per plane.  A source sample is read once for both planes.  The pan gains
// are HOST floats that travel with the descriptor by value (2.1 KiB of kernel arguments in all).  The right plane begins plane_stride floats behind the left, so
// its quads may sit at another offset from a 16-byte boundary: each plane stores 16 bytes wide where ITS address allows and 4 bytes wide where not.
//
// The two linked entries hold no kernel of their own: the meter's per-row phases and the limiter's oversampler are the mono entries' code, and the step that sees
// both channels -- the sum of the segment energies, the maximum of the m -- is the channel count C as a template parameter of the mono kernels
// (wave_loudness.hip: wave_loud_row_kernel, wave_limit.hip: wave_limit_kernel).  Here: C and the groups' lengths are checked, then the shared launchers run.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WP_TILE = 4096;  // output samples per plane of one workgroup: 256 threads x 4 quads (WM_TILE of wave_mix.hip)

struct wp_rows_t : cbx_wave_rows_t {
    long start[CBX_WAVE_MAX_ROWS];
    unsigned char flag[CBX_WAVE_MAX_ROWS];
    int gidx[CBX_WAVE_MAX_ROWS];
    float pan[CBX_WAVE_MAX_ROWS][2];  // left and right gain of the row
};

// grid ceil((out_len + a) / WP_TILE) x 256, a = the elements between the 16-byte boundary at or below `out` and `out`; plane c is out + c ps
__global__ __launch_bounds__(256) void wave_pan_mix_kernel(const float* __restrict__ wav, wp_rows_t rows, int R, const float* __restrict__ gain, const float* __restrict__ ramp,
                                                           int fade, float* __restrict__ out, long ps, long out_len, int accumulate) {
#pragma clang fp contract(off)
    const long a = (long)(((uintptr_t)out >> 2) & 3);
    const long t_lo = (long)blockIdx.x * WP_TILE - a, t_hi = t_lo + WP_TILE;  // the tile's outputs: [t_lo, t_hi) cut to [0, out_len)
    bool any = false;
    for (int r = 0; r < R; ++r) any = any || (rows.n[r] > 0 && rows.start[r] < t_hi && rows.start[r] + rows.n[r] > t_lo);
    if (!any && accumulate) return;  // (uniform)
    float acc[2][4][4];
    unsigned has = accumulate ? 0xffffu : 0u, hit = 0u;  // bit 4 it + k: acc holds a value / a row covers the sample (the same for both planes)
    for (int c = 0; c < 2; ++c) {
        const float* pl = out + c * ps;
        for (int it = 0; it < 4; ++it) {
            const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
            for (int k = 0; k < 4; ++k) acc[c][it][k] = 0.0f;
            if (!accumulate || p0 >= out_len) continue;
            if (p0 >= 0 && p0 + 4 <= out_len && ((uintptr_t)(pl + p0) & 15) == 0) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(pl + p0);
                acc[c][it][0] = t[0], acc[c][it][1] = t[1], acc[c][it][2] = t[2], acc[c][it][3] = t[3];
            } else {
                for (int k = 0; k < 4; ++k)
                    if (p0 + k >= 0 && p0 + k < out_len) acc[c][it][k] = pl[p0 + k];
            }
        }
    }
    if (any) {
        for (int r = 0; r < R; ++r) {
            const int n = rows.n[r];
            const long st = rows.start[r];
            if (n <= 0 || st >= t_hi || st + n <= t_lo) continue;  // (uniform)
            const int F = fade < n / 2 ? fade : n / 2;
            const bool fin = (rows.flag[r] & 1) != 0, fout = (rows.flag[r] & 2) != 0;
            const float* src = wav + rows.off[r];
            const float g = gain ? gain[rows.gidx[r]] : 1.0f;
            const float pl = rows.pan[r][0], pr = rows.pan[r][1];
            for (int it = 0; it < 4; ++it) {
                const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
                const long i0 = p0 - st;  // (may be negative, or reach beyond the row)
                if (i0 + 4 <= 0 || i0 >= n) continue;
                float v[4];
                if (i0 >= 0 && i0 + 4 <= n && ((uintptr_t)(src + i0) & 15) == 0) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(src + i0);
                    v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
                } else {
                    for (int k = 0; k < 4; ++k) v[k] = (i0 + k >= 0 && i0 + k < n) ? src[i0 + k] : 0.0f;
                }
                for (int k = 0; k < 4; ++k) {
                    const long i = i0 + k;
                    if (i < 0 || i >= n) continue;
                    float s = v[k];
                    if (gain) s = s * g;
                    if (fin && i < F) s = s * ramp[i];
                    else if (fout && i >= n - F) s = s * ramp[n - 1 - i];
                    const float tl = s * pl, tr = s * pr;
                    const unsigned bit = 1u << (4 * it + k);
                    acc[0][it][k] = (has & bit) ? acc[0][it][k] + tl : tl;
                    acc[1][it][k] = (has & bit) ? acc[1][it][k] + tr : tr;
                    has |= bit, hit |= bit;
                }
            }
        }
    }
    for (int c = 0; c < 2; ++c) {
        float* pl = out + c * ps;
        for (int it = 0; it < 4; ++it) {
            const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
            if (p0 >= out_len) break;
            const unsigned m = (hit >> (4 * it)) & 15u;
            if (accumulate && m == 0) continue;  // no row covers the quad: it is not written
            if (p0 >= 0 && p0 + 4 <= out_len && (!accumulate || m == 15u) && ((uintptr_t)(pl + p0) & 15) == 0) {
                *reinterpret_cast<f32x4*>(pl + p0) = f32x4{acc[c][it][0], acc[c][it][1], acc[c][it][2], acc[c][it][3]};
            } else {
                for (int k = 0; k < 4; ++k)
                    if (p0 + k >= 0 && p0 + k < out_len && (!accumulate || (m >> k & 1u))) pl[p0 + k] = acc[c][it][k];
            }
        }
    }
}

}  // namespace

extern "C" int cbx_wave_pan_mix_f32(const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, const float* pan, int R,
                                    const float* gain, int G, const int* gain_idx, const float* ramp, int fade, float* out, long plane_stride, long out_len,
                                    int accumulate, void* stream) {
    wp_rows_t rows = {};
    cbx_wave_span_t sp;
    CBX_REQUIRE(start && flags && pan, "wave_pan_mix: null pointer");
    const int rc = cbx_wave_rows("wave_pan_mix", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && out, "wave_pan_mix: null pointer");
    CBX_REQUIRE(out_len >= 0, "wave_pan_mix: out_len = %ld", out_len);
    CBX_REQUIRE(plane_stride >= out_len, "wave_pan_mix: plane_stride = %ld below out_len = %ld (the planes would overlap)", plane_stride, out_len);
    CBX_REQUIRE(fade >= 0 && (fade == 0 || ramp), "wave_pan_mix: fade = %d%s", fade, fade > 0 ? " without a ramp" : "");
    CBX_REQUIRE(accumulate == 0 || accumulate == 1, "wave_pan_mix: accumulate = %d outside {0, 1}", accumulate);
    CBX_REQUIRE(gain || !gain_idx, "wave_pan_mix: gain_idx without a gain vector");
    CBX_REQUIRE(!gain || G >= 1, "wave_pan_mix: G = %d gains", G);
    CBX_REQUIRE(!gain || gain_idx || G >= R, "wave_pan_mix: %d gains for %d rows and no gain_idx", G, R);
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(start[r] >= 0 && start[r] + rows.n[r] <= out_len, "wave_pan_mix: row %d covers [%ld, %ld) of an output of %ld", r, start[r], start[r] + rows.n[r], out_len);
        CBX_REQUIRE(flags[r] >= 0 && flags[r] <= 3, "wave_pan_mix: row %d has flags %d outside 0 .. 3", r, flags[r]);
        const int gi = gain_idx ? gain_idx[r] : r;
        CBX_REQUIRE(!gain || (gi >= 0 && gi < G), "wave_pan_mix: row %d uses gain %d of %d", r, gi, G);
        for (int c = 0; c < 2; ++c) {
            CBX_REQUIRE(fabsf(pan[2 * r + c]) < INFINITY, "wave_pan_mix: row %d has the %s gain %g, which is not finite", r, c ? "right" : "left", (double)pan[2 * r + c]);
            rows.pan[r][c] = pan[2 * r + c];
        }
        rows.start[r] = start[r];
        rows.flag[r] = (unsigned char)flags[r];
        rows.gidx[r] = gain ? gi : 0;
    }
    const cbx_wave_span_t to = {out_len, out_len, out_len > 0 ? 0 : -1, out_len};
    for (int c = 0; c < 2; ++c)
        if (const int e = cbx_wave_apart("wave_pan_mix", wav, sp, out + c * plane_stride, to, "the rows are read while other workgroups write")) return e;
    if (out_len == 0) return 0;
    const long gx = (out_len + 3 + WP_TILE - 1) / WP_TILE;  // (+ 3: out may begin up to three samples into its first quad; a last tile without an output returns)
    CBX_REQUIRE(gx <= 0x7fffffffl, "wave_pan_mix: %ld samples are too many for one launch", out_len);
    hipLaunchKernelGGL(wave_pan_mix_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, wav, rows, R, gain, ramp, fade, out, plane_stride, out_len, accumulate);
    return cbx_check_launch("wave_pan_mix");
}

extern "C" int cbx_wave_loudness_ch_f32(const float* wav, const long* row_off, const int* row_len, int R, int C, const double* coef, int hop, const double* target,
                                        double ceiling, double* stats, float* gain, double* ws, long ws_cap, void* stream) {
    if (const int rc = cbx_wave_groups("wave_loudness_ch", row_off, row_len, R, C)) return rc;
    return cbx_wave_loudness_run("wave_loudness_ch", wav, row_off, row_len, R, C, coef, hop, target, ceiling, stats, gain, ws, ws_cap, stream);
}

extern "C" int cbx_wave_limit_ch_f32(const float* wav, const long* row_off, const int* row_len, int R, int C, const float* gain, const double* ceiling, const float* tab,
                                     int U, int T, const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap,
                                     void* stream) {
    if (const int rc = cbx_wave_groups("wave_limit_ch", row_off, row_len, R, C)) return rc;
    return cbx_wave_limit_run("wave_limit_ch", wav, row_off, row_len, R, C, gain, ceiling, tab, U, T, win, H, out, out_off, out_cap, stats, ws, ws_cap, stream);
}
