// Dialogue (cbx_wave_mix_f32, include/cbx.h): the trimmed waveforms of the turns of a conversation are SUMMED into one buffer, each at an output position of its
// own, with a gain per voice and the join's fades -- so that the next speaker may come in before the last one has finished and a short interjection may lie over
// the other voice.  cbx_wave_join_f32 lays rows one after another (gaps >= 0: every output sample belongs to one row); here a sample may belong to any number of
// rows.  The reference has no counterpart: it returns one utterance of one voice (tts.py:272, mtl_tts.py:352, tts_turbo.py:320).
//
// Rows: R <= 64 waveforms `wav + off[r]`, n[r] samples each, row r's first sample at out[start[r]]; off / n / start / flags / gain_idx are HOST arrays that
// travel to the kernel by value (1.6 KiB of kernel arguments), so a call needs no upload.
//
// Order: a sample's covering rows are added in ASCENDING r, one rounded multiply per gain and per fade and one rounded add per further row -- a fixed order
// whatever the grid, the tile a sample falls into or the alignment of wav, a row or out; no atomics.
//
// One workgroup of 256 threads per tile of WM_TILE outputs, counted from the 16-byte boundary at or below `out`: a uniform loop over the rows finds those that
// meet the tile, every thread accumulates its four quads in registers in row order and stores them -- 16 bytes wide inside [0, out_len), 4-byte stores at the
// ragged ends (and, when accumulating, in a quad that some row does not cover).  Loads are 16 bytes wide where a quad lies inside its row and the source address
// allows, else 4-byte.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WM_TILE = 4096;  // output samples of one workgroup: 256 threads x 4 quads

struct wm_rows_t : cbx_wave_rows_t {
    long start[CBX_WAVE_MAX_ROWS];
    unsigned char flag[CBX_WAVE_MAX_ROWS];
    int gidx[CBX_WAVE_MAX_ROWS];
};

// grid ceil((out_len + a) / WM_TILE) x 256, a = the elements between the 16-byte boundary at or below `out` and `out`
__global__ __launch_bounds__(256) void wave_mix_kernel(const float* __restrict__ wav, wm_rows_t rows, int R, const float* __restrict__ gain, const float* __restrict__ ramp,
                                                       int fade, float* __restrict__ out, long out_len, int accumulate) {
#pragma clang fp contract(off)
    const long a = (long)(((uintptr_t)out >> 2) & 3);
    const long t_lo = (long)blockIdx.x * WM_TILE - a, t_hi = t_lo + WM_TILE;  // the tile's outputs: [t_lo, t_hi) cut to [0, out_len)
    bool any = false;
    for (int r = 0; r < R; ++r) any = any || (rows.n[r] > 0 && rows.start[r] < t_hi && rows.start[r] + rows.n[r] > t_lo);
    if (!any && accumulate) return;  // (uniform)
    float acc[4][4];
    unsigned has = accumulate ? 0xffffu : 0u, hit = 0u;  // bit 4 it + k: acc holds a value / a row covers the sample
    for (int it = 0; it < 4; ++it) {
        const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
        for (int k = 0; k < 4; ++k) acc[it][k] = 0.0f;
        if (!accumulate || p0 >= out_len) continue;
        if (p0 >= 0 && p0 + 4 <= out_len) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(out + p0);
            acc[it][0] = t[0], acc[it][1] = t[1], acc[it][2] = t[2], acc[it][3] = t[3];
        } else {
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= 0 && p0 + k < out_len) acc[it][k] = out[p0 + k];
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
                    const unsigned bit = 1u << (4 * it + k);
                    acc[it][k] = (has & bit) ? acc[it][k] + s : s;
                    has |= bit, hit |= bit;
                }
            }
        }
    }
    for (int it = 0; it < 4; ++it) {
        const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
        if (p0 >= out_len) break;
        const unsigned m = (hit >> (4 * it)) & 15u;
        if (accumulate && m == 0) continue;  // no row covers the quad: it is not written
        if (p0 >= 0 && p0 + 4 <= out_len && (!accumulate || m == 15u)) {
            *reinterpret_cast<f32x4*>(out + p0) = f32x4{acc[it][0], acc[it][1], acc[it][2], acc[it][3]};
        } else {
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= 0 && p0 + k < out_len && (!accumulate || (m >> k & 1u))) out[p0 + k] = acc[it][k];
        }
    }
}

}  // namespace

extern "C" int cbx_wave_mix_f32(const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, int R, const float* gain, int G,
                                const int* gain_idx, const float* ramp, int fade, float* out, long out_len, int accumulate, void* stream) {
    wm_rows_t rows = {};
    cbx_wave_span_t sp;
    CBX_REQUIRE(start && flags, "wave_mix: null pointer");
    const int rc = cbx_wave_rows("wave_mix", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && out, "wave_mix: null pointer");
    CBX_REQUIRE(out_len >= 0, "wave_mix: out_len = %ld", out_len);
    CBX_REQUIRE(fade >= 0 && (fade == 0 || ramp), "wave_mix: fade = %d%s", fade, fade > 0 ? " without a ramp" : "");
    CBX_REQUIRE(accumulate == 0 || accumulate == 1, "wave_mix: accumulate = %d outside {0, 1}", accumulate);
    CBX_REQUIRE(gain || !gain_idx, "wave_mix: gain_idx without a gain vector");
    CBX_REQUIRE(!gain || G >= 1, "wave_mix: G = %d gains", G);
    CBX_REQUIRE(!gain || gain_idx || G >= R, "wave_mix: %d gains for %d rows and no gain_idx", G, R);
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(start[r] >= 0 && start[r] + rows.n[r] <= out_len, "wave_mix: row %d covers [%ld, %ld) of an output of %ld", r, start[r], start[r] + rows.n[r], out_len);
        CBX_REQUIRE(flags[r] >= 0 && flags[r] <= 3, "wave_mix: row %d has flags %d outside 0 .. 3", r, flags[r]);
        const int gi = gain_idx ? gain_idx[r] : r;
        CBX_REQUIRE(!gain || (gi >= 0 && gi < G), "wave_mix: row %d uses gain %d of %d", r, gi, G);
        rows.start[r] = start[r];
        rows.flag[r] = (unsigned char)flags[r];
        rows.gidx[r] = gain ? gi : 0;
    }
    const cbx_wave_span_t to = {out_len, out_len, out_len > 0 ? 0 : -1, out_len};
    if (const int e = cbx_wave_apart("wave_mix", wav, sp, out, to, "the rows are read while other workgroups write")) return e;
    if (out_len == 0) return 0;
    const long gx = (out_len + 3 + WM_TILE - 1) / WM_TILE;  // (+ 3: out may begin up to three samples into its first quad; a last tile without an output returns)
    CBX_REQUIRE(gx <= 0x7fffffffl, "wave_mix: %ld samples are too many for one launch", out_len);
    hipLaunchKernelGGL(wave_mix_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, wav, rows, R, gain, ramp, fade, out, out_len, accumulate);
    return cbx_check_launch("wave_mix");
}
