// Dialogue (cbx_wave_mix_f32, and cbx_wave_pan_mix_f32 of wave_stereo.hip; include/cbx.h): the trimmed waveforms of the turns of a conversation are SUMMED into
// one buffer -- or, panned, into the two planes of a stereo buffer --, each at an output position of its own, with a gain per voice and the join's fades -- so that
// the next speaker may come in before the last one has finished and a short interjection may lie over the other voice.  cbx_wave_join_f32 lays rows one after
// another (gaps >= 0: every output sample belongs to one row); here a sample may belong to any number of rows.  The reference has no counterpart: it returns one
// utterance of one voice (tts.py:272, mtl_tts.py:352, tts_turbo.py:320).
//
// ONE kernel, wave_mix_kernel<P>, with the plane count P in {1, 2} as its template parameter, and ONE host side, cbx_wave_mix_run (declared in wave_common.h): the
// checks, the descriptor, the grid and the launch of both entries.  cbx_wave_mix_f32 is its P = 1 call; cbx_wave_pan_mix_f32 (wave_stereo.hip) its P = 2 call.
//
// Rows: R <= 64 waveforms `wav + off[r]`, n[r] samples each, row r's first sample at out[start[r]]; off / n / start / flags / gain_idx -- and with P = 2 the left
// and right gain of every row -- are HOST arrays that travel to the kernel by value (1.6 KiB of kernel arguments, 2.1 KiB with the pan gains), so a call needs
// no upload.
//
// Order: a sample's covering rows are added in ASCENDING r, one rounded multiply per gain and per fade and one rounded add per further row -- a fixed order
// whatever the grid, the tile a sample falls into or the alignment of wav, a row or out; no atomics.  P = 1 has no pan multiply at all (not even by 1.0f, which
// could change a NaN's payload); P = 2 adds one rounded multiply by the row's left and right gain and one rounded add PER PLANE, and reads a source sample once
// for both planes.
//
// One workgroup of 256 threads per tile of WM_TILE outputs (per plane), counted from the 16-byte boundary at or below `out`: a uniform loop over the rows finds
// those that meet the tile, every thread accumulates its four quads in registers in row order and stores them -- 16 bytes wide inside [0, out_len), 4-byte stores
// at the ragged ends (and, when accumulating, in a quad that some row does not cover).  Loads are 16 bytes wide where a quad lies inside its row and the source
// address allows, else 4-byte.  The right plane begins plane_stride floats behind the left, so its quads may sit at another offset from a 16-byte boundary: it is
// loaded and stored 16 bytes wide where ITS address allows and 4 bytes wide where not (the left plane's quads are aligned by the way the tiles are counted).
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WM_TILE = 4096;  // output samples per plane of one workgroup: 256 threads x 4 quads

struct wm_rows_t : cbx_wave_rows_t {
    long start[CBX_WAVE_MAX_ROWS];
    unsigned char flag[CBX_WAVE_MAX_ROWS];
    int gidx[CBX_WAVE_MAX_ROWS];
};

struct wm_pan_rows_t : wm_rows_t {
    float pan[CBX_WAVE_MAX_ROWS][2];  // left and right gain of the row
};

// the descriptor of an instance: the pan gains travel only where there are two planes
template <int P>
struct wm_desc {
    using type = wm_rows_t;
};
template <>
struct wm_desc<2> {
    using type = wm_pan_rows_t;
};

// grid ceil((out_len + a) / WM_TILE) x 256, a = the elements between the 16-byte boundary at or below `out` and `out`; plane c is out + c ps
template <int P>
__global__ __launch_bounds__(256) void wave_mix_kernel(const float* __restrict__ wav, typename wm_desc<P>::type rows, int R, const float* __restrict__ gain,
                                                       const float* __restrict__ ramp, int fade, float* __restrict__ out, long ps, long out_len, int accumulate) {
#pragma clang fp contract(off)
    const long a = (long)(((uintptr_t)out >> 2) & 3);
    const long t_lo = (long)blockIdx.x * WM_TILE - a, t_hi = t_lo + WM_TILE;  // the tile's outputs: [t_lo, t_hi) cut to [0, out_len)
    bool any = false;
    for (int r = 0; r < R; ++r) any = any || (rows.n[r] > 0 && rows.start[r] < t_hi && rows.start[r] + rows.n[r] > t_lo);
    if (!any && accumulate) return;  // (uniform)
    float acc[P][4][4];
    unsigned has = accumulate ? 0xffffu : 0u, hit = 0u;  // bit 4 it + k: acc holds a value / a row covers the sample (the same for every plane)
    for (int c = 0; c < P; ++c) {
        const float* pl = out + c * ps;
        for (int it = 0; it < 4; ++it) {
            const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
            for (int k = 0; k < 4; ++k) acc[c][it][k] = 0.0f;
            if (!accumulate || p0 >= out_len) continue;
            if (p0 >= 0 && p0 + 4 <= out_len && (c == 0 || ((uintptr_t)(pl + p0) & 15) == 0)) {
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
            float pg[P] = {};
            if constexpr (P > 1)
                for (int c = 0; c < P; ++c) pg[c] = rows.pan[r][c];
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
                    for (int c = 0; c < P; ++c) {
                        float t = s;
                        if constexpr (P > 1) t = s * pg[c];
                        acc[c][it][k] = (has & bit) ? acc[c][it][k] + t : t;
                    }
                    has |= bit, hit |= bit;
                }
            }
        }
    }
    for (int c = 0; c < P; ++c) {
        float* pl = out + c * ps;
        for (int it = 0; it < 4; ++it) {
            const long p0 = t_lo + 4 * ((long)it * 256 + threadIdx.x);
            if (p0 >= out_len) break;
            const unsigned m = (hit >> (4 * it)) & 15u;
            if (accumulate && m == 0) continue;  // no row covers the quad: it is not written
            if (p0 >= 0 && p0 + 4 <= out_len && (!accumulate || m == 15u) && (c == 0 || ((uintptr_t)(pl + p0) & 15) == 0)) {
                *reinterpret_cast<f32x4*>(pl + p0) = f32x4{acc[c][it][0], acc[c][it][1], acc[c][it][2], acc[c][it][3]};
            } else {
                for (int k = 0; k < 4; ++k)
                    if (p0 + k >= 0 && p0 + k < out_len && (!accumulate || (m >> k & 1u))) pl[p0 + k] = acc[c][it][k];
            }
        }
    }
}

}  // namespace

// The mixer behind its two entries (wave_common.h): `who` is the calling entry's name in every refusal, P its plane count; pan (P = 2: 2 R floats, left and right
// gain of every row) and plane_stride are not read with P = 1.
int cbx_wave_mix_run(const char* who, int P, const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, const float* pan, int R,
                     const float* gain, int G, const int* gain_idx, const float* ramp, int fade, float* out, long plane_stride, long out_len, int accumulate,
                     void* stream) {
    wm_pan_rows_t rows = {};
    cbx_wave_span_t sp;
    CBX_REQUIRE(start && flags && (P == 1 || pan), "%s: null pointer", who);
    const int rc = cbx_wave_rows(who, row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && out, "%s: null pointer", who);
    CBX_REQUIRE(out_len >= 0, "%s: out_len = %ld", who, out_len);
    CBX_REQUIRE(P == 1 || plane_stride >= out_len, "%s: plane_stride = %ld below out_len = %ld (the planes would overlap)", who, plane_stride, out_len);
    CBX_REQUIRE(fade >= 0 && (fade == 0 || ramp), "%s: fade = %d%s", who, fade, fade > 0 ? " without a ramp" : "");
    CBX_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate = %d outside {0, 1}", who, accumulate);
    CBX_REQUIRE(gain || !gain_idx, "%s: gain_idx without a gain vector", who);
    CBX_REQUIRE(!gain || G >= 1, "%s: G = %d gains", who, G);
    CBX_REQUIRE(!gain || gain_idx || G >= R, "%s: %d gains for %d rows and no gain_idx", who, G, R);
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(start[r] >= 0 && start[r] + rows.n[r] <= out_len, "%s: row %d covers [%ld, %ld) of an output of %ld", who, r, start[r], start[r] + rows.n[r], out_len);
        CBX_REQUIRE(flags[r] >= 0 && flags[r] <= 3, "%s: row %d has flags %d outside 0 .. 3", who, r, flags[r]);
        const int gi = gain_idx ? gain_idx[r] : r;
        CBX_REQUIRE(!gain || (gi >= 0 && gi < G), "%s: row %d uses gain %d of %d", who, r, gi, G);
        for (int c = 0; P == 2 && c < 2; ++c) {
            CBX_REQUIRE(fabsf(pan[2 * r + c]) < INFINITY, "%s: row %d has the %s gain %g, which is not finite", who, r, c ? "right" : "left", (double)pan[2 * r + c]);
            rows.pan[r][c] = pan[2 * r + c];
        }
        rows.start[r] = start[r];
        rows.flag[r] = (unsigned char)flags[r];
        rows.gidx[r] = gain ? gi : 0;
    }
    const cbx_wave_span_t to = {out_len, out_len, out_len > 0 ? 0 : -1, out_len};
    for (int c = 0; c < P; ++c)
        if (const int e = cbx_wave_apart(who, wav, sp, out + c * plane_stride, to, "the rows are read while other workgroups write")) return e;
    if (out_len == 0) return 0;
    const long gx = (out_len + 3 + WM_TILE - 1) / WM_TILE;  // (+ 3: out may begin up to three samples into its first quad; a last tile without an output returns)
    CBX_REQUIRE(gx <= 0x7fffffffl, "%s: %ld samples are too many for one launch", who, out_len);
    const dim3 grid((unsigned)gx), block(256);
    if (P == 1)
        hipLaunchKernelGGL(wave_mix_kernel<1>, grid, block, 0, (hipStream_t)stream, wav, (const wm_rows_t&)rows, R, gain, ramp, fade, out, 0l, out_len, accumulate);
    else
        hipLaunchKernelGGL(wave_mix_kernel<2>, grid, block, 0, (hipStream_t)stream, wav, rows, R, gain, ramp, fade, out, plane_stride, out_len, accumulate);
    return cbx_check_launch(who);
}

extern "C" int cbx_wave_mix_f32(const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, int R, const float* gain, int G,
                                const int* gain_idx, const float* ramp, int fade, float* out, long out_len, int accumulate, void* stream) {
    return cbx_wave_mix_run("wave_mix", 1, wav, row_off, row_len, start, flags, nullptr, R, gain, G, gain_idx, ramp, fade, out, 0, out_len, accumulate, stream);
}
