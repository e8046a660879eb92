// Long-form synthesis (cbx_wave_edges_f32, cbx_wave_join_f32, include/cbx.h): the waveforms of one sub-batch of text chunks are trimmed of their leading and
// trailing silence and laid out, with pauses between them and short fades at the seams, as ONE piece in one buffer -- behind the vocoder, on its stream, so that a
// sub-batch leaves the device in one copy.  The reference stops at 1000 speech tokens (tts.py:249, mtl_tts.py:328: max_new_tokens=1000, 40 s) and has no chunking.
//
// Rows: R <= 64 waveforms `wav + off[r]`, n[r] samples each, in text order; off / n / gap are HOST arrays that travel to the kernels by value (1 KiB of kernel
// arguments), so a call needs no upload.  Frame = 480 samples (one mel frame).
//
// Edges: frame f of row r covers [480 f, min(480 (f + 1), n)); m_f = its mean square in fp64.  One WAVE per frame: lane l squares and adds elements [4 l, 4 l + 4)
// and [256 + 4 l, 256 + 4 l + 4) in that order (16-byte loads where the row allows them, the same order where it does not), then a 6-step xor butterfly -- a fixed
// order per frame whatever the grid, no floating-point atomics, so the table is reproducible run to run.  The per-frame results go to a workspace; a second launch
// of the same entry (one workgroup per row) takes peak = max_f m_f and the first / last frame with m_f > peak * ratio and m_f > 0.  A row of 960 000 samples is read
// once by 500 workgroups.
//
// Join: workgroups (x, r) write the span of row r -- its kept samples [start, stop) with the fades, then its gap as zeros -- at off_r, which every workgroup derives
// itself as a prefix over the <= 64 entries of the edge table (no host round trip).  Aligned 16-byte stores inside the span, 4-byte stores at its ragged ends; nothing
// at or beyond `total` is written.  One fp32 multiply per faded sample.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WJ_FRAME = 480;
constexpr int WJ_TILE = 4096;  // output samples of one join workgroup: 256 threads x 4 quads

struct wj_rows_t : cbx_wave_rows_t {
    int gap[CBX_WAVE_MAX_ROWS];
};

// grid R x 256: the kept part of row r from its frames' mean squares
__global__ __launch_bounds__(256) void wave_edges_kernel(cbx_wave_rows_t rows, const double* __restrict__ ws, long ws_ld, double ratio, int pad, int* __restrict__ edges) {
    const int r = blockIdx.x;
    const int n = rows.n[r];
    const int nf = (int)(((long)n + WJ_FRAME - 1) / WJ_FRAME);
    const double* m = ws + (long)r * ws_ld;
    int lo, hi;
    cbx_wave_peak_edges(nf, ratio, [=](int f) { return m[f]; }, [](double v, double thr) { return v > thr && v > 0.0; }, &lo, &hi);
    if (threadIdx.x == 0) {
        int start = 0, stop = 0;
        if (hi >= 0) {
            const long f0 = (long)lo - pad, e1 = ((long)hi + 1 + pad) * WJ_FRAME;
            start = (int)((f0 > 0 ? f0 : 0) * WJ_FRAME);
            stop = (int)(e1 < n ? e1 : n);
        }
        edges[2 * r] = start;
        edges[2 * r + 1] = stop;
    }
}

// grid (ceil((max span + 3) / WJ_TILE), R) x 256: workgroup (x, r) writes quads [1024 x, 1024 (x + 1)) of row r's span, counted from the 16-byte boundary at or
// below out + off_r
__global__ __launch_bounds__(256) void wave_join_kernel(const float* __restrict__ wav, wj_rows_t rows, int R, const int* __restrict__ edges, const float* __restrict__ ramp,
                                                        int fade, int first, int last, float* __restrict__ out, int* __restrict__ layout) {
    const int r = blockIdx.y;
    long off = 0;
    int start = 0, stop = 0, L = 0, gap = 0;
    for (int q = 0; q <= r; ++q) {  // the layout prefix; the table is device data: cut into [0, n] whatever it holds
        const int n = rows.n[q];
        int a = edges[2 * q], b = edges[2 * q + 1];
        a = a < 0 ? 0 : (a > n ? n : a);
        b = b < a ? a : (b > n ? n : b);
        const int l = b - a;
        const int g = (l > 0 && !(last && q == R - 1)) ? rows.gap[q] : 0;
        if (q < r) off += (long)l + g;
        else start = a, stop = b, L = l, gap = g;
    }
    const long end = off + L + gap;  // the span of this row: out[off, end)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        layout[r] = (int)off;
        if (r == R - 1) layout[R] = (int)end;
    }
    const int F = fade < L / 2 ? fade : L / 2;
    const bool fin = !(first && r == 0 && start == 0), fout = !(last && r == R - 1 && stop == rows.n[r]);
    const float* src = wav + rows.off[r] + start;
    const bool out16 = ((uintptr_t)out & 15) == 0;
    const long q0 = out16 ? (off & ~3l) : off;  // where quad 0 of this row begins
    for (int it = 0; it < 4; ++it) {
        const long p0 = q0 + 4 * ((long)blockIdx.x * (WJ_TILE / 4) + it * 256 + threadIdx.x);
        if (p0 >= end) return;
        float v[4];
        const long i0 = p0 - off;  // (may be -3 .. -1 in the first quad)
        const bool whole = p0 >= off && p0 + 4 <= end;
        if (whole && i0 + 4 <= L && ((uintptr_t)(src + i0) & 15) == 0) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(src + i0);
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
            for (int k = 0; k < 4; ++k) v[k] = (i0 + k >= 0 && i0 + k < L) ? src[i0 + k] : 0.0f;
        }
        for (int k = 0; k < 4; ++k) {
            const long i = i0 + k;
            if (i < 0 || i >= L) continue;
            if (fin && i < F) v[k] = v[k] * ramp[i];
            else if (fout && i >= L - F) v[k] = v[k] * ramp[L - 1 - i];
        }
        if (whole && out16) {
            *reinterpret_cast<f32x4*>(out + p0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= off && p0 + k < end) out[p0 + k] = v[k];
        }
    }
}

}  // namespace

// The same frame pass for the pause control (wave_squeeze.hip; declared in cbx_common.h): ONE kernel, so its m_f are those of cbx_wave_edges_f32 bit for bit.
// ws holds R * nf doubles, nf = ceil(max n / 480) > 0.
int cbx_wave_frame_ms(const char* who, const float* wav, const long* row_off, const int* row_len, int R, long nf, double* ws, void* stream) {
    cbx_wave_rows_t rows;
    cbx_wave_span_t sp;
    const int rc = cbx_wave_rows(who, row_off, row_len, R, &rows, &sp);
    return rc ? rc : cbx_wave_block_pass<WJ_FRAME, true>(who, wav, rows, R, sp.n_max, nf, ws, stream);
}

extern "C" int cbx_wave_edges_f32(const float* wav, const long* row_off, const int* row_len, int R, double ratio, int pad, int* edges, double* ws, long ws_cap,
                                  void* stream) {
    cbx_wave_rows_t rows;
    cbx_wave_span_t sp;
    const int rc = cbx_wave_rows("wave_edges", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && edges && ws, "wave_edges: null pointer");
    CBX_REQUIRE(ratio >= 0.0 && ratio < INFINITY && pad >= 0 && pad <= (1 << 20), "wave_edges: bad threshold (ratio %g, pad %d)", ratio, pad);
    const long nf = (sp.n_max + WJ_FRAME - 1) / WJ_FRAME;
    CBX_REQUIRE(ws_cap >= (long)R * nf, "wave_edges: workspace of %ld doubles, %d rows of %ld frames need %ld", ws_cap, R, nf, (long)R * nf);
    if (nf > 0) {
        const int e = cbx_wave_block_pass<WJ_FRAME, true>("wave_edges", wav, rows, R, sp.n_max, nf, ws, stream);
        if (e) return e;
    }
    hipLaunchKernelGGL(wave_edges_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, rows, (const double*)ws, nf, ratio, pad, edges);
    return cbx_check_launch("wave_edges");
}

extern "C" int cbx_wave_join_f32(const float* wav, const long* row_off, const int* row_len, const int* gaps, int R, const int* edges, const float* ramp, int fade,
                                 int first, int last, float* out, long out_cap, int* layout, void* stream) {
    wj_rows_t rows = {};
    cbx_wave_span_t sp;
    CBX_REQUIRE(gaps, "wave_join: null pointer");
    const int rc = cbx_wave_rows("wave_join", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    long n_sum = sp.n_sum, span = 0;  // the rows with their gaps: all of them, and the longest
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(gaps[r] >= 0, "wave_join: row %d has gap %d", r, gaps[r]);
        rows.gap[r] = gaps[r];
        n_sum += gaps[r];
        span = (long)rows.n[r] + gaps[r] > span ? (long)rows.n[r] + gaps[r] : span;
    }
    CBX_REQUIRE(wav && edges && out && layout, "wave_join: null pointer");
    CBX_REQUIRE(fade >= 0 && (fade == 0 || ramp), "wave_join: fade = %d%s", fade, fade > 0 ? " without a ramp" : "");
    CBX_REQUIRE(n_sum <= 0x7fffffffl, "wave_join: %ld samples do not fit the int32 layout record", n_sum);
    CBX_REQUIRE(out_cap >= n_sum, "wave_join: out holds %ld samples, the rows and their gaps may need %ld", out_cap, n_sum);
    const long gx = (span + 3 + WJ_TILE - 1) / WJ_TILE;  // (+ 3: the span may begin up to three samples into its first quad; >= 1: the layout record is always written)
    hipLaunchKernelGGL(wave_join_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, R, edges, ramp, fade, first != 0, last != 0, out,
                       layout);
    return cbx_check_launch("wave_join");
}
