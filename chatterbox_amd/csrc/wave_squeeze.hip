// Pause control (cbx_wave_squeeze_f32, include/cbx.h): long silences INSIDE the waveforms of a batch are shortened to `keep` frames behind the vocoder, on its
// stream; the new lengths exist only on the device (the stats table) and travel to the host with the audio.  The reference returns what T3 sampled, holes
// included (tts.py:272, mtl_tts.py:352, tts_turbo.py:320, vc.py:104) and has no such step.
//
// Rows as cbx_wave_join_f32 takes them (HOST arrays by value).  Three launches:
//   1. the frame pass of cbx_wave_edges_f32 (wave_join.hip, cbx_wave_frame_ms: the same kernel, the same m_f bit for bit);
//   2. plan: one workgroup per row walks the row's frames in tiles of 256 -- backwards once (suffix minimum with a carry: the next non-silent frame of every
//      frame), forwards once (prefix maximum with a carry: the previous non-silent frame; with both ends of its run every frame decides alone whether it is
//      removed, however many tiles the run spans; then a prefix sum with a carry of "removed") -- and writes src[j] = source frame of output frame j, the stats and
//      the mapped edge table.  Integer scans only: xor butterflies (cbx_xor_lane) inside a wave, four wave totals through the LDS;
//   3. gather: one wave per OUTPUT frame copies its source frame (16-byte accesses where both rows allow them, 4-byte accesses elsewhere), blends the seam into
//      its last `fade` samples where the next output frame is not the next source frame, and writes the zero tail [n', n).
// Nothing depends on the grid or on a row's alignment; no atomics.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WS_FRAME = 480, WS_TILE = 256, WS_NONE = 0x7fffffff;

struct ws_rows_t : cbx_wave_rows_t {
    int keep[CBX_WAVE_MAX_ROWS];
};

template <int MASK>
__device__ __forceinline__ int ws_xor_lane(int v) {
    return __builtin_bit_cast(int, cbx_xor_lane<MASK>(__builtin_bit_cast(float, v)));
}

struct ws_min {
    static constexpr int unit = WS_NONE;
    __device__ static int op(int a, int b) { return a < b ? a : b; }
};
struct ws_max {
    static constexpr int unit = -1;
    __device__ static int op(int a, int b) { return a > b ? a : b; }
};
struct ws_add {
    static constexpr int unit = 0;
    __device__ static int op(int a, int b) { return a + b; }
};

// Inclusive scan of v over the 256 threads of the workgroup (UP: over threads <= tid, else over threads >= tid); *total = the reduction over all 256.
// Every thread calls it; two barriers.  s_w: 4 ints of LDS.
template <class OP, bool UP>
__device__ __forceinline__ int ws_block_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pre = v, tot = v, o;
#define WS_STEP(M)                                    \
    o = ws_xor_lane<M>(tot);                          \
    if (((lane & M) != 0) == UP) pre = OP::op(pre, o); \
    tot = OP::op(tot, o);
    WS_STEP(1) WS_STEP(2) WS_STEP(4) WS_STEP(8) WS_STEP(16) WS_STEP(32)
#undef WS_STEP
    if (lane == 0) s_w[wave] = tot;
    __syncthreads();
    int all = OP::unit;
    for (int w = 0; w < 4; ++w) {
        const int t = s_w[w];
        all = OP::op(all, t);
        if (UP ? w < wave : w > wave) pre = OP::op(pre, t);
    }
    __syncthreads();
    *total = all;
    return pre;
}

// grid R x 256: the plan of row r.  ms: the frame pass's table (ld doubles per row); nxt / src: ld ints per row each.
__global__ __launch_bounds__(256) void wave_squeeze_plan_kernel(ws_rows_t rows, const double* __restrict__ ms, long ld, double ratio, int* __restrict__ nxt,
                                                                int* __restrict__ src, int* __restrict__ edges, int* __restrict__ stats) {
    __shared__ double s_pk[256];
    __shared__ int s_w[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int n = rows.n[r], K = rows.keep[r];
    const int nf = (int)(((long)n + WS_FRAME - 1) / WS_FRAME);
    const int tiles = (nf + WS_TILE - 1) / WS_TILE;
    const double* m = ms + (long)r * ld;
    int* nx = nxt + (long)r * ld;
    int* sr = src + (long)r * ld;
    int e_in[2] = {0, n};  // the row's edge entry, cut into [0, n] as the join cuts it
    if (edges) {
        int a = edges[2 * r], b = edges[2 * r + 1];
        a = a < 0 ? 0 : (a > n ? n : a);
        b = b < a ? a : (b > n ? n : b);
        e_in[0] = a, e_in[1] = b;
    }
    double pk = 0.0;  // the peak as the edges kernel takes it: fmax from 0, a NaN frame is ignored
    for (int f = tid; f < nf; f += 256) pk = fmax(pk, m[f]);
    s_pk[tid] = pk;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_pk[tid] = fmax(s_pk[tid], s_pk[tid + s]);
        __syncthreads();
    }
    const double thr = s_pk[0] * ratio;
    // backwards: nx[f] = the first non-silent frame at or behind f (WS_NONE: none)
    int carry = WS_NONE, total;
    for (int t = tiles - 1; t >= 0; --t) {
        const int f = t * WS_TILE + tid;
        int v = WS_NONE;
        if (f < nf) {
            const double mf = m[f];
            if (!(mf <= thr || mf == 0.0)) v = f;  // (a NaN frame is not silent)
        }
        const int suf = ws_block_scan<ws_min, false>(v, s_w, &total);
        if (f < nf) nx[f] = suf < carry ? suf : carry;
        carry = total < carry ? total : carry;
    }
    // forwards: the previous non-silent frame, the decision, the count of removed frames ahead
    const int h = K - K / 2, tl = K / 2;
    int prev_c = -1, rem_c = 0, cut_c = 0;
    for (int t = 0; t < tiles; ++t) {
        const int f = t * WS_TILE + tid;
        bool silent = false;
        if (f < nf) {
            const double mf = m[f];
            silent = mf <= thr || mf == 0.0;
        }
        int prev = ws_block_scan<ws_max, true>((f < nf && !silent) ? f : -1, s_w, &total);
        prev = prev > prev_c ? prev : prev_c;
        prev_c = total > prev_c ? total : prev_c;
        int rem = 0, cut = 0;
        if (silent && K > 0 && prev >= 0) {  // (prev < 0: leading silence)
            const int a = prev + 1, b = nx[f];  // the run [a, b); b == WS_NONE: trailing silence
            if (b != WS_NONE && b - a > K && f >= a + h && f < b - tl) rem = 1, cut = f == a + h;
        }
        const int incl = ws_block_scan<ws_add, true>(rem | (cut << 16), s_w, &total);  // (<= 256 of either per tile)
        const int before = rem_c + (incl & 0xffff) - rem;
        rem_c += total & 0xffff, cut_c += total >> 16;
        if (f < nf) {
            if (!rem) sr[f - before] = f;
            if (edges)
                for (int k = 0; k < 2; ++k) {
                    const int p = e_in[k];
                    if (p < n && p / WS_FRAME == f) edges[2 * r + k] = rem ? WS_FRAME * (f - before) : p - WS_FRAME * before;
                }
        }
    }
    if (tid == 0) {
        const int n_new = n - WS_FRAME * rem_c;
        stats[4 * r] = n_new, stats[4 * r + 1] = cut_c, stats[4 * r + 2] = rem_c, stats[4 * r + 3] = n;
        if (edges)
            for (int k = 0; k < 2; ++k)
                if (e_in[k] >= n) edges[2 * r + k] = n_new;
    }
}

// grid (ceil(max frames / 4), R) x 256: wave w of workgroup (x, r) owns OUTPUT frame j = 4 x + w of row r
__global__ __launch_bounds__(256) void wave_squeeze_gather_kernel(const float* __restrict__ wav, ws_rows_t rows, const int* __restrict__ src, long ld,
                                                                  const int* __restrict__ stats, const float* __restrict__ ramp, int fade, float* __restrict__ out) {
    const int r = blockIdx.y, lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int n = rows.n[r];
    const long d0 = (long)j * WS_FRAME;
    if (d0 >= n) return;  // (wave-uniform)
    const int total = n - d0 < WS_FRAME ? (int)(n - d0) : WS_FRAME;  // what this wave writes
    const int nk = (int)(((long)stats[4 * r] + WS_FRAME - 1) / WS_FRAME);  // kept frames
    const int* sr = src + (long)r * ld;
    const float* x = wav + rows.off[r];
    float* y = out + rows.off[r] + d0;
    int kept = 0, F = 0;
    const float *p = x, *p2 = x;
    if (j < nk) {
        const int s = sr[j];
        const long s0 = (long)s * WS_FRAME;
        kept = n - s0 < WS_FRAME ? (int)(n - s0) : WS_FRAME;
        p = x + s0;
        if (j + 1 < nk) {
            const int s2 = sr[j + 1];
            if (s2 != s + 1) F = fade, p2 = x + (long)(s2 - 1) * WS_FRAME;  // a seam: both frames are whole
        }
    }
    const bool vec = (((uintptr_t)p | (uintptr_t)y) & 15) == 0;
    for (int q = lane; q < WS_FRAME / 4; q += 64) {
        const int e = 4 * q;
        if (e >= total) break;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec && e + 4 <= kept) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + e);
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
            for (int k = 0; k < 4; ++k)
                if (e + k < kept) v[k] = p[e + k];
        }
        if (e + 4 > WS_FRAME - F)
            for (int k = 0; k < 4; ++k) {
                const int i = e + k - (WS_FRAME - F);
                if (i >= 0) v[k] = __builtin_fmaf(ramp[i], p2[e + k] - v[k], v[k]);
            }
        if (vec && e + 4 <= total) {
            *reinterpret_cast<f32x4*>(y + e) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = 0; k < 4; ++k)
                if (e + k < total) y[e + k] = v[k];
        }
    }
}

}  // namespace

extern "C" int cbx_wave_squeeze_f32(const float* wav, const long* row_off, const int* row_len, const int* keep, int R, double ratio, const float* ramp, int fade,
                                    float* out, long out_cap, int* edges, int* stats, void* ws, long ws_cap, void* stream) {
    CBX_REQUIRE(wav && row_off && row_len && keep && out && stats && ws, "wave_squeeze: null pointer");
    ws_rows_t rows = {};
    cbx_wave_span_t sp;  // the rows span [lo, hi) of either buffer
    int rc = cbx_wave_rows("wave_squeeze", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(keep[r] == 0 || keep[r] >= 2, "wave_squeeze: row %d keeps %d frames of a pause (0: the row is copied; else >= 2)", r, keep[r]);
        rows.keep[r] = keep[r];
    }
    CBX_REQUIRE(ratio >= 0.0 && ratio < INFINITY, "wave_squeeze: bad threshold (ratio %g)", ratio);
    CBX_REQUIRE(fade >= 0 && fade <= WS_FRAME, "wave_squeeze: fade = %d outside [0, %d]", fade, WS_FRAME);
    CBX_REQUIRE(fade == 0 || ramp, "wave_squeeze: fade = %d without a ramp", fade);
    CBX_REQUIRE(out_cap >= sp.hi, "wave_squeeze: out holds %ld samples, the furthest row ends at %ld", out_cap, sp.hi);
    if ((rc = cbx_wave_apart("wave_squeeze", wav, sp, out, sp, "the rows are gathered, not moved in place"))) return rc;
    const long nf = (sp.n_max + WS_FRAME - 1) / WS_FRAME;
    const long need = 16 * (long)R * nf;  // R * nf doubles (m_f), R * nf ints (next non-silent frame), R * nf ints (src)
    CBX_REQUIRE(ws_cap >= need && ((uintptr_t)ws & 7) == 0, "wave_squeeze: workspace of %ld bytes at %p, %d rows of %ld frames need %ld on an 8-byte boundary", ws_cap, ws,
                R, nf, need);
    double* ms = (double*)ws;
    int* nxt = (int*)(ms + (long)R * nf);
    int* src = nxt + (long)R * nf;
    if (nf > 0) {
        const int e = cbx_wave_frame_ms("wave_squeeze", wav, row_off, row_len, R, nf, ms, stream);
        if (e) return e;
    }
    hipLaunchKernelGGL(wave_squeeze_plan_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, rows, (const double*)ms, nf, ratio, nxt, src, edges, stats);
    const int e = cbx_check_launch("wave_squeeze");
    if (e || nf == 0) return e;  // (every row empty: the stats and the table are written, there is nothing to gather)
    hipLaunchKernelGGL(wave_squeeze_gather_kernel, dim3((unsigned)((nf + 3) / 4), (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, (const int*)src, nf,
                       (const int*)stats, ramp, fade, out);
    return cbx_check_launch("wave_squeeze");
}
