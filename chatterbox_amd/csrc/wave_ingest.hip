// Audio in (cbx_wave_ingest, cbx_wave_trim_edges_f32, include/cbx.h): the mirror image of wave_format.hip.  Raw interleaved sample bytes of up to 64 sources --
// 8-bit, 16-bit, packed 24-bit and 32-bit PCM, fp32, G.711 mu-law / A-law -- are decoded, mixed down to mono and resampled to the rate of an analysis stage in ONE
// launch, and the silence at either end of the voice encoder's input is found on the device.  This replaces the host path of every audio input, frontend.load_wav
// / resample / trim_silence (NumPy / SciPy, fp64), which restates what the reference does with librosa on the CPU (tts.py:184 `librosa.load(wav_fpath,
// sr=S3GEN_SR)`, tts.py:187 and s3gen.py:139 `librosa.resample`, vc.py:88 `librosa.load(audio, sr=S3_SR)`, voice_encoder.py:224 `librosa.effects.trim`).
//
// Ingest: one workgroup per (256 outputs, row), one output per thread, wave_format_kernel's form.  The tile's input span (at most 255 D / U + T frames) is decoded
// and mixed while it is staged: the frames' bytes go to LDS in pieces of 16 KiB -- 16-byte loads for every 16-byte unit that lies inside the piece, byte loads for
// the units at its ragged ends, nothing outside the row is read --, are decoded from there (each frame once per tile), summed over the channels in channel order
// and divided by (float)C.  The phase table is staged in LDS when it fits WI_TAB floats at its padded stride and read from global memory otherwise (44100 -> 16000:
// 160 x 56, 11025 -> 16000: 640 x 21 floats; L2-resident); either way y = sum_j tab[p][j] x[k - j] by fmaf in the order j = 0 .. T - 1 from 0.
//
// Trim: wave per block of 512 samples (fp64 sum of squares, fixed order), then one workgroup per row takes the frames of 2048 at hop 512 -- four consecutive
// blocks each -- and writes {start, stop}.  No floating-point atomics; the result does not depend on the grid or on the row's alignment.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WI_TILE = 256;
constexpr int WI_SPAN = CBX_WAVE_INGEST_MAX_SPAN;  // LDS floats of a tile's decoded span
constexpr int WI_TAB = 3456;                       // LDS floats of a staged phase table at its padded stride (larger tables are read from global memory)
constexpr int WI_RAW = 16384;                      // LDS bytes of one piece of a span's raw frames
constexpr int WT_FRAME = 2048, WT_HOP = 512;

// (not cbx_wave_rows_t: an ingest row is counted in bytes and in `long` frames)
struct wi_rows_t {
    long off[CBX_WAVE_MAX_ROWS];      // first byte of the row, from `raw`
    long out_off[CBX_WAVE_MAX_ROWS];  // first output, floats from `out`
    long n[CBX_WAVE_MAX_ROWS];        // frames of the row
};

// ITU-T G.711 expansion of a code word to the 16-bit sample
__device__ __forceinline__ int wi_mulaw(unsigned code) {
    const unsigned u = ~code & 0xFF;
    const int t = ((int)((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}

__device__ __forceinline__ int wi_alaw(unsigned code) {
    const unsigned a = (code ^ 0x55) & 0xFF;
    const int seg = (int)((a & 0x70) >> 4);
    int t = (int)((a & 0x0F) << 4);
    t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
    return (a & 0x80) ? t : -t;
}

// one sample at LDS byte pointer q (aligned to the sample size) -> fp32
__device__ __forceinline__ float wi_decode(const unsigned char* q, int enc) {
    switch (enc) {
        case CBX_WAVE_IN_U8: return ((float)q[0] - 128.0f) / 128.0f;
        case CBX_WAVE_IN_S16: return (float)*reinterpret_cast<const short*>(q) / 32768.0f;
        case CBX_WAVE_IN_S24: return (float)((int)(((unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16)) << 8) >> 8) / 8388608.0f;
        case CBX_WAVE_IN_S32: return (float)*reinterpret_cast<const int*>(q) / 2147483648.0f;
        case CBX_WAVE_IN_F32: return *reinterpret_cast<const float*>(q);
        case CBX_WAVE_IN_MULAW: return (float)wi_mulaw(q[0]) / 32768.0f;
        default: return (float)wi_alaw(q[0]) / 32768.0f;
    }
}

__host__ __device__ __forceinline__ int wi_sample_size(int enc) {
    return enc == CBX_WAVE_IN_S16 ? 2 : enc == CBX_WAVE_IN_S24 ? 3 : (enc == CBX_WAVE_IN_S32 || enc == CBX_WAVE_IN_F32) ? 4 : 1;
}

// grid (ceil(max outputs / 256), R) x 256
__global__ __launch_bounds__(256) void wave_ingest_kernel(const unsigned char* __restrict__ raw, wi_rows_t rows, const float* __restrict__ tab, int U, int D, int hl, int T,
                                                          int enc, int C, int staged, float* __restrict__ out) {
    __shared__ uint4 s_raw[WI_RAW / 16];
    __shared__ float s_x[WI_SPAN];
    __shared__ float s_tab[WI_TAB];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long n = rows.n[r];
    const long cnt = (n * U + D - 1) / D;
    const long mb = (long)blockIdx.x * WI_TILE;
    if (mb >= cnt) return;  // (uniform over the workgroup, ahead of its barriers)
    const int nt = cnt - mb < WI_TILE ? (int)(cnt - mb) : WI_TILE;
    const long k_lo = (mb * D + hl) / U - (T - 1), k_top = ((mb + nt - 1) * D + hl) / U;
    const int span = (int)(k_top - k_lo + 1);
    const long ka = k_lo > 0 ? k_lo : 0, kb = k_top + 1 < n ? k_top + 1 : n;  // the span's frames inside the row: [ka, kb)
    for (int i = tid; i < span; i += WI_TILE)
        if (k_lo + i < ka || k_lo + i >= kb) s_x[i] = 0.0f;
    const bool filter = U != D;
    const int ts = T | 1;
    if (filter && staged)
        for (int i = tid; i < U * T; i += WI_TILE) s_tab[(i / T) * ts + i % T] = tab[i];
    const int ss = wi_sample_size(enc), fb = C * ss;
    const long fp = (WI_RAW - 32) / fb;  // frames of a piece
    for (long k0 = ka; k0 < kb; k0 += fp) {
        const int nf = kb - k0 < fp ? (int)(kb - k0) : (int)fp;
        const unsigned char* g0 = raw + rows.off[r] + k0 * fb;
        const int nbytes = nf * fb;
        const int mis = (int)((uintptr_t)g0 & 15);  // the piece's units begin at the 16-byte boundary at or below its first byte
        const int units = (mis + nbytes + 15) / 16;
        __syncthreads();  // (the previous piece has been decoded)
        for (int u = tid; u < units; u += WI_TILE) {
            const int b0 = 16 * u - mis;
            uint4 v;
            if (b0 >= 0 && b0 + 16 <= nbytes) {
                v = *reinterpret_cast<const uint4*>(g0 + b0);
            } else {  // a ragged end: the bytes of the piece alone
                unsigned w[4] = {0u, 0u, 0u, 0u};
                for (int e = 0; e < 16; ++e)
                    if (b0 + e >= 0 && b0 + e < nbytes) w[e >> 2] |= (unsigned)g0[b0 + e] << (8 * (e & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            s_raw[u] = v;
        }
        __syncthreads();
        const unsigned char* sb = reinterpret_cast<const unsigned char*>(s_raw) + mis;
        for (int i = tid; i < nf; i += WI_TILE) {
            const unsigned char* q = sb + i * fb;
            float acc = wi_decode(q, enc);
            for (int ch = 1; ch < C; ++ch) acc += wi_decode(q + ch * ss, enc);
            if (C > 1) acc = acc / (float)C;
            s_x[(int)(k0 - k_lo) + i] = acc;
        }
    }
    __syncthreads();
    if (tid >= nt) return;
    const long c = (mb + tid) * D + hl;
    const int p = (int)(c % U);
    const float* x = s_x + (c / U - k_lo);
    float acc = x[0];
    if (filter) {
        acc = 0.0f;
        if (staged) {
            const float* t = s_tab + p * ts;
            for (int j = 0; j < T; ++j) acc = fmaf(t[j], x[-j], acc);
        } else {
            const float* t = tab + (long)p * T;
            for (int j = 0; j < T; ++j) acc = fmaf(t[j], x[-j], acc);
        }
    }
    out[rows.out_off[r] + mb + tid] = acc;
}

// mean square of frame f (the row padded by 1024 zeros on either side: the blocks f - 2 .. f + 1), floored at 1e-20 as trim_silence floors the RMS at 1e-10
__device__ __forceinline__ double wt_frame(const double* m, int nb, int f) {
    double s = 0.0;
    for (int b = f - 2; b <= f + 1; ++b) s += (b >= 0 && b < nb) ? m[b] : 0.0;
    return fmax(s / (double)WT_FRAME, 1e-20);
}

// grid R x 256: the kept part of row r
__global__ __launch_bounds__(256) void wave_trim_edges_kernel(cbx_wave_rows_t rows, const double* __restrict__ ws, long ws_ld, double ratio, int* __restrict__ edges) {
    const int r = blockIdx.x;
    const int n = rows.n[r];
    const int nb = (n + WT_HOP - 1) / WT_HOP, nf = 1 + n / WT_HOP;
    const double* m = ws + (long)r * ws_ld;
    int lo, hi;
    cbx_wave_peak_edges(nf, ratio, [=](int f) { return wt_frame(m, nb, f); }, [](double v, double thr) { return v > thr; }, &lo, &hi);
    if (threadIdx.x == 0) {
        int start = 0, stop = 0;
        if (hi >= 0) {
            const long e1 = ((long)hi + 1) * WT_HOP;
            start = lo * WT_HOP;
            stop = (int)(e1 < n ? e1 : n);
        }
        edges[2 * r] = start;
        edges[2 * r + 1] = stop;
    }
}

long wi_gcd(long a, long b) {
    while (b) {
        const long t = a % b;
        a = b, b = t;
    }
    return a;
}

}  // namespace

extern "C" int cbx_wave_ingest(const void* raw, const long* row_off, const long* row_frames, int R, int encoding, int channels, const float* tab, int U, int D, int T,
                               float* out, const long* out_off, long out_cap, void* stream) {
    CBX_REQUIRE(raw && row_off && row_frames && out && out_off, "wave_ingest: null pointer");
    CBX_REQUIRE(R >= 1 && R <= CBX_WAVE_MAX_ROWS, "wave_ingest: R = %d outside [1, %d]", R, CBX_WAVE_MAX_ROWS);
    CBX_REQUIRE(encoding >= CBX_WAVE_IN_U8 && encoding <= CBX_WAVE_IN_ALAW, "wave_ingest: unknown encoding %d (0 u8, 1 s16, 2 s24, 3 s32, 4 f32, 5 mulaw, 6 alaw)", encoding);
    CBX_REQUIRE(channels >= 1 && channels <= 8, "wave_ingest: %d channels outside [1, 8]", channels);
    CBX_REQUIRE(U >= 1 && D >= 1 && U <= (1 << 20) && D <= (1 << 20) && wi_gcd(U, D) == 1, "wave_ingest: U / D = %d / %d is not a reduced ratio", U, D);
    const bool filter = U != D;
    const int hl = filter ? 10 * (U > D ? U : D) : 0;
    const int Tr = filter ? (2 * hl + U) / U : 1;  // ceil((2 hl + 1) / U)
    CBX_REQUIRE(T == Tr, "wave_ingest: a table of T = %d taps for U / D = %d / %d, which has T = %d", T, U, D, Tr);
    CBX_REQUIRE(!filter || tab, "wave_ingest: null pointer (the phase table)");
    CBX_REQUIRE((WI_TILE - 1l) * D / U + T + 1 <= CBX_WAVE_INGEST_MAX_SPAN, "wave_ingest: U / D = %d / %d: a tile's span of %ld frames is over the cap of %d", U, D,
                (WI_TILE - 1l) * D / U + T + 1, CBX_WAVE_INGEST_MAX_SPAN);
    CBX_REQUIRE((long)U * T <= CBX_WAVE_INGEST_MAX_TAB, "wave_ingest: U / D = %d / %d: a table of %ld floats is over the cap of %d", U, D, (long)U * T, CBX_WAVE_INGEST_MAX_TAB);
    const int ss = wi_sample_size(encoding);
    const int al = ss == 3 ? 1 : ss;  // packed 24-bit samples are read byte by byte
    CBX_REQUIRE((uintptr_t)raw % al == 0, "wave_ingest: the buffer is not aligned to the sample size %d", al);
    // the rows are counted in bytes and `long` frames and aligned to their sample size: a loop of its own, not cbx_wave_rows
    wi_rows_t rows = {};
    long cnt[CBX_WAVE_MAX_ROWS];
    for (int r = 0; r < R; ++r) {
        const long n = row_frames[r];
        CBX_REQUIRE(n >= 0 && row_off[r] >= 0 && n < (1l << 40), "wave_ingest: row %d has %ld frames at byte %ld", r, n, row_off[r]);
        CBX_REQUIRE(row_off[r] % al == 0, "wave_ingest: row %d begins at byte %ld, not a multiple of the sample size %d", r, row_off[r], al);
        cnt[r] = (n * U + D - 1) / D;
        CBX_REQUIRE(cnt[r] <= 0x7fffffffl, "wave_ingest: row %d would produce %ld outputs in one launch", r, cnt[r]);
        rows.off[r] = row_off[r], rows.out_off[r] = out_off[r], rows.n[r] = n;
    }
    cbx_wave_span_t to;
    if (const int e = cbx_wave_packed("wave_ingest", out_off, cnt, R, out_cap, "floats", &to)) return e;
    const long cnt_max = to.n_max;
    if (cnt_max == 0) return 0;
    const long gx = (cnt_max + WI_TILE - 1) / WI_TILE;
    const int staged = filter && U * (T | 1) <= WI_TAB;
    hipLaunchKernelGGL(wave_ingest_kernel, dim3((unsigned)gx, (unsigned)R), dim3(WI_TILE), 0, (hipStream_t)stream, (const unsigned char*)raw, rows, tab, U, D, hl, T, encoding,
                       channels, staged, out);
    return cbx_check_launch("wave_ingest");
}

extern "C" int cbx_wave_trim_edges_f32(const float* wav, const long* row_off, const int* row_len, int R, double ratio, int* edges, double* ws, long ws_cap, void* stream) {
    CBX_REQUIRE(wav && row_off && row_len && edges && ws, "wave_trim_edges: null pointer");
    if (const int e = cbx_wave_count("wave_trim_edges", row_off, row_len, R)) return e;
    CBX_REQUIRE(ratio >= 0.0 && ratio < INFINITY, "wave_trim_edges: bad threshold (ratio %g)", ratio);
    cbx_wave_rows_t rows;
    cbx_wave_span_t sp;
    if (const int e = cbx_wave_rows("wave_trim_edges", row_off, row_len, R, &rows, &sp)) return e;
    const long nb = (sp.n_max + WT_HOP - 1) / WT_HOP;
    CBX_REQUIRE(ws_cap >= (long)R * nb, "wave_trim_edges: workspace of %ld doubles, %d rows of %ld blocks need %ld", ws_cap, R, nb, (long)R * nb);
    if (nb > 0) {
        const int e = cbx_wave_block_pass<WT_HOP, false>("wave_trim_edges", wav, rows, R, sp.n_max, nb, ws, stream);
        if (e) return e;
    }
    hipLaunchKernelGGL(wave_trim_edges_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, rows, (const double*)ws, nb, ratio, edges);
    return cbx_check_launch("wave_trim_edges");
}
