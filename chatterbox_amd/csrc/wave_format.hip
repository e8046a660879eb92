// Output formats (cbx_wave_format_f32, include/cbx.h): the waveforms of a batch, or the new samples of a round of a stream, resampled from 24 kHz to the delivery
// rate and encoded (fp32, PCM16, G.711 mu-law / A-law) in ONE launch, ahead of the only copy to the host.  The reference returns 24 kHz fp32 (tts.py:272,
// mtl_tts.py:352, tts_turbo.py:320, vc.py:104: `torch.from_numpy(wav).unsqueeze(0)`) and leaves the conversion to the caller; the definition of resampling is the
// one this project already uses for every voice prompt, scipy.signal.resample_poly (frontend.resample).
//
// Rows: R <= 64 pieces `wav + off[r]` of len[r] samples, as cbx_wave_join_f32 takes them; every per-row number travels to the kernel by value (2.5 KiB of kernel
// arguments), so a call needs no upload.  U / D = rate / 24000 reduced, hl = 10 max(U, D), tab[p][j] = h[p + j U] the fp32 phase table of the host's fp64 design
// (T taps per output).  Output m of a row: c = m D + hl, p = c mod U, k_hi = c div U, y = sum_j tab[p][j] x[k_hi - j] by fmaf in the order j = 0 .. T - 1 from 0.
//
// One workgroup per (256 outputs, row), one output per thread.  The tile's input span -- at most 255 D / U + T + 4 <= 833 floats; absolute samples, read from the
// history below n0, from the piece in [n0, n0 + L), zero elsewhere -- and the phase table are staged in LDS; the table's row stride is odd, so lanes with
// different p fall on different banks.  The span begins where the piece's pointer is 16-byte aligned: quads inside the piece are one 16-byte load whatever the
// row's own alignment.  Workgroup 0 of a row also writes the row's next history (the last H samples up to n0 + L) into the OTHER history buffer.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WF_TILE = 256;
constexpr int WF_SPAN = 1024;       // LDS floats of a tile's input span (the entry checks 255 D / U + T + 8 against it)
constexpr int WF_TAB = 147 * 23;    // LDS floats of the phase table at its padded stride: U <= 147 phases of T <= 22 taps there, 61 taps at U = 1
constexpr int WF_IN_RATE = 24000;

struct wf_rows_t : cbx_wave_rows_t {       // (the core: the pieces, L = n[r] samples each)
    long out_off[CBX_WAVE_MAX_ROWS];  // first output of the launch, elements from `out`
    long n0[CBX_WAVE_MAX_ROWS];       // inputs consumed before this piece
    long m0[CBX_WAVE_MAX_ROWS];       // outputs produced before this launch
    int cnt[CBX_WAVE_MAX_ROWS];       // outputs of this launch: m0 <= m < m0 + cnt
};

// clamp(rintf(y * 32768), -32768, 32767), ties to even, NaN -> 0
__device__ __forceinline__ int wf_s16(float y) {
    if (!(y == y)) return 0;
    const float s = rintf(y * 32768.0f);
    return (int)fminf(fmaxf(s, -32768.0f), 32767.0f);
}

// G.711 mu-law of a 16-bit sample, on its upper 14 bits (bias 33, eight segments, complemented code word)
__device__ __forceinline__ unsigned char wf_mulaw(int pcm) {
    int v = pcm >> 2, mask = 0xFF;
    if (v < 0) v = -v, mask = 0x7F;
    v += 33;
    int seg = 0;
    while (seg < 8 && v > (0x40 << seg) - 1) ++seg;
    if (seg >= 8) return (unsigned char)(0x7F ^ mask);
    return (unsigned char)(((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask);
}

// G.711 A-law of a 16-bit sample, on its upper 13 bits (even-bit inversion)
__device__ __forceinline__ unsigned char wf_alaw(int pcm) {
    int v = pcm >> 3, mask = 0xD5;
    if (v < 0) v = -v - 1, mask = 0x55;
    int seg = 0;
    while (seg < 8 && v > (0x20 << seg) - 1) ++seg;
    if (seg >= 8) return (unsigned char)(0x7F ^ mask);
    return (unsigned char)(((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 0xF)) ^ mask);
}

// absolute sample k of a row: history below n0, the piece in [n0, n0 + L), zero elsewhere
__device__ __forceinline__ float wf_sample(const float* piece, const float* hist, long n0, long L, int H, long k) {
    if (k >= n0) return k < n0 + L ? piece[k - n0] : 0.0f;
    return (hist && k >= n0 - H) ? hist[k - (n0 - H)] : 0.0f;
}

// grid (max(1, ceil(max cnt / 256)), R) x 256
__global__ __launch_bounds__(256) void wave_format_kernel(const float* __restrict__ wav, wf_rows_t rows, const float* __restrict__ tab, int U, int D, int hl, int T,
                                                          int H, int enc, const float* __restrict__ hist_in, float* __restrict__ hist_out, void* __restrict__ out) {
    __shared__ float s_x[WF_SPAN];
    __shared__ float s_tab[WF_TAB];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long n0 = rows.n0[r], L = rows.n[r], cnt = rows.cnt[r];
    const float* piece = wav + rows.off[r];
    const float* hist = hist_in ? hist_in + (long)r * H : nullptr;
    if (blockIdx.x == 0 && hist_out && tid < H) hist_out[(long)r * H + tid] = wf_sample(piece, hist, n0, L, H, n0 + L - H + tid);
    const long mb = (long)blockIdx.x * WF_TILE;
    if (mb >= cnt) return;  // (uniform over the workgroup, ahead of its barrier)
    const int nt = cnt - mb < WF_TILE ? (int)(cnt - mb) : WF_TILE;
    const long m_first = rows.m0[r] + mb;
    const long k_lo = (m_first * D + hl) / U - (T - 1), k_top = ((m_first + nt - 1) * D + hl) / U;
    // the span begins at most three samples below k_lo, where piece + (ks - n0) is a 16-byte boundary
    const long mis = (k_lo - n0 + (long)(((uintptr_t)piece >> 2) & 3)) & 3;
    const long ks = k_lo - mis;
    const int span = (int)(k_top - ks + 1);
    for (int q = tid; 4 * q < span; q += WF_TILE) {
        const long k = ks + 4 * q;
        float v[4];
        if (k >= n0 && k + 4 <= n0 + L) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(piece + (k - n0));
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
            for (int e = 0; e < 4; ++e) v[e] = wf_sample(piece, hist, n0, L, H, k + e);
        }
        for (int e = 0; e < 4; ++e) s_x[4 * q + e] = v[e];
    }
    const bool filter = !(U == 1 && D == 1);  // 24000 -> 24000: y = x
    const int ts = T | 1;
    if (filter)
        for (int i = tid; i < U * T; i += WF_TILE) s_tab[(i / T) * ts + i % T] = tab[i];
    __syncthreads();
    if (tid >= nt) return;
    const long c = (m_first + tid) * D + hl;
    const int p = (int)(c % U);
    const float* x = s_x + (c / U - ks);
    float acc = x[0];
    if (filter) {
        const float* t = s_tab + p * ts;
        acc = 0.0f;
        for (int j = 0; j < T; ++j) acc = fmaf(t[j], x[-j], acc);
    }
    const long o = rows.out_off[r] + mb + tid;
    if (enc == 0) {
        static_cast<float*>(out)[o] = acc;
    } else if (enc == 1) {
        static_cast<short*>(out)[o] = (short)wf_s16(acc);
    } else {
        const int s = wf_s16(acc);
        static_cast<unsigned char*>(out)[o] = enc == 2 ? wf_mulaw(s) : wf_alaw(s);
    }
}

struct wf_rate_t {
    int rate, U, D;
};
const wf_rate_t WF_RATES[] = {{8000, 1, 3}, {16000, 2, 3}, {22050, 147, 160}, {24000, 1, 1}, {32000, 4, 3}, {44100, 147, 80}, {48000, 2, 1}};

}  // namespace

extern "C" int cbx_wave_format_f32(const float* wav, const long* row_off, const int* row_len, int R, int rate, int encoding, const float* tab, int U, int T,
                                   const long* n0, const long* m0, const int* fin, const float* hist_in, float* hist_out, void* out, const long* out_off,
                                   long out_cap, void* stream) {
    CBX_REQUIRE(wav && row_off && row_len && out && out_off, "wave_format: null pointer");
    if (const int e = cbx_wave_count("wave_format", row_off, row_len, R)) return e;
    CBX_REQUIRE(encoding >= 0 && encoding <= 3, "wave_format: unknown encoding %d (0 f32, 1 s16, 2 mulaw, 3 alaw)", encoding);
    const wf_rate_t* rt = nullptr;
    for (const wf_rate_t& c : WF_RATES)
        if (c.rate == rate) rt = &c;
    CBX_REQUIRE(rt, "wave_format: no conversion from %d to %d samples per second", WF_IN_RATE, rate);
    const bool filter = !(rt->U == 1 && rt->D == 1);
    const int UD = rt->U > rt->D ? rt->U : rt->D;
    const int hl = filter ? 10 * UD : 0;
    const int Tr = (2 * hl + rt->U) / rt->U, H = (2 * hl + rt->U - 1) / rt->U;  // ceil((2 hl + 1) / U), ceil(2 hl / U)
    CBX_REQUIRE(U == rt->U && T == Tr, "wave_format: a table of U = %d, T = %d for the rate %d, which has U = %d, T = %d", U, T, rate, rt->U, Tr);
    CBX_REQUIRE(!filter || tab, "wave_format: null pointer (the phase table)");
    CBX_REQUIRE((WF_TILE - 1l) * rt->D / rt->U + T + 8 <= WF_SPAN && rt->U * (T | 1) <= WF_TAB, "wave_format: the rate %d does not fit the kernel's LDS", rate);
    CBX_REQUIRE((n0 && m0 && fin) || (!n0 && !m0 && !fin), "wave_format: n0, m0 and final go together (all NULL: the one-shot call)");
    CBX_REQUIRE(!hist_out || hist_out != hist_in, "wave_format: the next history needs a buffer of its own");
    wf_rows_t rows = {};
    cbx_wave_span_t sp;
    if (const int e = cbx_wave_rows("wave_format", row_off, row_len, R, &rows, &sp)) return e;
    long cnt[CBX_WAVE_MAX_ROWS];
    for (int r = 0; r < R; ++r) {
        const long a = n0 ? n0[r] : 0, b = m0 ? m0[r] : 0;
        CBX_REQUIRE(a >= 0 && b >= 0 && a < (1l << 48) && b < (1l << 48), "wave_format: row %d continues at n0 = %ld, m0 = %ld", r, a, b);
        CBX_REQUIRE(a == 0 || hist_in || H == 0, "wave_format: row %d continues at n0 = %ld without a history", r, a);
        const long N = a + row_len[r];
        long m1;
        if (!fin || fin[r]) {
            m1 = (N * rt->U + rt->D - 1) / rt->D;
        } else {  // outputs whose taps all lie below N: floor(((N - 1) U - hl) / D) + 1
            const long num = (N - 1) * rt->U - hl;
            m1 = num < 0 ? 0 : num / rt->D + 1;
        }
        cnt[r] = m1 > b ? m1 - b : 0;
        CBX_REQUIRE(cnt[r] <= 0x7fffffffl, "wave_format: row %d would produce %ld outputs in one launch", r, cnt[r]);
        rows.out_off[r] = out_off[r], rows.n0[r] = a, rows.m0[r] = b, rows.cnt[r] = (int)cnt[r];
    }
    cbx_wave_span_t to;
    if (const int e = cbx_wave_packed("wave_format", out_off, cnt, R, out_cap, "elements", &to)) return e;
    const long cnt_max = to.n_max;
    const bool carry = hist_out && H > 0;
    if (cnt_max == 0 && !carry) return 0;
    const long gx = cnt_max > 0 ? (cnt_max + WF_TILE - 1) / WF_TILE : 1;
    hipLaunchKernelGGL(wave_format_kernel, dim3((unsigned)gx, (unsigned)R), dim3(WF_TILE), 0, (hipStream_t)stream, wav, rows, (const float*)tab, rt->U, rt->D, hl, T, H,
                       encoding, H > 0 ? hist_in : (const float*)nullptr, carry ? hist_out : (float*)nullptr, out);
    return cbx_check_launch("wave_format");
}
