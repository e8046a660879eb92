// Loudness (cbx_wave_loudness_f32, cbx_wave_gain_f32, include/cbx.h): the integrated loudness (ITU-R BS.1770-4, one channel) and the sample peak of the waveforms
// of a batch, the gain that brings each to its LUFS target under a peak ceiling, and the multiply that applies it -- behind the vocoder, on its stream, ahead of
// the only copy to the host.  The reference normalises only Turbo's voice prompt, on the host with pyloudnorm (tts_turbo.py:223-239); its outputs are not levelled.
//
// Rows: R <= 64 waveforms `wav + off[r]`, n[r] samples each; off / n / target are HOST arrays that travel to the kernels by value (1.3 KiB of kernel arguments), so
// a call needs no upload.  hop = fs / 10 samples; segment s of a row covers [s hop, (s + 1) hop).
//
// The K-weighting is a 4th-order IIR whose high pass has a double pole at ~0.9901 (24 kHz): state and sums are fp64.  DESIGN CHOSEN: the exact three-phase form,
// not the zero-state warm-up.  The cascade (transposed direct form II, as scipy.signal.lfilter runs it) is linear in its 4-vector state: over k samples
// state' = A^k state + (the zero-state response), A the 4 x 4 transition matrix.  The entry builds A from the coefficients on the host and passes A^(c 2^i),
// i = 0 .. 5, and A^hop by value (c = ceil(hop / 64)).
//   1. One WAVE per whole segment; lane l owns the contiguous sub-chunk [s hop + l c, s hop + (l + 1) c) and runs it from zero state; a 6-step Hillis-Steele scan
//      over the lanes (v_l += A^(c d) v_(l-d), d = 1, 2, .. 32: four 8-byte lane shifts and one 4 x 4 product per step) leaves in lane l the state at the end of
//      its sub-chunk for a segment entered at zero, so lane l - 1 holds lane l's incoming state.  The last lane with samples reruns its sub-chunk from that and
//      stores the segment's zero-state end state v_s.
//   2. One workgroup per row chains the segments, s_(k+1) = A^hop s_k + v_k, in place (staged through LDS, one lane walks the few hundred steps).
//   3. The launch of 1. again, lane 0 entering at the segment's true state: the same scan now gives every lane its TRUE incoming state; each lane reruns its
//      sub-chunk from it, adds the squares of the filtered samples and takes max |x|; a 6-step xor butterfly gives E_s and the segment's peak.
// 2 c = 76 steps per lane at 24 kHz (a warm-up of 4096 samples per lane would be 4134 and is approximate).  Every order is fixed whatever the grid or the row's
// alignment and there are no floating-point atomics, so the numbers are reproducible run to run.  The last, incomplete segment of a row is read for the peak only.
//
// A last launch, one workgroup per row, forms the 400 ms blocks from the E_s, applies the two gates and computes L, the peak and the gain (strided partial sums,
// then a fixed LDS tree).  A row that holds a NaN has a NaN peak; its segments from the first non-finite E_s on count as NaN (as the recursion would leave them),
// and a block with a NaN passes no gate.
//
// Gain: workgroups (x, r) multiply row r by gain[r] in place: 16-byte accesses counted from the 16-byte boundary at or below the row's first sample, 4-byte
// accesses at the ragged ends; nothing outside the rows is touched.
//
// The running meter (cbx_wave_loudness_push_f32): the same meter fed piece by piece.  Per row a record on the device -- the cascade's state on entry to the first
// segment that is not complete, the running peak, the table of the E_s -- and the t = n0 mod hop samples of that segment in a tail buffer (two, ping-pong).  The
// whole segments of tail ++ piece go through the SAME per-segment code as above (wl_segment, a template over where sample i comes from: -ffp-contract=on fuses per
// source expression, so one source is one arithmetic), the chain starts from the record's state instead of zero, and the row step reads the record's table: after
// any sequence of pushes the numbers are bit for bit the one-shot meter's over the concatenation.  One workgroup per row also takes max |piece| into the running
// peak and copies the (t + L) mod hop left-over samples to the other tail buffer.
#include <math.h>

#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

namespace {

constexpr int WL_CHAIN = 1024;  // segments of one LDS tile of the chain
constexpr int WL_TILE = 4096;  // samples of one gain workgroup: 256 threads x 4 quads

struct wl_coef_t {
    double c[10];  // b0 b1 b2 a1 a2 of the shelf, then of the high pass
};
struct wl_pow_t {
    double m[7][16];  // row-major 4 x 4: A^(c 2^i) for i = 0 .. 5, then A^hop
};
struct wl_target_t {
    double t[CBX_WAVE_MAX_ROWS];
};
struct wl_n0_t {
    long v[CBX_WAVE_MAX_ROWS];  // samples a running meter has consumed, per row
};
constexpr int WL_REC = 8;  // doubles of a running meter's record ahead of its E table: state[4], peak, three zeros

// where sample i of a segment pass comes from: a row of the batch, or the virtual signal tail[0, t) ++ piece of a running meter
struct wl_src_row_t {
    const float* p;
    __device__ __forceinline__ float operator()(long i) const { return p[i]; }
};
struct wl_src_cat_t {
    const float* tail;
    const float* p;
    long t;
    __device__ __forceinline__ float operator()(long i) const { return i < t ? tail[i] : p[i - t]; }
};

__device__ __forceinline__ bool wl_finite(double v) { return fabs(v) < INFINITY; }

// one sample through the two biquads (transposed direct form II); s[0..1] the shelf's state, s[2..3] the high pass's
__host__ __device__ __forceinline__ double wl_step(const wl_coef_t& k, double* s, double x) {
    const double u = k.c[0] * x + s[0];
    s[0] = k.c[1] * x - k.c[3] * u + s[1];
    s[1] = k.c[2] * x - k.c[4] * u;
    const double y = k.c[5] * u + s[2];
    s[2] = k.c[6] * u - k.c[8] * y + s[3];
    s[3] = k.c[7] * u - k.c[9] * y;
    return y;
}

// v += M t
__device__ __forceinline__ void wl_mac(const double* M, const double* t, double* v) {
    for (int q = 0; q < 4; ++q) v[q] += M[4 * q] * t[0] + M[4 * q + 1] * t[1] + M[4 * q + 2] * t[2] + M[4 * q + 3] * t[3];
}

// Workspace, in doubles, ld = segments of the longest row: [0, 4 R ld) the segment states (r ld + s) * 4 + q -- the zero-state end state v_s after pass 0, the
// incoming state s_s after the chain --, then E at 4 R ld + r ld + s and the segments' peaks at 5 R ld + r ld + s.
// One WAVE on segment s of the n samples x(0 .. n): fin = 0: v_s of a whole segment -> state; fin = 1: entered at `state`, E_s -> *e_out and the segment's peak ->
// *p_out (p_out NULL: no peaks are kept, and an incomplete segment is nobody's business)
template <class Src>
__device__ __forceinline__ void wl_segment(const Src& x, long n, long s, const wl_coef_t& k, const wl_pow_t& pw, int hop, int fin, double* state, double* e_out,
                                           double* p_out) {
    const int lane = threadIdx.x & 63;
    const long s0 = s * hop;
    if (s0 >= n) return;  // (wave-uniform, as every branch below that holds a lane exchange)
    const long cnt = n - s0 < hop ? n - s0 : (long)hop;
    const bool whole = cnt == hop;
    if (!whole && (!fin || !p_out)) return;
    const long c = (hop + 63) / 64;
    long a = s0 + lane * c, b = a + c;
    b = b < s0 + cnt ? b : s0 + cnt;
    a = a < b ? a : b;
    double e = 0.0;
    float pk = 0.0f;
    int bad = 0;
    if (whole) {
        double in[4] = {0.0, 0.0, 0.0, 0.0}, v[4], t[4];
        if (fin && lane == 0)
            for (int q = 0; q < 4; ++q) in[q] = state[q];
        for (int q = 0; q < 4; ++q) v[q] = in[q];
        for (long i = a; i < b; ++i) wl_step(k, v, (double)x(i));
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            for (int q = 0; q < 4; ++q) t[q] = __shfl_up(v[q], 1u << i);
            if (lane >= (1 << i)) wl_mac(pw.m[i], t, v);
        }
        for (int q = 0; q < 4; ++q) t[q] = __shfl_up(v[q], 1u);
        if (lane > 0)
            for (int q = 0; q < 4; ++q) in[q] = t[q];
        if (!fin) {
            if (lane == (int)((hop - 1) / c)) {  // the last lane with samples: the segment's end state
                for (long i = a; i < b; ++i) wl_step(k, in, (double)x(i));
                for (int q = 0; q < 4; ++q) state[q] = in[q];
            }
            return;
        }
        for (long i = a; i < b; ++i) {
            const float xi = x(i);
            const double y = wl_step(k, in, (double)xi);
            e += y * y;
            pk = fmaxf(pk, fabsf(xi));
            bad |= !(xi == xi);
        }
    } else {  // the incomplete segment at the end of a row belongs to no block: its peak only
        for (long i = a; i < b; ++i) {
            const float xi = x(i);
            pk = fmaxf(pk, fabsf(xi));
            bad |= !(xi == xi);
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        e += __shfl_xor(e, m);
        pk = fmaxf(pk, __shfl_xor(pk, m));
        bad |= __shfl_xor(bad, m);
    }
    if (lane == 0) {
        *e_out = e;
        if (p_out) *p_out = bad ? (double)NAN : (double)pk;
    }
}

// grid (ceil(segments / 4), R) x 256: wave w of workgroup (x, r) owns segment 4 x + w of row r.  fin = 0: v_s of every whole segment; fin = 1: E_s and the peak
__global__ __launch_bounds__(256) void wave_loud_seg_kernel(const float* __restrict__ wav, cbx_wave_rows_t rows, int R, wl_coef_t k, wl_pow_t pw, int hop, int fin,
                                                            double* __restrict__ ws, long ld) {
    const int r = blockIdx.y;
    const long s = (long)blockIdx.x * 4 + (long)(threadIdx.x >> 6);
    wl_segment(wl_src_row_t{wav + rows.off[r]}, (long)rows.n[r], s, k, pw, hop, fin, ws + ((long)r * ld + s) * 4, ws + (4l * R + r) * ld + s, ws + (5l * R + r) * ld + s);
}

// The running meter's launch of the same: grid (ceil(K_max / 4), R) x 256 over the K_r whole segments of tail_r[0, t_r) ++ piece_r.  ws: the segment states alone,
// (r ld + s) * 4 + q, ld = K_max; E_(S0 + s) goes to the row's record rec + r rec_ld
__global__ __launch_bounds__(256) void wave_loud_push_seg_kernel(const float* __restrict__ wav, cbx_wave_rows_t rows, wl_n0_t n0, const float* __restrict__ tail, wl_coef_t k,
                                                                 wl_pow_t pw, int hop, int fin, double* __restrict__ ws, long ld, double* __restrict__ rec, long rec_ld) {
    const int r = blockIdx.y;
    const long s = (long)blockIdx.x * 4 + (long)(threadIdx.x >> 6);
    const long t = n0.v[r] % hop, S0 = n0.v[r] / hop, n = t + rows.n[r];
    if (s >= n / hop) return;  // (wave-uniform) whole segments only: s < K_r <= ld, S0 + s < seg_cap
    wl_segment(wl_src_cat_t{tail + (long)r * hop, wav + rows.off[r], t}, n, s, k, pw, hop, fin, ws + ((long)r * ld + s) * 4, rec + (long)r * rec_ld + WL_REC + S0 + s,
               (double*)nullptr);
}

// v_s -> the incoming state s_s of the S segments at st, in place: s_0 = cur (thread 0's), s_(k+1) = A^hop s_k + v_k; cur leaves as s_S
__device__ __forceinline__ void wl_chain(double* sm, double* st, long S, const wl_pow_t& pw, double* cur) {
    const int tid = threadIdx.x;
    for (long k0 = 0; k0 < S; k0 += WL_CHAIN) {
        const int m = S - k0 < WL_CHAIN ? (int)(S - k0) : WL_CHAIN;
        for (int i = tid; i < 4 * m; i += 256) sm[i] = st[4 * k0 + i];
        __syncthreads();
        if (tid == 0) {
            for (int j = 0; j < m; ++j) {
                double v[4], nx[4];
                for (int q = 0; q < 4; ++q) v[q] = sm[4 * j + q], sm[4 * j + q] = cur[q], nx[q] = v[q];
                wl_mac(pw.m[6], cur, nx);
                for (int q = 0; q < 4; ++q) cur[q] = nx[q];
            }
        }
        __syncthreads();
        for (int i = tid; i < 4 * m; i += 256) st[4 * k0 + i] = sm[i];
        __syncthreads();
    }
}

// grid R x 256: the chain over every whole segment of row r, from zero state
__global__ __launch_bounds__(256) void wave_loud_chain_kernel(cbx_wave_rows_t rows, wl_pow_t pw, int hop, double* __restrict__ ws, long ld) {
    __shared__ double sm[4 * WL_CHAIN];
    const int r = blockIdx.x;
    double cur[4] = {0.0, 0.0, 0.0, 0.0};  // (lane 0's)
    wl_chain(sm, ws + (long)r * ld * 4, rows.n[r] / hop, pw, cur);
}

// grid R x 256, the running meter's row r: the chain over its K new segments from the record's state, which becomes the state on entry to segment S0 + K; the
// running peak takes max |piece| (NaN once a NaN was seen); the (t + L) mod hop samples behind the last whole segment go to the OTHER tail buffer
__global__ __launch_bounds__(256) void wave_loud_push_chain_kernel(const float* __restrict__ wav, cbx_wave_rows_t rows, wl_n0_t n0, const float* __restrict__ tail_in,
                                                                   float* __restrict__ tail_out, wl_pow_t pw, int hop, double* __restrict__ ws, long ld,
                                                                   double* __restrict__ rec, long rec_ld) {
    __shared__ double sm[4 * WL_CHAIN];
    __shared__ float s_pk[256];
    __shared__ int s_nan[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long t = n0.v[r] % hop, L = rows.n[r], K = (t + L) / hop;
    const float* p = wav + rows.off[r];
    double* R0 = rec + (long)r * rec_ld;
    double cur[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid == 0)
        for (int q = 0; q < 4; ++q) cur[q] = R0[q];
    wl_chain(sm, ws + (long)r * ld * 4, K, pw, cur);
    if (tid == 0 && K > 0)
        for (int q = 0; q < 4; ++q) R0[q] = cur[q];
    float pk = 0.0f;
    int bad = 0;
    for (long i = tid; i < L; i += 256) {
        const float x = p[i];
        pk = fmaxf(pk, fabsf(x));
        bad |= !(x == x);
    }
    s_pk[tid] = pk, s_nan[tid] = bad;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_pk[tid] = fmaxf(s_pk[tid], s_pk[tid + s]), s_nan[tid] |= s_nan[tid + s];
        __syncthreads();
    }
    if (tid == 0 && L > 0) {
        const double old = R0[4];
        R0[4] = (s_nan[0] || !(old == old)) ? (double)NAN : fmax(old, (double)s_pk[0]);
    }
    const long rem = t + L - K * hop;  // (< hop)
    for (long j = tid; j < rem; j += 256) {
        const long i = K * hop + j;
        tail_out[(long)r * hop + j] = i < t ? tail_in[(long)r * hop + i] : p[i - t];
    }
}

// sum of v over the workgroup in a fixed order; every thread gets it
__device__ __forceinline__ double wl_block_sum(double* sm, int tid, double v) {
    __syncthreads();
    sm[tid] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) sm[tid] = sm[tid] + sm[tid + s];
        __syncthreads();
    }
    return sm[0];
}

// grid (R / C) x 256: blocks, gates, L, peak and gain of signal g = rows [g C, g C + C) of one length (C = 1: row g).  C = 2 (cbx_wave_loudness_ch_f32): the
// segment energy is e_s = E_(0,s) + E_(1,s), one fp64 add in channel order, and the peak is the larger channel's; C = 1 reads E_s itself.  PUSH (the running
// meter, C = 1): ws is the records, ld their stride, rows.n[r] the SEGMENTS of row r so far, and the peak is the record's
template <bool PUSH, int C>
__global__ __launch_bounds__(256) void wave_loud_row_kernel(cbx_wave_rows_t rows, int R, int hop, wl_target_t target, double ceiling, const double* __restrict__ ws, long ld,
                                                            double* __restrict__ stats, float* __restrict__ gain) {
    static_assert(!PUSH || C == 1, "the running meter is mono");
    __shared__ double sm[256];
    __shared__ int s_bad[256], s_nan[256];
    const int g = blockIdx.x, r = g * C, tid = threadIdx.x;
    const long n = rows.n[r];
    const long S = PUSH ? n : n / hop, nseg = PUSH ? n : (n + hop - 1) / hop;
    const double* E = PUSH ? ws + (long)r * ld + WL_REC : ws + (4l * R + r) * ld;
    const double* P = ws + (5l * R + r) * ld;  // (not read by PUSH)
    const auto es = [&](long s) { return C == 1 ? E[s] : E[s] + E[ld + s]; };  // (row r + 1's table follows row r's)
    double pk = 0.0;
    int pnan = 0;
    long bad = S;  // the first segment whose energy is not finite
    for (long s = tid; s < nseg; s += 256) {
        double v = PUSH ? 0.0 : P[s];
        pnan |= !(v == v);
        if (C == 2) {
            const double v1 = P[ld + s];
            pnan |= !(v1 == v1);
            v = fmax(v, v1);
        }
        pk = fmax(pk, v);
        if (s < S && !wl_finite(es(s))) bad = s < bad ? s : bad;
    }
    sm[tid] = pk, s_bad[tid] = (int)bad, s_nan[tid] = pnan;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            sm[tid] = fmax(sm[tid], sm[tid + s]);
            s_bad[tid] = s_bad[tid + s] < s_bad[tid] ? s_bad[tid + s] : s_bad[tid];
            s_nan[tid] |= s_nan[tid + s];
        }
        __syncthreads();
    }
    const double peak = PUSH ? ws[(long)r * ld + 4] : (s_nan[0] ? (double)NAN : sm[0]);
    bad = s_bad[0];
    const long nb = S >= 4 ? S - 3 : 0;
    const double den = 4.0 * (double)hop;
    // absolute gate
    double sum = 0.0, num = 0.0;
    for (long j = tid; j < nb; j += 256) {
        const double z = j + 3 >= bad ? (double)NAN : (es(j) + es(j + 1) + es(j + 2) + es(j + 3)) / den;
        const double l = -0.691 + 10.0 * log10(z);
        if (l >= -70.0) sum += z, num += 1.0;
    }
    sum = wl_block_sum(sm, tid, sum);
    num = wl_block_sum(sm, tid, num);
    double L = -INFINITY, used = 0.0;
    if (num > 0.0) {  // (uniform over the workgroup)
        const double gate = -0.691 + 10.0 * log10(sum / num) - 10.0;
        double sum2 = 0.0, num2 = 0.0;
        for (long j = tid; j < nb; j += 256) {
            const double z = j + 3 >= bad ? (double)NAN : (es(j) + es(j + 1) + es(j + 2) + es(j + 3)) / den;
            const double l = -0.691 + 10.0 * log10(z);
            if (l >= -70.0 && l > gate) sum2 += z, num2 += 1.0;
        }
        sum2 = wl_block_sum(sm, tid, sum2);
        num2 = wl_block_sum(sm, tid, num2);
        if (num2 > 0.0) L = -0.691 + 10.0 * log10(sum2 / num2), used = num2;
    }
    if (tid == 0) {
        const double t = target.t[g];
        double gn = 1.0;
        if (t == t) {
            gn = pow(10.0, (t - L) / 20.0);
            if (ceiling > 0.0 && peak * gn > ceiling) gn = ceiling / peak;
            if (!wl_finite(L) || !wl_finite(peak) || !wl_finite(gn)) gn = 1.0;
        }
        stats[4 * g] = L, stats[4 * g + 1] = peak, stats[4 * g + 2] = gn, stats[4 * g + 3] = used;
        gain[g] = (float)gn;
    }
}

// grid (ceil((max n + 3) / WL_TILE), R) x 256: workgroup (x, r) owns quads [1024 x, 1024 (x + 1)) of row r, counted from the 16-byte boundary at or below its start
__global__ __launch_bounds__(256) void wave_gain_kernel(float* __restrict__ wav, cbx_wave_rows_t rows, const float* __restrict__ gain) {
    const int r = blockIdx.y;
    const long n = rows.n[r];
    float* p = wav + rows.off[r];
    const float g = gain[r];
    const long mis = (long)(((uintptr_t)p >> 2) & 3);
    for (int it = 0; it < 4; ++it) {
        const long i0 = 4 * ((long)blockIdx.x * (WL_TILE / 4) + it * 256 + threadIdx.x) - mis;  // (-3 .. -1 in the first quad of a misaligned row)
        if (i0 >= n) return;
        if (i0 >= 0 && i0 + 4 <= n) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + i0);
            *reinterpret_cast<f32x4*>(p + i0) = f32x4{t[0] * g, t[1] * g, t[2] * g, t[3] * g};
        } else {
            for (int e = 0; e < 4; ++e)
                if (i0 + e >= 0 && i0 + e < n) p[i0 + e] = p[i0 + e] * g;
        }
    }
}

// o = a b, 4 x 4 row-major (o is neither a nor b)
void wl_matmul(const double* a, const double* b, double* o) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[4 * i + j] = a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j] + a[4 * i + 3] * b[12 + j];
}

// o = a^e by squaring, e >= 0
void wl_matpow(const double* a, long e, double* o) {
    double base[16], t[16];
    for (int i = 0; i < 16; ++i) base[i] = a[i], o[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (; e > 0; e >>= 1) {
        if (e & 1) {
            wl_matmul(o, base, t);
            for (int i = 0; i < 16; ++i) o[i] = t[i];
        }
        wl_matmul(base, base, t);
        for (int i = 0; i < 16; ++i) base[i] = t[i];
    }
}

// the caller's coefficients, all finite -> *k
int wl_coefs(const char* who, const double* coef, wl_coef_t* k) {
    for (int i = 0; i < 10; ++i) {
        CBX_REQUIRE(fabs(coef[i]) < INFINITY, "%s: coefficient %d is not finite", who, i);
        k->c[i] = coef[i];
    }
    return 0;
}

// the powers of the cascade's transition matrix the kernels take by value
void wl_powers(const wl_coef_t& k, int hop, wl_pow_t* pw) {
    double A[16];
    for (int j = 0; j < 4; ++j) {  // column j of A: one step of the cascade on unit vector j with a zero sample
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        st[j] = 1.0;
        wl_step(k, st, 0.0);
        for (int q = 0; q < 4; ++q) A[4 * q + j] = st[q];
    }
    wl_matpow(A, (hop + 63) / 64, pw->m[0]);
    for (int i = 1; i < 6; ++i) wl_matmul(pw->m[i - 1], pw->m[i - 1], pw->m[i]);
    wl_matpow(A, hop, pw->m[6]);
}

}  // namespace

// The meter behind cbx_wave_loudness_f32 (C = 1, who = "wave_loudness") and cbx_wave_loudness_ch_f32 (wave_stereo.hip, which has checked C and the groups'
// lengths): the per-row phases over all R rows, then the row step once per signal of C rows.  target, stats, gain: R / C entries.
int cbx_wave_loudness_run(const char* who, const float* wav, const long* row_off, const int* row_len, int R, int C, const double* coef, int hop, const double* target,
                          double ceiling, double* stats, float* gain, double* ws, long ws_cap, void* stream) {
    cbx_wave_rows_t rows;
    cbx_wave_span_t sp;
    const int rc = cbx_wave_rows(who, row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && coef && target && stats && gain && ws, "%s: null pointer", who);
    CBX_REQUIRE(hop >= 1, "%s: hop = %d (a tenth of a second in samples, at least 1)", who, hop);
    wl_coef_t k;
    if (const int e = wl_coefs(who, coef, &k)) return e;
    const long nseg = (sp.n_max + hop - 1) / hop;
    CBX_REQUIRE(ws_cap >= 6l * R * nseg, "%s: workspace of %ld doubles, %d rows of %ld segments need %ld", who, ws_cap, R, nseg, 6l * R * nseg);
    wl_target_t tg;
    for (int r = 0; r < CBX_WAVE_MAX_ROWS; ++r) tg.t[r] = r < R / C ? target[r] : (double)NAN;
    if (nseg > 0) {
        const long gx = (nseg + 3) / 4;
        CBX_REQUIRE(gx <= 0x7fffffffl, "%s: a row of %ld samples is too long for one launch", who, sp.n_max);
        wl_pow_t pw;
        wl_powers(k, hop, &pw);
        hipLaunchKernelGGL(wave_loud_seg_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, R, k, pw, hop, 0, ws, nseg);
        int e = cbx_check_launch(who);
        if (e) return e;
        hipLaunchKernelGGL(wave_loud_chain_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, rows, pw, hop, ws, nseg);
        if ((e = cbx_check_launch(who))) return e;
        hipLaunchKernelGGL(wave_loud_seg_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, R, k, pw, hop, 1, ws, nseg);
        if ((e = cbx_check_launch(who))) return e;
    }
    const auto row_kernel = C == 2 ? wave_loud_row_kernel<false, 2> : wave_loud_row_kernel<false, 1>;
    hipLaunchKernelGGL(row_kernel, dim3((unsigned)(R / C)), dim3(256), 0, (hipStream_t)stream, rows, R, hop, tg, ceiling, (const double*)ws, nseg, stats, gain);
    return cbx_check_launch(who);
}

extern "C" int cbx_wave_loudness_f32(const float* wav, const long* row_off, const int* row_len, int R, const double* coef, int hop, const double* target,
                                     double ceiling, double* stats, float* gain, double* ws, long ws_cap, void* stream) {
    return cbx_wave_loudness_run("wave_loudness", wav, row_off, row_len, R, 1, coef, hop, target, ceiling, stats, gain, ws, ws_cap, stream);
}

extern "C" int cbx_wave_loudness_push_f32(const float* wav, const long* row_off, const int* row_len, const long* n0, int R, const double* coef, int hop,
                                          const double* target, double ceiling, double* rec, long seg_cap, const float* tail_in, float* tail_out, double* stats,
                                          float* gain, double* ws, long ws_cap, void* stream) {
    cbx_wave_rows_t rows;
    cbx_wave_span_t sp;
    const int rc = cbx_wave_rows("wave_loudness_push", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && n0 && coef && target && rec && tail_in && tail_out && stats && gain && ws, "wave_loudness_push: null pointer");
    CBX_REQUIRE(tail_in != tail_out, "wave_loudness_push: tail_out is tail_in (the two tail buffers alternate)");
    CBX_REQUIRE(hop >= 1, "wave_loudness_push: hop = %d (a tenth of a second in samples, at least 1)", hop);
    wl_coef_t k;
    if (const int e = wl_coefs("wave_loudness_push", coef, &k)) return e;
    wl_n0_t at;
    cbx_wave_rows_t segs = rows;  // n[r]: the segments of row r after this push
    long k_max = 0;
    for (int r = 0; r < CBX_WAVE_MAX_ROWS; ++r) at.v[r] = 0;
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(n0[r] >= 0, "wave_loudness_push: row %d has consumed %ld samples", r, n0[r]);
        const long K = (n0[r] % hop + row_len[r]) / hop, S1 = n0[r] / hop + K;
        CBX_REQUIRE(S1 <= seg_cap && S1 <= 0x7fffffffl, "wave_loudness_push: row %d reaches %ld segments, the record holds %ld", r, S1, seg_cap);
        at.v[r] = n0[r], segs.n[r] = (int)S1;
        k_max = K > k_max ? K : k_max;
    }
    CBX_REQUIRE(ws_cap >= 4l * R * k_max, "wave_loudness_push: workspace of %ld doubles, %d rows of %ld new segments need %ld", ws_cap, R, k_max, 4l * R * k_max);
    wl_target_t tg;
    for (int r = 0; r < CBX_WAVE_MAX_ROWS; ++r) tg.t[r] = r < R ? target[r] : (double)NAN;
    const long rec_ld = WL_REC + seg_cap, gx = (k_max + 3) / 4;
    wl_pow_t pw = {};
    int e;
    if (k_max > 0) {
        wl_powers(k, hop, &pw);
        hipLaunchKernelGGL(wave_loud_push_seg_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, at, tail_in, k, pw, hop, 0, ws, k_max,
                           rec, rec_ld);
        if ((e = cbx_check_launch("wave_loudness_push"))) return e;
    }
    hipLaunchKernelGGL(wave_loud_push_chain_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, at, tail_in, tail_out, pw, hop, ws, k_max, rec, rec_ld);
    if ((e = cbx_check_launch("wave_loudness_push"))) return e;
    if (k_max > 0) {
        hipLaunchKernelGGL(wave_loud_push_seg_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, at, tail_in, k, pw, hop, 1, ws, k_max,
                           rec, rec_ld);
        if ((e = cbx_check_launch("wave_loudness_push"))) return e;
    }
    hipLaunchKernelGGL((wave_loud_row_kernel<true, 1>), dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, segs, R, hop, tg, ceiling, (const double*)rec, rec_ld, stats, gain);
    return cbx_check_launch("wave_loudness_push");
}

extern "C" int cbx_wave_gain_f32(float* wav, const long* row_off, const int* row_len, int R, const float* gain, void* stream) {
    cbx_wave_rows_t rows;
    cbx_wave_span_t sp;
    const int rc = cbx_wave_rows("wave_gain", row_off, row_len, R, &rows, &sp);
    if (rc) return rc;
    CBX_REQUIRE(wav && gain, "wave_gain: null pointer");
    if (sp.n_max == 0) return 0;
    const long gx = (sp.n_max + 3 + WL_TILE - 1) / WL_TILE;  // (+ 3: a row may begin up to three samples into its first quad)
    hipLaunchKernelGGL(wave_gain_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, gain);
    return cbx_check_launch("wave_gain");
}
