// What the delivery kernels (wave_*.hip) share: the by-value descriptor of "up to 64 rows of one allocation" with its host checks, the block-energy pass of the
// two trims and the pause control, and the two tree reductions of the edges kernels.  An entry's own per-row fields live in a struct of its own that derives
// from the core descriptor; every kernel's argument block stays under 4 KiB (the pitch step's, the largest, is 3 KiB).
//
// How to include it: cbx_common.h first, then "../../chatterbox_amd/csrc/wave_common.h".  These sources are also compiled as copies elsewhere (tests/simt, the
// emulator, whose builder rewrites every header of this directory and puts it beside the copies, the include line turned into the sibling's name).  A builder that
// knows only cbx_common.h still reaches this file by that path through its include directory two levels below the root; it takes this file as it is, and must not
// be led from here to a second, unrewritten cbx_common.h -- so this header includes nothing.
#pragma once

constexpr int CBX_WAVE_MAX_ROWS = 64;

// rows `wav + off[r]` of n[r] elements each; entries behind R are zero
struct cbx_wave_rows_t {
    long off[CBX_WAVE_MAX_ROWS];
    int n[CBX_WAVE_MAX_ROWS];
};

// what a set of rows adds up to: the longest, the sum, and the span [lo, hi) of the non-empty ones (lo = -1: every row is empty)
struct cbx_wave_span_t {
    long n_max, n_sum, lo, hi;
};

static inline void cbx_wave_span_add(cbx_wave_span_t* sp, long off, long n) {
    sp->n_max = n > sp->n_max ? n : sp->n_max;
    sp->n_sum += n;
    if (n > 0) {
        sp->lo = sp->lo < 0 || off < sp->lo ? off : sp->lo;
        sp->hi = off + n > sp->hi ? off + n : sp->hi;
    }
}

// the first two checks of cbx_wave_rows alone, for an entry whose own checks stand between them and the rows'
static inline int cbx_wave_count(const char* who, const long* row_off, const int* row_len, int R) {
    CBX_REQUIRE(row_off && row_len, "%s: null pointer", who);
    CBX_REQUIRE(R >= 1 && R <= CBX_WAVE_MAX_ROWS, "%s: R = %d outside [1, %d]", who, R, CBX_WAVE_MAX_ROWS);
    return 0;
}

// the host arrays of a call -> the by-value descriptor and its span; every refusal carries the entry's name
static inline int cbx_wave_rows(const char* who, const long* row_off, const int* row_len, int R, cbx_wave_rows_t* rows, cbx_wave_span_t* sp) {
    if (const int rc = cbx_wave_count(who, row_off, row_len, R)) return rc;
    *rows = cbx_wave_rows_t{};
    *sp = cbx_wave_span_t{0, 0, -1, 0};
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(row_len[r] >= 0 && row_off[r] >= 0, "%s: row %d has length %d at offset %ld", who, r, row_len[r], row_off[r]);
        rows->off[r] = row_off[r], rows->n[r] = row_len[r];
        cbx_wave_span_add(sp, row_off[r], row_len[r]);
    }
    return 0;
}

// the packed outputs of a call: row r writes out[out_off[r], out_off[r] + cnt[r]) of out_cap elements, and the rows together (`unit`: what the entry calls an
// element; NULL: rows of another layout, no sum) fit; their span -> *sp
static inline int cbx_wave_packed(const char* who, const long* out_off, const long* cnt, int R, long out_cap, const char* unit, cbx_wave_span_t* sp) {
    *sp = cbx_wave_span_t{0, 0, -1, 0};
    for (int r = 0; r < R; ++r) {
        CBX_REQUIRE(cnt[r] >= 0 && out_off[r] >= 0 && out_off[r] + cnt[r] <= out_cap, "%s: row %d writes [%ld, %ld) of an output of %ld", who, r, out_off[r],
                    out_off[r] + cnt[r], out_cap);
        cbx_wave_span_add(sp, out_off[r], cnt[r]);
    }
    CBX_REQUIRE(!unit || sp->n_sum <= out_cap, "%s: out holds %ld %s, the rows produce %ld", who, out_cap, unit, sp->n_sum);
    return 0;
}

// an entry that does not run in place: the rows' span of wav and the outputs' span of out share no byte (`why`: the entry's reason, part of the message)
static inline int cbx_wave_apart(const char* who, const float* wav, const cbx_wave_span_t& in, const float* out, const cbx_wave_span_t& to, const char* why) {
    if (in.lo < 0 || to.lo < 0) return 0;
    const uintptr_t a0 = (uintptr_t)(wav + in.lo), a1 = (uintptr_t)(wav + in.hi), b0 = (uintptr_t)(out + to.lo), b1 = (uintptr_t)(out + to.hi);
    CBX_REQUIRE(a1 <= b0 || b1 <= a0, "%s: out overlaps wav (%s)", who, why);
    return 0;
}

// The mixer, the meter and the limiter behind their entries, with the plane count P in {1, 2} of the output or the channel count C in {1, 2} of a signal as an
// argument (wave_mix.hip, wave_loudness.hip, wave_limit.hip): the mono entries are the P = 1 / C = 1 calls; the entries of wave_stereo.hip are the P = 2 call and,
// for the linked pair, check C and the groups' lengths and call the same code -- one source, one arithmetic.  `who`: the entry's name in every refusal.
int cbx_wave_mix_run(const char* who, int P, const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, const float* pan, int R,
                     const float* gain, int G, const int* gain_idx, const float* ramp, int fade, float* out, long plane_stride, long out_len, int accumulate,
                     void* stream);
int cbx_wave_loudness_run(const char* who, const float* wav, const long* row_off, const int* row_len, int R, int C, const double* coef, int hop, const double* target,
                          double ceiling, double* stats, float* gain, double* ws, long ws_cap, void* stream);
int cbx_wave_limit_run(const char* who, const float* wav, const long* row_off, const int* row_len, int R, int C, const float* gain, const double* ceiling,
                       const float* tab, int U, int T, const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap,
                       void* stream);

// the rows of a linked entry: C in {1, 2} and R a multiple of it, the C rows of every signal of one length
static inline int cbx_wave_groups(const char* who, const long* row_off, const int* row_len, int R, int C) {
    if (const int rc = cbx_wave_count(who, row_off, row_len, R)) return rc;
    CBX_REQUIRE(C == 1 || C == 2, "%s: C = %d channels outside {1, 2}", who, C);
    CBX_REQUIRE(R % C == 0, "%s: %d rows are no whole number of signals of %d channels", who, R, C);
    for (int r = 0; r < R; r += C)
        for (int c = 1; c < C; ++c)
            CBX_REQUIRE(row_len[r + c] == row_len[r], "%s: rows %d and %d, channels of one signal, have the lengths %d and %d", who, r, r + c, row_len[r], row_len[r + c]);
    return 0;
}

// Block b of row r covers [BLOCK b, min(BLOCK (b + 1), n)); ws[r ws_ld + b] = the fp64 sum of its squares, divided by its count where MEAN.  One WAVE per block:
// lane l squares and adds elements [4 l, 4 l + 4) and [256 + 4 l, 256 + 4 l + 4) in that order (16-byte loads where the row allows them, the same order where it
// does not), then a 6-step xor butterfly -- a fixed order per block whatever the grid or the row's alignment, no floating-point atomics.
// grid (ceil(max blocks / 4), R) x 256: wave w of workgroup (x, r) owns block 4 x + w of row r
template <int BLOCK, bool MEAN>
__global__ __launch_bounds__(256) void wave_block_ms_kernel(const float* __restrict__ wav, cbx_wave_rows_t rows, double* __restrict__ ws, long ws_ld) {
    const int r = blockIdx.y, lane = threadIdx.x & 63;
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int n = rows.n[r];
    const long s0 = (long)b * BLOCK;
    if (s0 >= n) return;  // (wave-uniform)
    const int cnt = n - s0 < BLOCK ? (int)(n - s0) : BLOCK;
    const float* p = wav + rows.off[r] + s0;
    const bool aligned = ((uintptr_t)p & 15) == 0;
    double acc = 0.0;
    for (int q = lane; q < BLOCK / 4; q += 64) {
        const int e = 4 * q;
        if (e >= cnt) break;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // (elements beyond the row add an exact zero)
        if (aligned && e + 4 <= cnt) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + e);
            v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
        } else {
            for (int k = 0; k < 4; ++k)
                if (e + k < cnt) v[k] = p[e + k];
        }
        for (int k = 0; k < 4; ++k) acc += (double)v[k] * (double)v[k];
    }
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) ws[(long)r * ws_ld + b] = MEAN ? acc / (double)cnt : acc;
}

// the block pass of a call over nb = ceil(n_max / BLOCK) > 0 blocks per row -> ws[r * nb + b]
template <int BLOCK, bool MEAN>
static inline int cbx_wave_block_pass(const char* who, const float* wav, const cbx_wave_rows_t& rows, int R, long n_max, long nb, double* ws, void* stream) {
    const long gx = (nb + 3) / 4;
    CBX_REQUIRE(gx <= 0x7fffffffl, "%s: a row of %ld samples is too long for one launch", who, n_max);
    const auto kernel = wave_block_ms_kernel<BLOCK, MEAN>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, (hipStream_t)stream, wav, rows, ws, nb);
    return cbx_check_launch(who);
}

// The two reductions of an edges kernel over the nf frames of a row, by all 256 threads of its workgroup: peak = max_f value(f) (fmax from 0: a NaN frame is
// ignored), then the first and the last frame with pass(value(f), peak * ratio) -> *lo, *hi (*hi < 0: none).  Strided accumulate, then the 128 .. 1 LDS tree.
template <class VALUE, class PASS>
__device__ __forceinline__ void cbx_wave_peak_edges(int nf, double ratio, VALUE value, PASS pass, int* lo_out, int* hi_out) {
    __shared__ double s_pk[256];
    __shared__ int s_lo[256], s_hi[256];
    const int tid = threadIdx.x;
    double pk = 0.0;
    for (int f = tid; f < nf; f += 256) pk = fmax(pk, value(f));
    s_pk[tid] = pk;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_pk[tid] = fmax(s_pk[tid], s_pk[tid + s]);
        __syncthreads();
    }
    const double thr = s_pk[0] * ratio;
    int lo = 0x7fffffff, hi = -1;
    for (int f = tid; f < nf; f += 256) {
        if (pass(value(f), thr)) {
            lo = f < lo ? f : lo;
            hi = f > hi ? f : hi;
        }
    }
    s_lo[tid] = lo, s_hi[tid] = hi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            s_lo[tid] = s_lo[tid + s] < s_lo[tid] ? s_lo[tid + s] : s_lo[tid];
            s_hi[tid] = s_hi[tid + s] > s_hi[tid] ? s_hi[tid + s] : s_hi[tid];
        }
        __syncthreads();
    }
    *lo_out = s_lo[0], *hi_out = s_hi[0];
}
