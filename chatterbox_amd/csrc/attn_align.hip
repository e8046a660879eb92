// Word timestamps (cbx_attn_text_mass_f32, cbx_align_path_f32; include/cbx.h): the attention mass that selected heads of a decoder layer put on the TEXT columns
// while each speech token was sampled, and the monotonic path through that mass.  The reference's later alignment analyser reads the same heads through forward
// hooks that materialise whole attention rows on the host; here the rows never exist: the normaliser of a causal row is an online maximum and sum, and only the
// text columns are evaluated a second time and stored.  Plain C++: no inline assembly, no atomics, every output element written by one thread per launch in a
// fixed summation order, so the emulator build and the GPU run the same arithmetic (up to the library's expf).
//
// Mass: one wave per (row, 4 consecutive queries), all selected heads in list order.  A lane holds ONE key row (64 floats) in registers, read straight from the
// cache with 16-byte loads, and reads the queries as LDS broadcasts: 16 LDS reads per 64 fmas.  Pass 1, per head: keys in tiles of 64, each lane keeps a running
// maximum and sum for each of the 4 queries over the keys j = lane (mod 64) it has seen; the 64 partial (m, l) of a query are joined by the xor butterfly 32 .. 1.
// Pass 2, per tile of 64 text columns: for every head in list order p = expf(s - M) / L is added up in a register, then one store per (query, column).  The work
// is small (2 GFLOP per layer at 8 x 250 queries x 1400 keys x 3 heads): the simple exact form was preferred to staging K tiles for several waves.
//
// Path: one workgroup per row, thread t owns text column t, the previous row of D double-buffered in LDS (one barrier per frame), the move bits of a frame leave
// as one ballot word per wave; then thread 0 walks back through the move words, which the workgroup stages in LDS 64 frames at a time.
#include <math.h>

#include "cbx_common.h"

namespace {

constexpr int TM_ROWS = 64;     // rows of a launch (per-row numbers travel by value)
constexpr int TM_QW = 4;        // queries of a wave
constexpr int TM_KT = 64;       // keys / text columns of a tile: one per lane
constexpr int TM_SEL = 16;      // selected heads
constexpr int TM_CTX = 4608;    // the RoPE table
constexpr int TM_TEXT = 1024;   // text columns

struct tm_rows_t {
    int q_len[TM_ROWS], q0[TM_ROWS], ctx0[TM_ROWS], t0[TM_ROWS], t_len[TM_ROWS];
    int heads[TM_SEL];
};

// the key row of this lane: 64 floats at a 16-byte boundary
__device__ __forceinline__ void tm_load_key(const float* __restrict__ p, f32x4 (&kr)[16]) {
#pragma unroll
    for (int c = 0; c < 16; ++c) kr[c] = *reinterpret_cast<const f32x4*>(p + 4 * c);
}

// q . k in the fixed order d = 0 .. 63, one fma per term from 0
__device__ __forceinline__ float tm_dot(const float* sq, const f32x4 (&kr)[16]) {
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const f32x4 qv = *reinterpret_cast<const f32x4*>(sq + 4 * c);
        acc = __builtin_fmaf(qv[0], kr[c][0], acc);
        acc = __builtin_fmaf(qv[1], kr[c][1], acc);
        acc = __builtin_fmaf(qv[2], kr[c][2], acc);
        acc = __builtin_fmaf(qv[3], kr[c][3], acc);
    }
    return acc;
}

// grid (ceil(max q_len / 4), nz) x 64
__global__ __launch_bounds__(64) void attn_text_mass_kernel(const float* __restrict__ q, const float* __restrict__ k, float* __restrict__ mass, tm_rows_t rows,
                                                            int n_sel, long q_sb, long q_st, long k_sb, long k_st, long k_sh, long m_sb, long m_si, float scale,
                                                            float weight, int accumulate) {
    __shared__ __attribute__((aligned(16))) float s_q[TM_SEL][TM_QW][64];
    __shared__ float s_m[TM_SEL][TM_QW], s_l[TM_SEL][TM_QW];
    const int z = blockIdx.y, lane = threadIdx.x;
    const int ql = rows.q_len[z], i0 = blockIdx.x * TM_QW;
    if (i0 >= ql) return;  // (uniform over the workgroup, ahead of its barriers)
    const int nq = ql - i0 < TM_QW ? ql - i0 : TM_QW;
    const int c0 = rows.ctx0[z], t0 = rows.t0[z], tl = rows.t_len[z];
    const int jmax = c0 + i0 + nq - 1;  // the last key any query of this wave sees: nothing beyond it is loaded
    // the queries of every selected head: lane -> (query lane / 16, floats 4 (lane % 16) ..); queries past q_len are zeros and never stored
    for (int s = 0; s < n_sel; ++s) {
        const int qq = lane >> 4, d4 = (lane & 15) * 4;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (qq < nq) v = *reinterpret_cast<const f32x4*>(q + (long)z * q_sb + (long)(rows.q0[z] + i0 + qq) * q_st + (long)rows.heads[s] * 64 + d4);
        *reinterpret_cast<f32x4*>(&s_q[s][qq][d4]) = v;
    }
    __syncthreads();
    f32x4 kr[16];
    // ---- pass 1: the normaliser of every (head, query) over the whole causal row
    for (int s = 0; s < n_sel; ++s) {
        const float* kh = k + (long)z * k_sb + (long)rows.heads[s] * k_sh;
        float m[TM_QW], l[TM_QW];
#pragma unroll
        for (int qq = 0; qq < TM_QW; ++qq) m[qq] = -INFINITY, l[qq] = 0.0f;
        for (int jb = 0; jb <= jmax; jb += TM_KT) {
            const int j = jb + lane;
            if (j <= jmax) {
                tm_load_key(kh + (long)j * k_st, kr);
#pragma unroll
                for (int qq = 0; qq < TM_QW; ++qq) {
                    const float sc = scale * tm_dot(s_q[s][qq], kr);
                    if (qq < nq && j <= c0 + i0 + qq) {  // a key this query does not see changes nothing, whatever the cache holds there
                        if (sc > m[qq]) {
                            l[qq] = l[qq] * expf(m[qq] - sc) + 1.0f;  // (m = -inf: l = 0 * 0 + 1)
                            m[qq] = sc;
                        } else {
                            l[qq] += expf(sc - m[qq]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int qq = 0; qq < TM_QW; ++qq) {
            float M = m[qq];
            for (int x = 32; x >= 1; x >>= 1) M = fmaxf(M, __shfl_xor(M, x));
            // key 0 is visible to every query, so M is finite (for finite scores); a lane that saw no key has l = 0 and m = -inf: 0 * expf(-inf) = 0
            float L = qq < nq ? l[qq] * expf(m[qq] - M) : 0.0f;
            for (int x = 32; x >= 1; x >>= 1) L += __shfl_xor(L, x);
            if (lane == 0) s_m[s][qq] = M, s_l[s][qq] = L;
        }
    }
    __syncthreads();
    // ---- pass 2: the text columns, heads added in list order
    for (int tb = 0; tb < tl; tb += TM_KT) {
        const int t = tb + lane;
        if (t >= tl) continue;  // (no barrier below)
        const int j = t0 + t;   // t0 + t_len <= ctx0 + 1: every query sees every text column
        float acc[TM_QW];
#pragma unroll
        for (int qq = 0; qq < TM_QW; ++qq) acc[qq] = 0.0f;
        for (int s = 0; s < n_sel; ++s) {
            tm_load_key(k + (long)z * k_sb + (long)rows.heads[s] * k_sh + (long)j * k_st, kr);
#pragma unroll
            for (int qq = 0; qq < TM_QW; ++qq) {
                const float sc = scale * tm_dot(s_q[s][qq], kr);
                if (qq < nq) acc[qq] += expf(sc - s_m[s][qq]) / s_l[s][qq];
            }
        }
#pragma unroll
        for (int qq = 0; qq < TM_QW; ++qq) {
            if (qq < nq) {
                float* o = mass + (long)z * m_sb + (long)(i0 + qq) * m_si + t;
                *o = (accumulate ? *o : 0.0f) + weight * acc[qq];
            }
        }
    }
}

constexpr int AP_ROWS = 64;     // rows of a launch
constexpr int AP_N = 4096;      // frames
constexpr int AP_M = 1024;      // text tokens: one thread each
constexpr int AP_CHUNK = 64;    // frames of move words staged for the walk back

struct ap_rows_t {
    int n[AP_ROWS], m[AP_ROWS];
};

// grid (nz) x 64 W, W = ceil(max m / 64) waves; row z's move words at ws + z * n_max * W: word [i][w] = the ballot of wave w in frame i
__global__ __launch_bounds__(AP_M) void align_path_kernel(const float* __restrict__ score, long s_sb, long s_si, ap_rows_t rows, int n_max, int W,
                                                          unsigned long long* __restrict__ ws, int* __restrict__ spans, long sp_sb, int* __restrict__ frame_tok,
                                                          long ft_sb) {
    __shared__ float s_d[2][AP_M + 1];  // s_d[b][1 + t] = D[i][t]; s_d[b][0] = -inf: the column left of token 0
    __shared__ unsigned long long s_mv[AP_CHUNK * (AP_M / 64)];
    __shared__ int s_e;
    const int z = blockIdx.x, t = threadIdx.x;
    const int n = rows.n[z], m = rows.m[z];
    const float* sc = score + (long)z * s_sb;
    unsigned long long* mv = ws + (long)z * n_max * W;
    if (t == 0) s_d[0][0] = s_d[1][0] = -INFINITY;
    if (t < m) s_d[0][1 + t] = t == 0 ? sc[0] : -INFINITY;
    __syncthreads();
    for (int i = 1; i < n; ++i) {
        const float* prev = s_d[(i - 1) & 1];
        bool adv = false;
        if (t < m) {
            const float stay = prev[1 + t], diag = prev[t];
            adv = diag > stay;  // a tie stays
            s_d[i & 1][1 + t] = sc[(long)i * s_si + t] + (adv ? diag : stay);
        }
        const unsigned long long word = __ballot(adv);
        if ((t & 63) == 0) mv[(long)i * W + (t >> 6)] = word;
        __syncthreads();
    }
    const float* last = s_d[(n - 1) & 1];
    if (t == 0) {
        int e = m - 1;
        if (n < m) {  // the lowest t <= n - 1 with the largest D[n - 1][t]
            e = 0;
            for (int c = 1; c < n; ++c) e = last[1 + c] > last[1 + e] ? c : e;
        }
        s_e = e;
    }
    __syncthreads();  // (also: every move word of this workgroup is visible to it)
    const int e = s_e;
    int* sp = spans + (long)z * sp_sb;
    int* ft = frame_tok + (long)z * ft_sb;
    if (t > e && t < m) sp[2 * t] = n, sp[2 * t + 1] = n;  // never reached
    // the walk back from (n - 1, e), the move words of frames [hi - 64, hi) staged at a time; frame 0 has no move: the path is at token 0 there
    int tok = e;
    for (int hi = n; hi > 0; hi -= AP_CHUNK) {
        const int lo = hi > AP_CHUNK ? hi - AP_CHUNK : 0;
        for (int x = t; x < (hi - lo) * W; x += blockDim.x) s_mv[x] = lo + x / W >= 1 ? mv[(long)lo * W + x] : 0ull;
        __syncthreads();
        if (t == 0) {
            for (int i = hi - 1; i >= lo; --i) {
                ft[i] = tok;
                if (i == n - 1) sp[2 * tok + 1] = n;
                const int step = (int)((s_mv[(i - lo) * W + (tok >> 6)] >> (tok & 63)) & 1ull);
                if (step) sp[2 * tok] = i, sp[2 * (tok - 1) + 1] = i;
                tok -= step;
            }
        }
        __syncthreads();
    }
    if (t == 0) sp[0] = 0;  // the path starts at token 0
}

}  // namespace

extern "C" int cbx_attn_text_mass_f32(const float* q, const float* k, float* mass, const int* heads, int n_sel, int n_heads, const int* q0, const int* q_len,
                                      const int* ctx0, const int* t0, const int* t_len, int nz, long q_sb, long q_st, long k_sb, long k_st, long k_sh, long m_sb, long m_si,
                                      float scale, float weight, int accumulate, void* stream) {
    CBX_REQUIRE(q && k && mass && heads && q_len && ctx0 && t0 && t_len, "attn_text_mass: null pointer");
    CBX_REQUIRE(nz >= 1 && nz <= TM_ROWS, "attn_text_mass: nz = %d outside [1, %d]", nz, TM_ROWS);
    CBX_REQUIRE(n_sel >= 1 && n_sel <= TM_SEL, "attn_text_mass: n_sel = %d outside [1, %d]", n_sel, TM_SEL);
    CBX_REQUIRE(n_heads >= 1, "attn_text_mass: n_heads = %d", n_heads);
    CBX_REQUIRE((((uintptr_t)q | (uintptr_t)k) & 15) == 0 && q_sb % 4 == 0 && q_st % 4 == 0 && k_sb % 4 == 0 && k_st % 4 == 0 && k_sh % 4 == 0,
                "attn_text_mass: q and k are read with 16-byte loads (pointers on 16-byte boundaries, strides multiples of 4 floats)");
    CBX_REQUIRE(q_sb >= 0 && q_st >= 0 && k_sb >= 0 && k_st >= 0 && k_sh >= 0 && m_sb >= 0 && m_si >= 0, "attn_text_mass: a negative stride");
    tm_rows_t rows;
    for (int z = 0; z < TM_ROWS; ++z) rows.q_len[z] = rows.q0[z] = rows.ctx0[z] = rows.t0[z] = rows.t_len[z] = 0;
    for (int s = 0; s < TM_SEL; ++s) rows.heads[s] = 0;
    for (int s = 0; s < n_sel; ++s) {
        CBX_REQUIRE(heads[s] >= 0 && heads[s] < n_heads, "attn_text_mass: heads[%d] = %d outside [0, %d)", s, heads[s], n_heads);
        rows.heads[s] = heads[s];
    }
    int q_max = 0;
    for (int z = 0; z < nz; ++z) {
        CBX_REQUIRE(q_len[z] >= 0 && ctx0[z] >= 0 && (long)ctx0[z] + q_len[z] <= TM_CTX, "attn_text_mass: row %d has %d queries behind %d keys (a context of at most %d)",
                    z, q_len[z], ctx0[z], TM_CTX);
        CBX_REQUIRE(t0[z] >= 0 && t_len[z] >= 0 && t_len[z] <= TM_TEXT, "attn_text_mass: row %d has text columns [%d, %d + %d) (at most %d)", z, t0[z], t0[z], t_len[z],
                    TM_TEXT);
        CBX_REQUIRE((long)t0[z] + t_len[z] <= (long)ctx0[z] + 1, "attn_text_mass: row %d: text columns [%d, %d) are not visible to its first query (ctx0 = %d)", z, t0[z],
                    t0[z] + t_len[z], ctx0[z]);
        CBX_REQUIRE(m_si >= t_len[z] && (nz == 1 || m_sb >= (long)q_len[z] * m_si), "attn_text_mass: row %d (%d x %d) does not fit the strides of mass (%ld, %ld)", z,
                    q_len[z], t_len[z], m_sb, m_si);
        CBX_REQUIRE(!q0 || q0[z] >= 0, "attn_text_mass: row %d begins at query %d", z, q0[z]);
        rows.q0[z] = q0 ? q0[z] : 0;
        rows.q_len[z] = q_len[z], rows.ctx0[z] = ctx0[z], rows.t0[z] = t0[z], rows.t_len[z] = t_len[z];
        q_max = q_len[z] > q_max && t_len[z] > 0 ? q_len[z] : q_max;
    }
    if (q_max == 0) return 0;
    hipLaunchKernelGGL(attn_text_mass_kernel, dim3((unsigned)((q_max + TM_QW - 1) / TM_QW), (unsigned)nz), dim3(64), 0, (hipStream_t)stream, q, k, mass, rows, n_sel,
                       q_sb, q_st, k_sb, k_st, k_sh, m_sb, m_si, scale, weight, accumulate);
    return cbx_check_launch("attn_text_mass");
}

extern "C" int cbx_align_path_f32(const float* score, long s_sb, long s_si, const int* n, const int* m, int nz, int* spans, long sp_sb, int* frame_tok, long ft_sb,
                                  void* ws, long ws_cap, void* stream) {
    CBX_REQUIRE(score && n && m && spans && frame_tok && ws, "align_path: null pointer");
    CBX_REQUIRE(nz >= 1 && nz <= AP_ROWS, "align_path: nz = %d outside [1, %d]", nz, AP_ROWS);
    CBX_REQUIRE(((uintptr_t)ws & 7) == 0, "align_path: the workspace holds 8-byte words");
    ap_rows_t rows;
    for (int z = 0; z < AP_ROWS; ++z) rows.n[z] = rows.m[z] = 1;
    int n_max = 0, m_max = 0;
    for (int z = 0; z < nz; ++z) {
        CBX_REQUIRE(n[z] >= 1 && n[z] <= AP_N && m[z] >= 1 && m[z] <= AP_M, "align_path: row %d has %d frames (1 .. %d) and %d text tokens (1 .. %d)", z, n[z], AP_N, m[z],
                    AP_M);
        CBX_REQUIRE(s_si >= m[z] && (nz == 1 || (s_sb >= (long)n[z] * s_si && sp_sb >= 2L * m[z] && ft_sb >= n[z])),
                    "align_path: row %d (%d x %d) does not fit the strides (score %ld, %ld; spans %ld; frame_tok %ld)", z, n[z], m[z], s_sb, s_si, sp_sb, ft_sb);
        rows.n[z] = n[z], rows.m[z] = m[z];
        n_max = n[z] > n_max ? n[z] : n_max, m_max = m[z] > m_max ? m[z] : m_max;
    }
    const int W = (m_max + 63) / 64;
    CBX_REQUIRE(ws_cap >= 8 * (long)nz * n_max * W, "align_path: a workspace of %ld bytes, the move words need 8 * %d * %d * %d", ws_cap, nz, n_max, W);
    hipLaunchKernelGGL(align_path_kernel, dim3((unsigned)nz), dim3((unsigned)(64 * W)), 0, (hipStream_t)stream, score, s_sb, s_si, rows, n_max, W,
                       (unsigned long long*)ws, spans, sp_sb, frame_tok, ft_sb);
    return cbx_check_launch("align_path");
}
