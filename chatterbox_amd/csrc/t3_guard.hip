// Alignment guard (cbx_guard_text_mass_f32, cbx_guard_update_f32; include/cbx.h): the quantity the word-timestamp pass reads after the fact (attn_align.hip) taken
// INSIDE the token step, for the one new query of every conditional row, and a small state machine per utterance that follows the text position, holds the
// end-of-speech token back until the text has been spoken and forces it when the alignment says the utterance is over.  Both launches are captured with the step:
// everything that varies per step or per request (positions, step, done, text lengths, thresholds) is read from device memory.  Plain C++: no inline assembly, no
// atomics, every output element written by exactly one thread in a fixed summation order, so two runs are bit-identical and the emulator build runs the same
// arithmetic (up to the library's expf / rsqrtf).
//
// Mass: one workgroup of 256 threads per (row, selected head), that head's K streamed ONCE.  Wave 0 rebuilds the row's q as the attention launch of the layer sees
// it (split-K parts added in part order, rstd, RoPE at positions[row]); a thread holds one key row (64 floats, 16-byte loads) in registers and reads q as LDS
// broadcasts; the scores of the whole causal row stay in LDS (4608 floats), so the maximum, the sum and the text columns are three passes over LDS, not over K.
// At the step's shapes (8 rows x 3 heads x <= 1.2 k keys: 7 MB) the launch is latency, not bandwidth; a split over workgroups would add a merge for nothing.
//
// Update: one workgroup of 1024 threads per utterance, thread t owns text column t (the head sum, the history store, its share of the two reductions); thread 0
// runs the scalar state machine; when a reason holds, the workgroup overwrites the utterance's two logit rows.
#include <math.h>

#include "cbx_common.h"

namespace {

constexpr int GM_NT = 256;      // threads of a mass workgroup
constexpr int GM_CTX = 4608;    // the RoPE table: scores of one causal row in LDS
constexpr int GM_TEXT = 1024;   // text columns
constexpr int GM_SEL = 16;      // selected heads of a launch
constexpr int GU_NT = 1024;     // threads of an update workgroup: one per text column

struct gm_heads_t {
    int h[GM_SEL];
};

// grid (B, n_sel) x 256
__global__ __launch_bounds__(GM_NT) void guard_text_mass_kernel(const float* __restrict__ qkv, long ld_qkv, int nparts, long part_stride, const float* __restrict__ ssq,
                                                                int rms_dim, float rms_eps, const int* __restrict__ positions, const float* __restrict__ cos_t,
                                                                const float* __restrict__ sin_t, const float* __restrict__ kc, long k_sr, long k_sh, int max_ctx,
                                                                gm_heads_t heads, const int* __restrict__ done, const int* __restrict__ t_len, int t0, int t_cap,
                                                                float scale, float* __restrict__ p, long p_ss, long p_sb) {
    __shared__ __attribute__((aligned(16))) float s_q[64];
    __shared__ float s_s[GM_CTX];
    __shared__ float s_red[2][GM_NT / 64];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (done[b]) return;
    const int tl = t_len[b], pos = positions[b];
    // (uniform over the workgroup, ahead of its barriers) a row the caps do not admit writes nothing and reads nothing of K
    if (tl < 1 || tl > t_cap || pos < 0 || pos >= max_ctx || t0 + tl > pos + 1) return;
    const int head = heads.h[s];
    if (wid == 0) {  // q as decode_attn_rope sees it (attention.hip): parts in part order, rstd of the projection's input, RoPE at positions[row]
        const float* qp = qkv + (long)b * ld_qkv + head * 64;
        float qv = qp[lane];
        if (nparts > 1) {
            float sq = ssq[b];
            for (int j = 1; j < nparts; ++j) qv += qp[j * part_stride + lane], sq += ssq[j * 16 + b];
            qv *= rsqrtf(sq / rms_dim + rms_eps);
        }
        const float c = cos_t ? cos_t[(long)pos * 64 + lane] : 1.f, sn = cos_t ? sin_t[(long)pos * 64 + lane] : 0.f;
        const float sgn = lane < 32 ? -1.f : 1.f;
        s_q[lane] = qv * c + sgn * __shfl_xor(qv, 32) * sn;
    }
    __syncthreads();
    // ---- the scores of the whole causal row, K read once: thread tid owns the keys j = tid (mod 256), j <= pos; nothing beyond pos is loaded
    const float* kh = kc + (long)b * k_sr + (long)head * k_sh;
    float mx = -INFINITY;
    for (int j = tid; j <= pos; j += GM_NT) {
        const float* kp = kh + (long)j * 64;
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kp + 4 * c);
            const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + 4 * c);
            acc = __builtin_fmaf(qv[0], kv[0], acc);
            acc = __builtin_fmaf(qv[1], kv[1], acc);
            acc = __builtin_fmaf(qv[2], kv[2], acc);
            acc = __builtin_fmaf(qv[3], kv[3], acc);
        }
        const float sc = scale * acc;
        s_s[j] = sc;
        mx = fmaxf(mx, sc);
    }
    for (int x = 32; x >= 1; x >>= 1) mx = fmaxf(mx, __shfl_xor(mx, x));
    if (lane == 0) s_red[0][wid] = mx;
    __syncthreads();  // (also: every score of the row is in LDS)
    float M = s_red[0][0];
#pragma unroll
    for (int w = 1; w < GM_NT / 64; ++w) M = fmaxf(M, s_red[0][w]);
    // ---- L: per thread in the order of its keys, the 64 lanes of a wave by the xor butterfly 32 .. 1, the waves in wave order
    float l = 0.0f;
    for (int j = tid; j <= pos; j += GM_NT) l += expf(s_s[j] - M);
    for (int x = 32; x >= 1; x >>= 1) l += __shfl_xor(l, x);
    if (lane == 0) s_red[1][wid] = l;
    __syncthreads();
    float L = s_red[1][0];
#pragma unroll
    for (int w = 1; w < GM_NT / 64; ++w) L += s_red[1][w];
    // ---- the text columns: the only elements stored
    float* o = p + (long)s * p_ss + (long)b * p_sb;
    for (int t = tid; t < tl; t += GM_NT) o[t] = expf(s_s[t0 + t] - M) / L;
}

// grid (B) x 1024.  state[b][8] = {pos, complete, completed_at, fired, fired_at, 0, 0, 0}; sums[b][4] = {tail_sum[3], rep_sum};
// thr[b][8] = {back, ahead, end_tokens, tail, repeat, repeat_skip, token_run, hold_min}
__global__ __launch_bounds__(GU_NT) void guard_update_kernel(const float* __restrict__ p, long p_ss, long p_sb, int n_sel, float weight, const int* __restrict__ t_len,
                                                             const int* __restrict__ step, const int* __restrict__ done, const float* __restrict__ thr,
                                                             const long long* __restrict__ out_tokens, int max_steps, float* __restrict__ mass, long m_sb, long m_si,
                                                             int* __restrict__ state, float* __restrict__ sums, int* __restrict__ trace, float* __restrict__ logits,
                                                             long ld_logits, int V, int B, int eos, float* __restrict__ dev_params) {
    __shared__ float s_a[GU_NT];
    __shared__ float s_bv[GU_NT / 64], s_rv[GU_NT / 64];
    __shared__ int s_bi[GU_NT / 64];
    __shared__ int s_reason;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
    int* stt = state + (long)b * 8;
    if (done[b] || stt[3]) return;  // a row that is done or has fired does nothing
    const int m = t_len[b], i = step[b];
    if (m < 1 || m > GU_NT || m > m_si || i < 0 || i >= max_steps) return;  // (uniform) nothing to follow, or no room for this step
    const float* th = thr + (long)b * 8;
    const int back = (int)th[0], ahead = (int)th[1], rskip = (int)th[5], token_run = (int)th[6], hold_min = (int)th[7];
    const int et = (int)th[2] < 1 ? 1 : (int)th[2] > 3 ? 3 : (int)th[2];  // tail_sum has three entries
    // ---- 1. a[t]: the heads in list order, then the weight; into the history
    float a = -INFINITY;  // columns beyond the text never win a maximum
    if (t < m) {
        float sum = 0.0f;
        for (int s = 0; s < n_sel; ++s) sum += p[(long)s * p_ss + (long)b * p_sb + t];
        a = weight * sum;
        mass[(long)b * m_sb + (long)i * m_si + t] = a;
    }
    s_a[t] = a;
    // ---- 2. the lowest t with the largest a[t]; the largest a[t] over t < m - repeat_skip
    float bv = a, rv = t < m - rskip ? a : -INFINITY;
    int bi = t;
    for (int x = 32; x >= 1; x >>= 1) {
        const float ov = __shfl_xor(bv, x);
        const int oi = __shfl_xor(bi, x);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        rv = fmaxf(rv, __shfl_xor(rv, x));
    }
    if (lane == 0) s_bv[wid] = bv, s_bi[wid] = bi, s_rv[wid] = rv;
    __syncthreads();
    if (t == 0) {
        float best = s_bv[0], rep = s_rv[0];
        int cur = s_bi[0];
        for (int w = 1; w < GU_NT / 64; ++w) {
            if (s_bv[w] > best) best = s_bv[w], cur = s_bi[w];  // (wave w holds higher columns than every wave before it: a tie keeps the lower)
            rep = fmaxf(rep, s_rv[w]);
        }
        if (m - rskip <= 0) rep = 0.0f;
        int pos = stt[0], complete = stt[1], completed_at = stt[2];
        const int d = cur - pos;
        if (d >= -back && d <= ahead) pos = cur;  // a jump outside the window is ignored
        // ---- 3. / 4.
        if (!complete && pos >= m - et) complete = 1, completed_at = i;
        float* sm = sums + (long)b * 4;
        const int nt = et < m ? et : m, first = m - nt;  // the last min(end_tokens, m) text columns
        float tail_max = -INFINITY;
        for (int j = 0; j < nt; ++j) {
            if (complete) sm[j] += s_a[first + j];
            tail_max = fmaxf(tail_max, sm[j]);
        }
        if (complete) sm[3] += rep;
        // ---- 5. the last token_run sampled tokens are one token
        bool run = token_run > 0 && i >= token_run;
        if (run) {
            const long long* ot = out_tokens + (long)b * max_steps;
            for (int k = 2; k <= token_run; ++k) run = run && ot[i - k] == ot[i - 1];
        }
        // ---- 6. / 7.
        const int reason = complete && tail_max >= th[3] ? 1 : complete && sm[3] >= th[4] ? 2 : run ? 3 : 0;  // (the two sums exist once complete)
        int ban = -1;
        if (reason) stt[3] = reason, stt[4] = i;
        else if (hold_min >= 0 && m >= hold_min && !complete) ban = eos;
        dev_params[(long)b * CBX_SAMPLER_NPARAMS + 6] = (float)ban;
        stt[0] = pos, stt[1] = complete, stt[2] = completed_at;
        trace[(long)b * max_steps + i] = pos | complete << 16 | (ban >= 0 ? 1 : 0) << 17 | reason << 18;
        s_reason = reason;
    }
    __syncthreads();
    if (s_reason) {  // both CFG rows: c + w (c - u) is this pattern for every w, so every processor order leaves probability 1 on the end token
        float* lc = logits + (long)b * ld_logits;
        float* lu = logits + (long)(B + b) * ld_logits;
        for (int v = t; v < V; v += GU_NT) {
            const float x = v == eos ? 32768.0f : 0.0f;
            lc[v] = x, lu[v] = x;
        }
    }
}

}  // namespace

extern "C" int cbx_guard_text_mass_f32(const float* qkv, long ld_qkv, int qkv_nparts, long qkv_part_stride, const float* qkv_ssq, int rms_dim, float rms_eps,
                                       const int* positions, const float* cos_t, const float* sin_t, const float* kc, long k_row_stride, long k_head_stride, int max_ctx,
                                       const int* heads, int n_sel, int n_heads, int B, const int* done, const int* t_len, int t0, int t_cap, float scale, float* p,
                                       long p_ss, long p_sb, void* stream) {
    CBX_REQUIRE(qkv && positions && kc && heads && done && t_len && p, "guard_text_mass: null pointer");
    CBX_REQUIRE((cos_t == nullptr) == (sin_t == nullptr), "guard_text_mass: cos_t and sin_t come together (both NULL: no RoPE)");
    CBX_REQUIRE(B >= 1 && B <= 64, "guard_text_mass: B = %d outside [1, 64]", B);
    CBX_REQUIRE(n_sel >= 1 && n_sel <= GM_SEL, "guard_text_mass: n_sel = %d outside [1, %d]", n_sel, GM_SEL);
    CBX_REQUIRE(n_heads >= 1, "guard_text_mass: n_heads = %d", n_heads);
    CBX_REQUIRE(qkv_nparts == 0 || qkv_nparts == 1 || qkv_nparts == 2 || qkv_nparts == 4, "guard_text_mass: qkv_nparts = %d (0 / 1, 2 or 4)", qkv_nparts);
    CBX_REQUIRE(qkv_nparts <= 1 || (qkv_ssq && rms_dim > 0 && qkv_part_stride >= 0 && B <= 16),
                "guard_text_mass: split-K parts need qkv_ssq ([nparts][16]: at most 16 rows), rms_dim > 0 and a part stride >= 0");
    CBX_REQUIRE(ld_qkv >= (long)n_heads * 64 && k_row_stride >= 0 && k_head_stride >= 0 && p_ss >= 0 && p_sb >= 0, "guard_text_mass: a stride that is negative or short");
    CBX_REQUIRE(((uintptr_t)kc & 15) == 0 && k_row_stride % 4 == 0 && k_head_stride % 4 == 0,
                "guard_text_mass: k is read with 16-byte loads (pointer on a 16-byte boundary, strides multiples of 4 floats)");
    CBX_REQUIRE(max_ctx >= 1 && max_ctx <= GM_CTX && k_head_stride >= (long)max_ctx * 64, "guard_text_mass: max_ctx = %d outside [1, %d], or beyond a head's keys (%ld floats)",
                max_ctx, GM_CTX, k_head_stride);
    CBX_REQUIRE(t0 >= 0 && t_cap >= 1 && t_cap <= GM_TEXT && p_sb >= t_cap && (n_sel == 1 || p_ss >= (B - 1) * p_sb + t_cap),
                "guard_text_mass: text columns [%d, %d + t_len), t_len <= t_cap = %d (at most %d), do not fit the strides of p (%ld, %ld)", t0, t0, t_cap, GM_TEXT, p_ss, p_sb);
    gm_heads_t hs;
    for (int s = 0; s < GM_SEL; ++s) hs.h[s] = 0;
    for (int s = 0; s < n_sel; ++s) {
        CBX_REQUIRE(heads[s] >= 0 && heads[s] < n_heads, "guard_text_mass: heads[%d] = %d outside [0, %d)", s, heads[s], n_heads);
        hs.h[s] = heads[s];
    }
    hipLaunchKernelGGL(guard_text_mass_kernel, dim3((unsigned)B, (unsigned)n_sel), dim3(GM_NT), 0, (hipStream_t)stream, qkv, ld_qkv, qkv_nparts, qkv_part_stride, qkv_ssq,
                       rms_dim, rms_eps, positions, cos_t, sin_t, kc, k_row_stride, k_head_stride, max_ctx, hs, done, t_len, t0, t_cap, scale, p, p_ss, p_sb);
    return cbx_check_launch("guard_text_mass");
}

extern "C" int cbx_guard_update_f32(const float* p, long p_ss, long p_sb, int n_sel, const int* t_len, const int* step, const int* done, const float* thresholds,
                                    const long long* out_tokens, int max_steps, float* mass, long m_sb, long m_si, int* state, float* sums, int* trace, float* logits,
                                    long ld_logits, int V, int B, int eos, float* dev_params, void* stream) {
    CBX_REQUIRE(p && t_len && step && done && thresholds && out_tokens && mass && state && sums && trace && logits && dev_params, "guard_update: null pointer");
    CBX_REQUIRE(B >= 1 && B <= 64, "guard_update: B = %d outside [1, 64]", B);
    CBX_REQUIRE(n_sel >= 1 && n_sel <= 1024, "guard_update: n_sel = %d outside [1, 1024]", n_sel);
    CBX_REQUIRE(max_steps >= 1 && V >= 1 && eos >= 0 && eos < V && ld_logits >= V, "guard_update: max_steps = %d, V = %d, eos = %d, ld_logits = %ld", max_steps, V, eos, ld_logits);
    CBX_REQUIRE(p_ss >= 0 && p_sb >= 0 && m_si >= 1 && (B == 1 || m_sb >= (long)max_steps * m_si), "guard_update: strides of p (%ld, %ld) or of the history (%ld, %ld)", p_ss,
                p_sb, m_sb, m_si);
    hipLaunchKernelGGL(guard_update_kernel, dim3((unsigned)B), dim3(GU_NT), 0, (hipStream_t)stream, p, p_ss, p_sb, n_sel, 1.0f / (float)n_sel, t_len, step, done, thresholds,
                       out_tokens, max_steps, mass, m_sb, m_si, state, sums, trace, logits, ld_logits, V, B, eos, dev_params);
    return cbx_check_launch("guard_update");
}
