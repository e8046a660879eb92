/* cbx.h -- C ABI of libcbx_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the Chatterbox hot path
 * generate() = T3.inference -> S3Gen.flow_inference -> HiFT.inference.
 *
 * The reference (resemble-ai/chatterbox) has no FFI: its numerical layer is PyTorch ATen + HF transformers +
 * diffusers called from Python.  Each entry point below replaces the ATen/HF op group that the cited reference
 * lines dispatch; INTEGRATION.md shows the ctypes binding.  Conventions:
 *   - plain C types only; every pointer is a DEVICE pointer valid on `stream` (a hipStream_t passed as void*);
 *   - all tensors fp32 row-major "channel-last" (rows = time/tokens, columns = channels) unless stated;
 *   - the callee never allocates, never synchronises, and is hipGraph-capturable;
 *   - return 0 on success, else a negative CBX_E* / positive hipError_t; cbx_last_error() gives text.
 */
#ifndef CBX_H
#define CBX_H
#ifdef __cplusplus
extern "C" {
#endif

#define CBX_ABI_VERSION 16 /* 2: cbx_gemm_t.precision, cbx_flash_attn_split_f32; 4: packed decode GEMV operands, RMSNorm / residual folded into cbx_gemv_f32;
                              5: precision 16 (f16x3) + cbx_set_range_flag; 6: LayerNorm folded into the GEMM A operand (ln_stats / ln_w / ln_b, cbx_row_stats_f32);
                              7: plane-format operands (cbx_gemm_planes, cbx_split_planes_f32, cbx_layernorm_planes_f32, cbx_flash_attn_split_po),
                                 per-device range flag, cbx_gemm_ln_fusable; 8: cbx_gemm_pl_t.PT (transposed column range), cbx_set_decode_attn_workspace;
                              9: 12- and 4-column decode GEMV tiles (cbx_gemv_t.half_tile = 12 / 4), cbx_t3_step_t.qkv_tile, d_ksplit = 1;
                              10: no process-wide state on the decode path -- cbx_decode_attn_t / cbx_decode_attn_rope (geometry and the split-context
                                  workspace per call), cbx_gemv_t.flags, cbx_t3_step_t.da_* / gemv_flags; the cbx_set_* setters remain as TEST HOOKS of
                                  the positional entry points only;
                              11: cbx_gemv_t.col_tiles / ssq_out (column-tile / split-K form of the RMSNorm-folded decode GEMV), cbx_decode_attn_t.qkv_nparts /
                                  qkv_part_stride / qkv_ssq / rms_dim / rms_eps (the attention adds the q/k/v partial sums and applies rstd),
                                  cbx_t3_step_t.qkv_ksplit / qkv_ct / head_ct / qkv_ssq, cbx_t3_prefill;
                              12: stage-level seams of the flow and the vocoder: cbx_planes_t, cbx_s3gen_encode, cbx_cfm_solve, cbx_hift_f0_source, cbx_hift_decode;
                              13: per-call launch geometry of the plane-format kernels (cbx_gemm_pl_t.tile, cbx_flash_attn_planes_v, cbx_cfm_t.gemm_tile /
                                  attn_version: no process-wide state on the flow path either) incl. the CO-RESIDENT forms of the throughput schedule
                                  (one workgroup per CU that leaves half of the register file and 64 KiB of LDS to another stream), CBX_GEMV_SHALLOW;
                              14: the batch-1 decode path of the GPT-2 backbones (Turbo / Nano): cbx_gemv_row_f32, cbx_decode_attn_parts; the token loop in C: cbx_t3_loop_*;
                              15: cbx_flash_attn_kv_f32 (K / V head strides: attention over the KV cache in the prefill);
                              16: cbx_gpt2_prefill (the prefill of the GPT-2 backbones as one call, optionally behind a cached conditioning prefix); added
                                  later without a version step (no existing struct or signature changed): cbx_gpt2_decode_step, cbx_gpt2_loop_*; cbx_prefill_embed,
                                  cbx_kv_prefix_paste_f32 (batched public API: the prefill input and the cached voice prefixes of a mixed-voice batch, one launch each) */
#define CBX_EINVAL (-22)

/* activations usable in GEMM / elementwise epilogues */
enum { CBX_ACT_NONE = 0, CBX_ACT_SILU = 1, CBX_ACT_GELU_ERF = 2, CBX_ACT_GELU_TANH = 3, CBX_ACT_MISH = 4,
       CBX_ACT_LRELU = 5, CBX_ACT_ELU = 6, CBX_ACT_TANH = 7, CBX_ACT_SNAKE = 8, CBX_ACT_ABS = 9 };

int cbx_abi_version(void);
const char* cbx_last_error(void);

/* ---- implicit-GEMM linear / conv1d / batched matmul on fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32) ----
 * C[z][m][n] = beta*C + alpha*( act1( sum_{tap,c} A[z][ (m*stride + tap*dil - pad_left)/up ][c] * W[z][n][tap*Cin+c]
 *                                      + bias[n] ) + R[z][m][n] ),      C2 = act2(C)   (optional)
 * Replaces F.linear / F.conv1d / F.conv_transpose1d (phase-packed weights) / torch.matmul on:
 *   HF LlamaAttention/LlamaMLP projections (models/t3/t3.py:326-333,378-384), CFM estimator convs and
 *   transformer-block linears (models/s3gen/decoder.py:243-333, matcha/transformer.py:243-316), conformer
 *   encoder linears/convs (transformer/upsample_encoder.py:237-304), HiFT convs (hifigan.py:412-444).
 * z = z1*nz2 + z2 (two-level batch: e.g. utterance row, attention head).
 * K is walked in float4 units: K % 4 == 0 -- a call with any other K is REFUSED (on strided views its tail float4 would multiply the
 * 1 .. 3 columns behind K of both operands in): pad K with zero columns -- except with w_kn, where A only has to be readable and finite
 * up to the next multiple of 4 (W rows >= K read as zero).
 */
typedef struct cbx_gemm_t {
    const float* A; const float* W; float* C;
    const float* bias;        /* [N] or NULL */
    const float* R;           /* residual, or NULL */
    float* C2;                /* second output act2(C), or NULL */
    const float* act1_param;  /* per-column parameter of act1 (snake alpha) or NULL */
    const float* act2_param;
    const int* lens;          /* per-z1 number of valid INPUT rows (rows >= lens read as 0), or NULL */
    int M, N, K;              /* output rows per batch, output columns, K = taps*Cin */
    int Cin, taps, dil, stride, pad_left, up, Tin;
    int nz1, nz2;
    int w_kn;                 /* 0: W is [N][K] (torch Linear layout); 1: W is [K][N] (e.g. P @ V) */
    int swiglu;               /* 1: packed [32 gate | 32 up] column groups -> C[m][N/2] = silu(gate)*up */
    int act1, act2;
    float act1_slope, act2_slope, alpha, beta;
    long lda, a_s1, a_s2;     /* strides in floats */
    long ldw, w_s1, w_s2;
    long ldc, c_s1, c_s2;
    long ldr, r_s1, r_s2;
    long ldc2, c2_s1, c2_s2;
    int precision;            /* 0 = exact; 1 = exact fp32 MFMA
                                 (bitwise an fmaf chain); 3 = "bf16x3", 6 = "bf16x6": every fp32 operand split into 2 / 3
                                 bf16 planes and the product rebuilt from 3 / 6 bf16-MFMA plane products with fp32
                                 accumulation (rel. error ~4e-6 / ~1e-7; fp32 MFMA ~2.5e-7); 16 = "f16x3": two fp16 planes
                                 a = h + l/2048, three fp16-MFMA products in two fp32 accumulators (rel. error ~1e-7 at the cost of
                                 bf16x3; operands must satisfy |a| <= 65504, see cbx_set_range_flag).  Shapes the split kernel does
                                 not serve (w_kn, swiglu, M <= 32, conv Cin % 32 != 0) run exact. */
    int reserved0;
    /* ABI v6: LayerNorm folded into the A operand of a Linear (precision 16, taps == 1, nz == 1, no lens):
     * A'[m][k] = (A[m][k] - mean[m]) * rstd[m] * ln_w[k] + ln_b[k] is applied on the way to the matrix cores, so the standalone
     * F.layer_norm pass (one read + one write of the activation) becomes a statistics pass (cbx_row_stats_f32: one read). */
    const float* ln_stats;    /* [M][2] = {mean, rstd} per row, or NULL */
    const float* ln_w;        /* [K] */
    const float* ln_b;        /* [K] */
} cbx_gemm_t;
int cbx_gemm_f32(const cbx_gemm_t* p, void* stream);
/* Device word that every precision-16 launch (GEMM, flash attention, plane-format producers) ORs a 1 into when it meets an operand outside
 * the fp16 range (its result is then not meaningful and the caller repeats the computation at precision 6, which has the fp32 exponent
 * range).  NULL (the default) = not reported.  One word PER DEVICE: the call registers the word for the calling thread's current device and
 * a launch reports into the word of the device it runs on; the word must stay allocated while such launches are in flight. */
int cbx_set_range_flag(int* dev_flag);
/* stats[r] = {mean, rstd = 1/sqrt(var + eps)} of row r of x (C = 256: the CFM transformer blocks), computed exactly as cbx_layernorm_f32
 * computes them; feeds cbx_gemm_t.ln_stats.  Replaces the statistics half of F.layer_norm (matcha/transformer.py:243-316 norm1 / norm3). */
int cbx_row_stats_f32(const float* x, float* stats, long rows, int C, long ldx, float eps, void* stream);

/* Would cbx_gemm_f32 accept ln_stats for a precision-16 Linear with M rows, K columns and row stride lda (floats)?  0 when a tuning knob
 * (cbx_set_split_tile) or a > 2 GiB operand rules the folded form out: the caller then runs
 * cbx_layernorm_f32 + a plain Linear (F.layer_norm + F.linear, matcha/transformer.py:243-316). */
int cbx_gemm_ln_fusable(long M, int K, long lda);

/* ---- PLANE-FORMAT operands (ABI v7): the f16x3 arithmetic without per-tile conversion ----
 * A "planes" tensor stores an fp32 tensor X as two fp16 planes X = h + l / 2048, h = RNE16(X), l = RNE16(2048 (X - h)): element (row, c)
 * of plane h at base[row*ld + c], of plane l at base[row*ld + lo + c] (halves) -- the same 4 bytes per element as fp32, 22 significand
 * bits (the f16x3 mode of cbx_gemm_t.precision; |X| <= 65504, producers raise the cbx_set_range_flag word otherwise).
 * Constant weights are split once at load, activations are WRITTEN in plane format by their producer (the epilogues below), and the
 * consumer's K loop is a plain fp16 MFMA loop fed by direct global -> LDS loads.
 *
 * cbx_gemm_planes: C[z][m][n] and / or P[z][m][n] = act( sum_{tap,c} A[z][m*stride + tap*dil - pad_left][c] * W[n][tap*Cin + c] + bias[n] )
 *                                                      + R[z][m][n]      (act: none, GELU (erf) or SiLU; act_param / alpha reserved: NULL / 0 or 1)
 * A, W planes (W in [N][K] layout); C fp32 and / or P planes (either may be NULL); R fp32 residual.  Rows outside [0, min(Tin, lens[z]))
 * read as zero.  K % 32 == 0, Cin % 32 == 0.  Replaces the F.linear / F.conv1d calls of the CFM estimator: CausalConv1d / ResnetBlock1D
 * (models/s3gen/decoder.py:49-98, matcha/decoder.py:56-61), BasicTransformerBlock projections and FeedForward (matcha/transformer.py:243-316),
 * final_proj (decoder.py:331-333). */
typedef struct cbx_gemm_pl_t {
    const void* A; const void* W;   /* fp16 planes */
    float* C;                       /* fp32 output or NULL */
    void* P;                        /* planes output or NULL */
    const float* bias;              /* [N] or NULL */
    const float* R;                 /* fp32 residual or NULL */
    const float* act_param;         /* per-column activation parameter or NULL */
    const int* lens;                /* per-z number of valid INPUT rows or NULL */
    int M, N, K;                    /* output rows per batch, columns, K = taps * Cin */
    int Cin, taps, dil, stride, pad_left, Tin, nz1;
    int act; float act_slope, alpha;
    long lda, a_lo, a_s1;           /* halves */
    long ldw, w_lo, w_s1;           /* halves; w_s1 = per-batch stride of W (0: shared) */
    long ldc, c_s1;                 /* floats */
    long ldr, r_s1;                 /* floats */
    long ldp, p_lo, p_s1;           /* halves */
    int reserved0;                  /* 0 (diagnostic switches of a -DCBX_DIAG build) */
    /* ABI v8 -- transposed plane output for a column range (the V^T operand of cbx_flash_attn_planes produced by the SAME launch as the
     * q | k projection: to_q / to_k / to_v of matcha/transformer.py:243-316 as ONE Linear over [Wq; Wk; Wv]).  PT != NULL: output columns
     * n >= pt_n0 are not written to C / P; element (m, n) goes to PT[(m / pt_T) * pt_zs + (n - pt_n0) * pt_ld + (m % pt_T)] (h plane; the
     * l plane pt_lo halves further), i.e. one (N - pt_n0) x pt_T matrix per group of pt_T rows.  Needs P for the columns below pt_n0,
     * pt_n0 % 256 == 0, pt_T % 4 == 0, M % 4 == 0, no C / R / activation, nz1 == 1. */
    void* PT; int pt_n0, pt_T; long pt_ld, pt_lo, pt_zs;   /* halves */
    /* ABI v13 -- launch geometry of THIS call: 0 = the library's measured choice (or the cbx_set_planes_tile test hook); n > 0 = form n of the tile menu
     * (gemm_planes.hip); CBX_PL_TILE_CORESIDENT (-1) = the measured choice among the forms that leave room on the CU: ONE workgroup of 8 waves and <= 120
     * VGPRs per CU (form 8 where K % 64 == 0: 128 KiB of LDS, 32 KiB left; form 17 otherwise: 96 KiB), so that the workgroups of a latency-bound kernel chain on ANOTHER stream (the T3 decode step of the next
     * batch) stay co-resident instead of waiting for these to retire (profiles/r05_overlap_*); round 6: the two wide Linears of a transformer block (ff1 + GELU, q | k | v) keep
     * their loader-wave forms even then (measured: profiles/r06_{s,t,v}_*_ab.log).  Forms 41 / 42 (round 6) = forms 32 / 35 with the DEFERRED epilogue: a finished tile is folded
     * and the rest of its epilogue is issued between the MFMA groups of the workgroup's next tile.  Same arithmetic in every form. */
    int tile;
    /* ABI v13 -- LayerNorm of the FINISHED row, produced by the epilogue (N == 256 only: the attention out-projection, ff2 and the 1 x 1 residual conv of the CFM
     * estimator, whose consumer is nn.LayerNorm -> Linear, matcha/transformer.py:243-316 norm3 / the next block's norm1).  ln_w != NULL: besides C (the fp32
     * row incl. bias and residual) the launch writes LNP[m][n] = (C[m][n] - mean_m) * rstd_m * ln_w[n] + ln_b[n] in plane format (row stride ld_lnp, plane
     * offset lnp_lo, batch stride lnp_s1, halves), mean / variance over the 256 columns in fp32 (two passes, as cbx_layernorm_f32), eps ln_eps.  It replaces the
     * cbx_layernorm_planes_f32 launch between the two Linears.  Needs N == 256, K % 32 == 0, no activation, no P / PT; runs on the row-spanning 64 x 256 tile. */
    const float* ln_w; const float* ln_b; void* LNP; long ld_lnp, lnp_lo, lnp_s1; float ln_eps;
} cbx_gemm_pl_t;
#define CBX_PL_TILE_CORESIDENT (-1)
/* ABI v13: a stream ATTRIBUTE (like its priority): launches on a co-resident stream that would otherwise put several workgroups of one kernel on a CU
 * (LayerNorm, the split-operand GEMM of the encoder / vocoder) reserve enough LDS that at most one or two fit, so half of every SIMD's register file stays free
 * for another stream's kernels.  No effect on results.  Mark a stream once, before using it (ChatterboxEngine marks its flow + vocoder stream). */
int cbx_set_stream_coresident(void* stream, int on);
int cbx_gemm_planes(const cbx_gemm_pl_t* p, void* stream);
/* tuning knob: tile shape of cbx_gemm_planes (0 = automatic; see gemm_planes.hip) */
int cbx_set_planes_tile(int t);
/* tuning knob: 1 (default) = persistent workgroups walking several output tiles each (DMA runs across tile boundaries), 0 = one tile per workgroup */
int cbx_set_planes_persist(int on);
/* x (rows, C) fp32 -> planes (weights at load; estimator inputs).  C, ldx, ldp, p_lo multiples of 4. */
int cbx_split_planes_f32(const float* x, void* planes, long rows, int C, long ldx, long ldp, long p_lo, void* stream);
/* cbx_layernorm_f32 (C = 256, LayerNorm form) whose result is written in plane format: nn.LayerNorm (+ Mish + time bias) feeding a conv /
 * Linear (decoder.py:49-63, matcha/transformer.py:243-316 norm1 / norm3). */
int cbx_layernorm_planes_f32(const float* x, void* planes, const float* w, const float* b, const float* post_add, long rows, int C,
                             long ldx, long ldp, long p_lo, float eps, int act, float out_scale, void* stream);

/* ---- skinny-M weight-streaming GEMM for decode (M = 2*B rows <= 64), HBM-roofline kernel ----
 * out[ks][m][n] = sum_{k in slice ks} x[m][k] * W[n][k]  (+ bias on slice 0);  ksplit > 1 leaves partial sums that
 * cbx_add_rmsnorm_f32 reduces in fixed order.  swiglu: W is the packed [32 gate | 32 up] image, N = #features,
 * out[m][f] = silu(gate_f) * up_f.  Replaces the q_len == 1 HF Llama projections + speech head (t3.py:378-386). */
typedef struct cbx_gemv_t {
    const float* x; const float* W; const float* bias; float* out;
    int M, N, K;
    int ksplit;      /* K slices across workgroups (grid.y) */
    int nw;          /* waves per workgroup sharing one 16-column tile: 4 or 8 */
    int swiglu;
    int act;         /* CBX_ACT_* applied after the bias (ksplit == 1 only): gelu_new of GPT-2's c_fc */
    long ldx, ldw, ldo, part_stride;
    /* ABI v4 */
    int w_packed;    /* W is the lane-ordered packed image written by cbx_pack_gemv_weight_f32 (ldw ignored; swiglu: tiles
                        2f = gate, 2f+1 = up of feature tile f) */
    int x_packed;    /* x is in the same packed layout (rows padded to 16, ldx ignored); needs w_packed */
    int half_tile;   /* (was reserved0) narrow output tiles: 0 = 16 columns per workgroup; 1 or 8 = 8 columns (W is the 8-row-tile packed
                        image, cbx_pack_gemv_weight_f32 with swiglu = 8): twice the workgroups for projections with few output tiles
                        (N = 1024: 128 instead of 64); 12 / 4 = 12 / 4 columns (images packed with swiglu = 12 / 4): N = 3072 resp.
                        N = 1024 on exactly 256 workgroups.  Same per-column arithmetic as the 16-column form (bit-identical results) */
    int out_packed;  /* out (and res) use the packed operand layout of the CONSUMING gemv (its K = this N; N % 32 == 0); with ksplit > 1
                        the partial images are part_stride floats apart */
    const float* norm_w; /* [K] or NULL: LlamaRMSNorm(x) folded in (x * norm_w feeds the MFMAs, rstd applied in the epilogue);
                            needs w_packed, x_packed, ksplit == 1 */
    const float* res;    /* or NULL: out = res + x W^T, res in the same layout as out (in place allowed); ksplit == 1 */
    float eps;           /* RMSNorm epsilon */
    int n_xpart;         /* 0, 2 or 4: the x operand is x + sum_j xpart[j] (split-K partial images of the producing projection, packed
                            layout, reduced in fixed order on the way to the MFMA); needs norm_w, nw == 8, M <= 16 -- or M <= 32 (two whole row tiles per
                            image, pad rows zero) in the plain RMSNorm fp32 form: no swiglu, ln_cw or w_bf16 */
    const float* xpart;  /* [n_xpart] images, xpart_stride floats apart */
    long xpart_stride;
    float* x_out;        /* or NULL: receives x + sum_j xpart[j] (packed; must not alias x: other workgroups still read it).  Since ABI v11 rows >= M of
                          * a packed image (x_packed operands, xpart, x_out) are NEITHER READ NOR WRITTEN: lanes past M fetch row 0 and are zeroed before
                          * the MFMA, x_out stores are guarded -- a host that reuses a buffer keeps whatever its pad rows held (the engines zero theirs) */
    int w_bf16;          /* W is a cbx_pack_gemv_weight_bf16 image (opt-in: weights rounded to bf16, half the streamed bytes; M <= 16) */
    int flags;           /* (was reserved1) ABI v10, CBX_GEMV_* bits below; 0 = the plain launch */
    const float* ln_cw;  /* or NULL: LayerNorm instead of RMSNorm (GPT-2 ln_1 / ln_2 / ln_f): with norm_w = LN weight w, ln_cw[n] = */
    const float* ln_cb;  /* sum_k w[k] W[n][k] and ln_cb[n] = sum_k b[k] W[n][k] + bias[n] (constants of the layer, computed at load): */
                         /* out[m][n] = rstd[m] (sum_k x' w W - mean'[m] ln_cw[n]) + ln_cb[n], then `act`, on the SHIFTED row x' = x - c[m], c[m] = the */
                         /* median of channels 0, K/2, K - 1 of the (summed) row: mean' = sum_k x' / K, rstd = rsqrt(sum_k x'^2 / K - mean'^2 + eps) -- */
                         /* the one-pass variance and the mean term do not cancel when |mean| >> std; x_out still receives the unshifted row */
    /* ABI v11 -- column-tile / split-K form of the RMSNorm-folded packed GEMV (norm_w, packed fp32 operands in the 16-column image, M <= 16 -- or M <= 32 with
     * col_tiles <= 3 and no ln_cw: two row tiles share every weight register, each row bit for bit what a launch on its own 16-row image gives --, no
     * bias / residual / activation; xpart / x_out as above).  col_tiles = 1 .. 4: a workgroup owns that many 16-column tiles, which share every x
     * register (activation : weight bytes per workgroup = 1 : col_tiles instead of 1 : 1 -- the decode GEMVs are bound by the bytes a CU moves,
     * profiles/r04_decode_launch_timeline.txt), and 1 / ksplit of K on 8 waves (K % (256 ksplit) == 0).  ksplit == 1: out = RMSNorm(x) W^T as
     * before.  ksplit > 1: out[ks] (part_stride floats apart) holds the UN-normalised partial sums of K slice ks and ssq_out[ks * 16 * ceil(M / 16) + m] the
     * slice's sum of squares of row m: the consumer adds the partials in fixed order and applies rstd = rsqrt(sum_ks ssq / K + eps)
     * (cbx_decode_attn_t.qkv_nparts does).  0 = the one-tile form above. */
    int col_tiles;
    float* ssq_out;
} cbx_gemv_t;
/* Packed GEMV weight layout (decode path; the weights are constants, so they are laid out once for the MFMA lane order):
 *   dst[(((tile * (K/32) + kb) * 2 + h) * 64 + lane) * 4 + s] = src[tile*16 + (lane & 15)][kb*32 + (lane >> 4)*8 + h*4 + s]
 * i.e. each (16-row tile, 32-deep K block) is 2 KiB of contiguous memory in exactly the order the 64 lanes of a wave load it
 * (two 1-KiB instructions).  Rows are zero-padded to a multiple of 16.  swiglu = 1: src holds [gate (F rows); up (F rows)] and
 * the tiles are interleaved gate/up per 16 features.  dst must hold ceil(N/16)*16*K floats.
 * swiglu = 8 / 12 / 4: the narrow-tile image (tr-row tiles, 4 * tr lanes per half block: dst[(((tile * (K/32) + kb) * 2 + h) * 4 * tr + q * tr + c) * 4 + s]
 * = src[tile * tr + c][kb*32 + q*8 + h*4 + s]) for cbx_gemv_t.half_tile; dst holds ceil(N/tr)*tr*K floats. */
int cbx_pack_gemv_weight_f32(const float* src, float* dst, int N, int K, long ld_src, int swiglu, void* stream);
/* the same image with the weights rounded (RNE) to bf16: [tile][K/32][lanes][8 bf16] (cbx_gemv_t.w_bf16); dst holds half the bytes */
int cbx_pack_gemv_weight_bf16(const float* src, void* dst, int N, int K, long ld_src, int swiglu, void* stream);
int cbx_gemv_f32(const cbx_gemv_t* p, void* stream);
/* cbx_gemv_t.flags (ABI v10: per launch, set by the caller -- the engines carry them in their own tune, nothing process-wide):
 * CBX_GEMV_PRE_EPI: the launch requests the operands of its epilogue (residual element, bias, LayerNorm-fold constants) together with its first
 *   weight batch instead of after the reduction -- one dependent memory round trip less; same values added in the same order.
 * CBX_GEMV_DEEP: an 8-wave plain packed GEMV whose waves own >= 256 of K (the down projection with ksplit = 1) requests 8 K blocks per batch
 *   instead of 4 -- half the dependent load batches.  Both: results unchanged bit for bit (tests/test_zz_abi_v9_gpu.py, on hardware). */
#define CBX_GEMV_PRE_EPI 1
#define CBX_GEMV_DEEP 2
/* CBX_GEMV_SHALLOW (ABI v13): the RMSNorm-folded SwiGLU launch (gate | up of the decode step) requests 2 K blocks per batch instead of 4: <= 128 VGPRs instead of
 * 162, so that its workgroups fit on a CU beside a workgroup of ANOTHER stream that leaves half of the register file free (the throughput schedule of
 * ChatterboxEngine.synthesize_pipelined: T3 of batch k + 1 beside flow + vocoder of batch k).  Same products, same order: bit-identical. */
#define CBX_GEMV_SHALLOW 4
/* TEST HOOKS (default 0): OR the bit into the flags of EVERY cbx_gemv_f32 launch of the process. */
int cbx_set_gemv_deep_batches(int on);
int cbx_set_gemv_epilogue_prefetch(int on);
/* x += sum_k part[k] (fixed order), h = RMSNorm(x) * w : residual add + split-K reduce + LlamaRMSNorm in one pass (the residual /
 * input_layernorm / post_attention_layernorm steps of HF LlamaDecoderLayer inside T3.inference's loop, t3.py:378-386) */
int cbx_add_rmsnorm_f32(float* x, const float* part, int ksplit, long part_stride, long ldp, const float* w, float* h,
                        int rows, int C, long ldx, long ldh, float eps, void* stream);
/* same with LayerNorm (rms = 0, bias b) for the GPT-2 backbone of Turbo/Nano (HF GPT2Block ln_1 / ln_2 / ln_f, driven by
 * T3.inference_turbo, t3.py:392-468) */
int cbx_add_norm_f32(float* x, const float* part, int ksplit, long part_stride, long ldp, const float* w, const float* b,
                     float* h, int rows, int C, long ldx, long ldh, float eps, int rms, void* stream);

/* ---- normalisation (wavefront reductions, one wave per row) ----
 * LayerNorm / RMSNorm over the last dim (C <= 4096, C % 4 == 0):
 *   y = act( (x-mean)*rstd*w + b ) [+ post_add[c]] [* rowmask]            (nn.LayerNorm, HF LlamaRMSNorm)
 * Replaces F.layer_norm (+Mish of CausalBlock1D, decoder.py:49-63) and LlamaRMSNorm. */
int cbx_layernorm_f32(const float* x, float* y, const float* w, const float* b, const float* post_add,
                      long rows, int C, long ldx, long ldy, float eps, int rms, int act, float out_scale,
                      void* stream);

/* ---- attention ----
 * Flash-style fp32 attention, head_dim 64: O = softmax(scale*Q K^T + mask) V, one (z1,head) per grid.y slice.
 * q/k/v/o are addressed as base + z1*s_b + t*s_t + head*64 (+ kv: s_kb/s_kt). key_lens[z1] masks keys >= len
 * (diffusers additive -1e10 bias, decoder.py:26-34,285-286); causal!=0 adds j<=i+causal_off (HF sdpa is_causal).
 * Replaces F.scaled_dot_product_attention in diffusers AttnProcessor2_0 and HF sdpa_attention_forward. */
int cbx_flash_attn_f32(const float* q, const float* k, const float* v, float* o, const int* key_lens,
                       int nz1, int n_heads, int Tq, int Tk, long q_sb, long q_st, long k_sb, long k_st,
                       long v_sb, long v_st, long o_sb, long o_st, float scale, int causal, void* stream);
/* ABI v15: the same with HEAD strides for K and V (k_sh / v_sh floats between the heads of one token; cbx_flash_attn_f32 = 64): keys and values read where
 * DynamicCache keeps them -- T3's KV cache [row][head][max_ctx][64] has k_st = 64, k_sh = max_ctx * 64.  Serves the prefill of the TEXT positions of T3.inference
 * when the 34 conditioning positions of a voice are already cached (t3.py:303-335: the prompt [cond | text | BOS BOS]; HF sdpa is_causal with Tq < Tk: query i sees
 * keys j <= i + (Tk - Tq)). */
int cbx_flash_attn_kv_f32(const float* q, const float* k, const float* v, float* o, const int* key_lens, int nz1, int n_heads, int Tq, int Tk,
                          long q_sb, long q_st, long k_sb, long k_st, long k_sh, long v_sb, long v_st, long v_sh, long o_sb, long o_st, float scale,
                          int causal, void* stream);
/* Same contract on the bf16 / fp16 matrix cores with split fp32 operands: precision 3 ("bf16x3", rel. error ~4e-6 per
 * contraction), 6 ("bf16x6", fp32-level) or 16 ("f16x3", fp32-level, fp16 operand range), see cbx_gemm_t.precision.
 * 5.3x / 2.7x / 5.3x fewer matrix-core cycles. */
int cbx_flash_attn_split_f32(const float* q, const float* k, const float* v, float* o, const int* key_lens,
                             int nz1, int n_heads, int Tq, int Tk, long q_sb, long q_st, long k_sb, long k_st,
                             long v_sb, long v_st, long o_sb, long o_st, float scale, int causal, int precision,
                             void* stream);

/* cbx_flash_attn_split_f32 at precision 16 whose output is written in plane format (o_sb / o_st / o_lo in halves): the attention result
 * feeds only the to_out projection (matcha/transformer.py:275-283 via diffusers Attention), a cbx_gemm_planes. */
int cbx_flash_attn_split_po(const float* q, const float* k, const float* v, void* o_planes, const int* key_lens,
                            int nz1, int n_heads, int Tq, int Tk, long q_sb, long q_st, long k_sb, long k_st,
                            long v_sb, long v_st, long o_sb, long o_st, long o_lo, float scale, int causal, void* stream);

/* (cbx_mlp_planes -- the fused feed-forward launch of ABI v7-v12 -- is gone: measured equal at B = 8 and 18-27 % behind at batch 1, no configuration wanted it) */
/* Flash attention (head_dim 64, f16x3 arithmetic) on plane-format operands: q, k [token][d] planes as a cbx_gemm_planes P output holds them,
 * vt = V^T [d][token] planes (the v projection computed with swapped operands: A = W_v, W = the activations; row stride vt_sd >= Tk rounded
 * up to 8, tails finite), o [token][d] planes.  All strides / plane offsets in halves; heads are 64 columns (q, k, o) or 64 rows (vt) apart.
 * No operand conversion, no VALU staging: K and V^T tiles are DMA'd global -> LDS.  Replaces diffusers Attention / F.scaled_dot_product_attention
 * inside BasicTransformerBlock (matcha/transformer.py:243-316). */
int cbx_flash_attn_planes(const void* q, const void* k, const void* vt, void* o, const int* key_lens, int nz1, int n_heads, int Tq,
                          int Tk, long q_sb, long q_st, long q_lo, long k_sb, long k_st, long k_lo, long vt_sb, long vt_sd,
                          long vt_lo, long o_sb, long o_st, long o_lo, float scale, int causal, void* stream);
/* ABI v13: the same with the kernel version chosen PER CALL (0 = the library's automatic choice: version 4, or its 128-query twin (the kernel of version 5) where the grid
 * of 256-query workgroups would fill at most half of the chip -- batch 1; else 1 .. 6 as cbx_set_attn_planes_version).  5 = the CO-RESIDENT form:
 * the free-running loop of version 4 on 4-wave workgroups of 128 queries, one per CU (96 KiB of LDS, one wave of ~200 VGPRs per SIMD): 3/5 of the register
 * file stay free for another stream's workgroups; bit-identical to version 4; +8 % per launch when alone (profiles/r05_overlap_*). */
int cbx_flash_attn_planes_v(const void* q, const void* k, const void* vt, void* o, const int* key_lens, int nz1, int n_heads, int Tq,
                            int Tk, long q_sb, long q_st, long q_lo, long k_sb, long k_st, long k_lo, long vt_sb, long vt_sd,
                            long vt_lo, long o_sb, long o_st, long o_lo, float scale, int causal, int version, void* stream);
/* tuning knob (A/B hook, no engine calls it): kernel version of cbx_flash_attn_planes (0 = automatic; 4 = free-running loop, every wave meets the others once per
 * key tile; 2 = two wave groups alternating matrix / vector blocks; 1 = one group; 3 = version 2 with wave priorities; 6 = version 4 with its DMAs issued between
 * the softmax and the PV product: measured equal, profiles/r06_y_*) */
int cbx_set_attn_planes_version(int v);

/* Single-query decode attention over a KV cache (HF DynamicCache + sdpa, q_len == 1; t3.py:378-384).
 * cache layout [row][head][pos][64]; ctx_lens[row] = number of valid positions (including the new token). */
int cbx_decode_attn_f32(const float* q, const float* kc, const float* vc, float* o, const int* ctx_lens,
                        int rows, int n_heads, long q_ld, long o_ld, long cache_row_stride, long cache_head_stride,
                        float scale, void* stream);

/* Fused per-token attention of the decode loop: HF apply_rotary_pos_emb on q,k of the fused qkv row (head_dim 64,
 * rotate_half form; cos_t == sin_t == NULL skips the rotation: GPT-2) + DynamicCache append at positions[row] + sdpa over
 * positions [0, positions[row]] (t3.py:378-384, 438-446).
 * o_packed: o is written in the packed operand layout of the o-projection GEMV (cbx_gemv_t.x_packed; o_ld ignored). */
int cbx_decode_attn_rope_f32(const float* qkv, const int* positions, const float* cos_t, const float* sin_t, float* kc,
                             float* vc, float* o, int rows, int n_heads, long ld_qkv, long o_ld, int o_packed,
                             long cache_row_stride, long cache_head_stride, float scale, void* stream);
/* ABI v10: the same op with everything it depends on IN the call -- the form the engines use (no process-wide state: two engines, two streams
 * or a hipGraph captured earlier never see each other's geometry or share a workspace).
 *   unroll   : key rows in flight per 16-lane group and step: 0 (= 4), 4, 8 or 16.
 *   pipeline : bit 0 = software-pipelined K / V stream (the rows of the next step are requested before the current step is multiplied; two
 *              register sets; 4 or 8 rows per step); bit 1 = non-temporal K / V loads (4 rows per step); bit 2 = speculative first step
 *              (positions 0 .. 63 of every (row, head) are requested before positions[row] has arrived; needs cache_head_stride >= 64 * 64).
 *              Every combination gives the results of pipeline = 0 bit for bit (hardware test: tests/test_zz_abi_v9_gpu.py).
 *   split_ws / split_cnt / split_pairs : CALLER-OWNED workspace of the split-context form -- 66 * 8 floats per (row, head) and one int per
 *              (row, head), zeroed once by the caller, re-armed by every launch -- or NULL.  With rows * n_heads < 128 <= split_pairs the
 *              context of a (row, head) that is >= split_min (0 = 512) positions long is walked by up to 8 workgroups, merged in split order
 *              (deterministic).  One workspace serves launches that are ordered on one stream; concurrent launches need their own. */
typedef struct cbx_decode_attn_t {
    const float* qkv; const int* positions; const float *cos_t, *sin_t;
    float *kc, *vc, *o;
    int rows, n_heads; long ld_qkv, o_ld; int o_packed;
    long cache_row_stride, cache_head_stride; float scale;
    int unroll, pipeline, split_min;
    float* split_ws; int* split_cnt; long split_pairs;
    /* ABI v11: qkv_nparts = 2 .. 4: `qkv` holds that many UN-normalised split-K partial sums of the fused q/k/v row (cbx_gemv_t.col_tiles with
     * ksplit > 1), qkv_part_stride floats apart; the kernel adds them in fixed order and multiplies by rstd[row] = rsqrt(sum_p qkv_ssq[p * 16 * ceil(rows / 16) + row]
     * / rms_dim + rms_eps) (LlamaRMSNorm of the projection's input, folded through the contraction); rows <= 32.  0 / 1: qkv is the finished row. */
    int qkv_nparts; long qkv_part_stride; const float* qkv_ssq; int rms_dim; float rms_eps;
} cbx_decode_attn_t;
int cbx_decode_attn_rope(const cbx_decode_attn_t* p, void* stream);

/* ---- few-row decode (ABI v14): 1 .. 4 activation rows, weights in the checkpoint's row-major layout ----
 * cbx_gemv_row_f32:  out[m][n] = act( x'[m] . W[n][:] + bias[n] ) + res[m][n],  m < M <= 4, n < N, where the operand x' is
 *     x                                   (ln_w == NULL, parts == NULL),
 *     LayerNorm(x) * ln_w + ln_b          (ln_w, ln_b; eps; two-pass variance: F.layer_norm), or
 *     the attention output of the row     (parts: the n_parts split-context records per head that cbx_decode_attn_parts left, merged in
 *                                          slice order; K == 64 n_heads; x unused).
 * A wave owns rows_per_wave (0 = automatic: ~1024 waves) output columns over the whole of K and requests all of its weights up front: no LDS
 * reduction, no partial images.  K in {256, 768, 1024, 3072, 4096}; W [N][ldw] fp32, 16-byte aligned; res may alias out.
 * Replaces HF Conv1D / nn.Linear at q_len == 1 + GPT2Block ln_1 / ln_2 / ln_f inside T3.inference_turbo's loop (models/t3/t3.py:435-460) for
 * batches of at most 4 rows (the engines use it up to 2: beyond, the 16-row MFMA tile of cbx_gemv_f32 is faster). */
#define CBX_ATTN_PART_REC 68 /* floats per (row, head, slice) record: {running max, sum, -, -, 64 numerators} */
typedef struct cbx_gemv_row_t {
    const float* x; const float* W; const float* bias; const float* res; float* out;
    const float *ln_w, *ln_b; float eps;
    const float* parts; int n_parts, n_heads;
    int N, K; long ldw;
    int act;            /* CBX_ACT_* after the bias */
    int rows_per_wave;  /* 0 = automatic; 1, 2, 3, 4, 8 (K >= 3072 or parts: 1, 2) */
    int M;              /* activation rows, 1 .. 4 (0 = 1) */
    long ldx, ldo, ldr; /* M > 1: floats between consecutive rows of x, out, res */
    long parts_row_stride; /* M > 1: floats between the records of consecutive rows (n_heads * n_parts * CBX_ATTN_PART_REC when dense) */
} cbx_gemv_row_t;
int cbx_gemv_row_f32(const cbx_gemv_row_t* p, void* stream);
/* Decode attention of ONE new token per row over a small (row, head) grid, split over n_splits workgroups per (row, head) by 16-position
 * chunks (chunk c belongs to slice c % n_splits -- independent of the context length, so the cache stream starts before positions[] has
 * arrived).  Appends the token's k / v (RoPE'd when cos_t / sin_t are given; GPT-2: NULL) to the caches at positions[row] and leaves
 * parts[((row * n_heads + head) * n_splits + slice) * CBX_ATTN_PART_REC] for the consumer to merge (cbx_gemv_row_t.parts): no ticket, no
 * fence, no last-arriver.  chunks = 16-position chunks in flight per workgroup (2, 4 (= 0) or 8).  The caches hold >= max_ctx positions
 * behind every (row, head).  Replaces the q_len == 1 attention of HF GPT2Attention / LlamaAttention (t3.py:435-460 via sdpa). */
typedef struct cbx_attn_parts_t {
    const float* qkv; const int* positions; const float *cos_t, *sin_t;
    float *kc, *vc, *parts;
    int rows, n_heads, n_splits, chunks, max_ctx;
    long ld_qkv, cache_row_stride, cache_head_stride;
    float scale;
} cbx_attn_parts_t;
int cbx_decode_attn_parts(const cbx_attn_parts_t* p, void* stream);
/* tuning knob: tile shape of the split-bf16 GEMM (0 = automatic; 64, 12864, 128, 1282) */
int cbx_set_split_tile(int t);
/* TEST HOOKS of the positional cbx_decode_attn_rope_f32 (process-wide; the engines pass cbx_decode_attn_t instead): unroll / pipeline /
 * split_min as the fields above, and the workspace it splits through, registered for the calling
 * thread's current device (single-stream use only). */
int cbx_set_decode_attn_unroll(int u);
int cbx_set_decode_attn_pipeline(int on);
int cbx_set_decode_attn_workspace(float* ws, int* zeroed_counters, long max_pairs);
int cbx_set_decode_attn_split_min(int min_ctx);

/* Row softmax over materialised scores with optional relative-position term and key mask
 * (RelPositionMultiHeadedAttention.forward, transformer/attention.py:249-330):
 *   p[z][i][j] = softmax_j( scale*(ac[z][i][j] + bd[z][i][T-1-i+j]) ), keys j >= key_lens[z1] -> 0. */
int cbx_softmax_relpos_f32(const float* ac, const float* bd, float* p, const int* key_lens, int nz1, int nz2,
                           int Tq, int Tk, long ld_ac, long ld_bd, long ld_p, long zs_ac, long zs_bd, long zs_p,
                           float scale, void* stream);

/* The same attention WITHOUT materialised scores (flash form, exact fp32 MFMA; written after the GPU budget of round 3 was spent: verified on
 * the SIMT emulator against the materialised path, not yet timed):
 *   o[z][i][h] = sum_j softmax_j( scale*(qu[z][i][h] . k[z][j][h] + qv[z][i][h] . pp[T-1-i+j][h]) ) v[z][j][h],  keys j >= key_lens[z] masked.
 * qu = q + pos_bias_u, qv = q + pos_bias_v, k, v: [z][token][head][64] views that share one batch stride q_sb and token stride q_st (the
 * fused q | q | k | v projection); pp = linear_pos(pos_emb): (2T-1) rows of n_heads*64, row stride pp_st; o: [z][token][head][64].
 * Memory O(T) instead of 16 T^2 floats per head; the position term costs as many MFMAs as q k^T (each 32-row block of pp (q+v)^T serves
 * two key blocks).  Replaces RelPositionMultiHeadedAttention.forward (transformer/attention.py:249-330) for long utterances (60 s VC). */
int cbx_flash_relpos_f32(const float* qu, const float* qv, const float* k, const float* v, const float* pp, float* o, const int* key_lens,
                         int nz1, int n_heads, int T, long q_sb, long q_st, long pp_st, long o_sb, long o_st, float scale, void* stream);

/* ---- elementwise / glue ---- */
/* y[r][c] = act(x[r][c]) (per-column param for snake), 2-D strided: the activations that cannot ride a GEMM / LayerNorm epilogue
 * (Mish of the ResNet time MLPs, matcha/decoder.py:49,58; Snake at a ResBlock entry, hifigan.py:34-60,146-150). */
int cbx_act_f32(const float* x, float* y, const float* param, long rows, int C, long ldx, long ldy, int act,
                float slope, void* stream);
/* generic 2-D strided copy / scale-add: y = a*x + b*y (skip-connection concat of the CFM up block, decoder.py:294,316-317; conformer
 * macaron residuals, transformer/encoder_layer.py:193-229) */
int cbx_axpby_f32(const float* x, float* y, long rows, int C, long ldx, long ldy, float a, float b, void* stream);
/* out[r][:] = table[ids[r]][:] * scale [+ table2[ids2[r]][:]]   (nn.Embedding gathers: speech_emb + LearnedPositionEmbeddings, t3.py:116-119,
 * 370-371; flow.input_embedding, flow.py:106,166; negative ids give zeros).
 * flags bit 1 (value 2): out is the packed operand image of a decode GEMV (cbx_gemv_t.x_packed, K = C % 32 == 0; ld_out ignored;
 * rows of the last 16-row tile that are not written keep their previous contents). */
int cbx_embed_f32(const long long* ids, const float* table, const float* table2, const int* ids2, float* out,
                  long rows, int C, long ld_out, float scale, int flags, void* stream);
/* RoPE (HF apply_rotary_pos_emb, rotate_half form, as called by LlamaAttention in T3's prefill, t3.py:326-333) on q,k rows of a fused
 * qkv buffer + KV-cache append.
 * positions[r] gives the absolute position of row r; cos/sin tables are [max_pos][64] (cat(freqs,freqs)). */
int cbx_rope_kv_f32(float* qkv, const int* positions, const float* cos_t, const float* sin_t, float* kc, float* vc,
                    const int* cache_rows, long n_rows, int n_heads, long ld_qkv, long cache_row_stride,
                    long cache_head_stride, void* stream);
/* CFM Euler + CFG update (flow_matching.py:125-141): x += dt*((1+w)*v[b] - w*v[B+b]) written to both row sets. */
int cbx_cfm_euler_f32(float* xin, const float* v, int B, long T, int C, long ld_x, long ld_v, long xs_b, long vs_b,
                      float dt, float w, int cfg, void* stream);

/* ---- T3 sampler (t3.py:339-368 + HF logits processors): one workgroup per utterance ---- */
#define CBX_SAMPLER_NPARAMS 8
typedef struct cbx_sampler_t {
    const float* logits;       /* [2*B][ld] rows b (cond) and B+b (uncond) when cfg, else [B][ld] */
    long ld; int V; int B; int cfg;
    float cfg_weight, temperature, min_p, top_p, rep_penalty;
    int top_k;                 /* 0 = off */
    int order;                 /* 0: T3.inference (penalty,temperature,min-p,top-p); 1: inference_turbo
                                  (temperature,top-k,top-p,penalty)  (t3.py:339-356 vs 396-404) */
    int ban_token;             /* probability forced to 0 (EOS ban for fixed-length runs) or -1 */
    int eos_token;
    int ban_from;              /* ids >= ban_from (EOS included) get probability 0; 0 = off.  Synthetic random-weight
                                  fixed-length runs use 6561 so that only valid S3 tokens are emitted.  Bans act AFTER the
                                  processors (like zeroing softmax entries); if no probability mass is left (the arg-max is
                                  banned and min-p / top-k pruned the rest) the result is the allowed id with the largest
                                  CFG-combined raw logit, lowest id on ties */
    unsigned char* seen;       /* [B][V] 0/1 map of generated ids (repetition penalty) */
    const float* uniforms;     /* [B][max_steps] U[0,1): the injected RNG of torch.multinomial */
    int max_steps;
    int* step;                 /* [B] step index, incremented */
    long long* out_tokens;     /* [B][max_steps] */
    int* done;                 /* [B] set when EOS sampled; finished utterances are skipped */
    int* n_generated;          /* [B] */
    long long* next_ids;       /* [rows] id to embed at the next decode step (both CFG rows), or NULL */
    int* next_pos_ids;         /* [rows] learned speech-position index of the next input (= step+1), or NULL */
    int* positions;            /* [rows] RoPE / cache position of the next input, incremented, or NULL */
    int* ctx_lens;             /* [rows] context length of the next decode step, incremented, or NULL */
    const float* dev_params;   /* ABI v4: NULL, or [B][CBX_SAMPLER_NPARAMS] floats in DEVICE memory that override, per utterance,
                                  {cfg_weight, temperature, min_p, top_p, rep_penalty, top_k, ban_token, ban_from}: a new request
                                  with other settings then needs no re-capture of the decode hipGraph */
} cbx_sampler_t;
int cbx_t3_sample(const cbx_sampler_t* p, void* stream);

/* ---- stage-level entry point: ONE token step of T3.inference's loop for every row (t3.py:338-386) ----
 * Sequences the kernel-level entry points above on `stream` (embedding gather, n_layers x 5 launches, head, sampler): no allocation,
 * no synchronisation, hipGraph-capturable.  rows <= 32 (the packed-operand path: one or two 16-row tiles; 17 .. 32 rows need fp32 images and qkv_ct, head_ct <= 3); all weights are cbx_pack_gemv_weight_f32 images
 * (wgu with swiglu = 1), all buffers caller-owned device memory. */
typedef struct cbx_t3_layer_t {
    const float *ln1, *ln2;               /* [dim] RMSNorm weights (input_layernorm, post_attention_layernorm) */
    const float *wqkv, *wo, *wgu, *wd;    /* packed images: [3*dim][dim], [dim][dim], gate|up [2*ffn][dim], [dim][ffn] */
} cbx_t3_layer_t;
typedef struct cbx_t3_step_t {
    int n_layers, rows, dim, ffn, n_heads, vocab;
    int o_nw, gu_nw, d_nw, d_ksplit;      /* launch geometry (T3Engine.tune): 8 / 8 / 16 / 2; d_ksplit = 1 (ABI v9): the down projection adds
                                             the residual itself (no partial images, no fold in the next q/k/v GEMV) */
    int half_tiles, w_bf16;               /* cbx_gemv_t.half_tile of the wo / wd images (0, 1 = 8, 4); 1: all weight images are bf16 */
    float eps, attn_scale;
    const cbx_t3_layer_t* layers;         /* HOST array [n_layers] */
    const float *speech_emb, *speech_pos, *final_norm, *head; /* embeddings [V][dim], [P][dim]; tfmr.norm; packed head [ceil16(vocab)][dim] */
    const float *cos_t, *sin_t;           /* RoPE tables [max_pos][64] */
    float *kc, *vc;                       /* KV cache [n_layers][rows][n_heads][max_ctx][64] */
    long kv_row_stride, kv_head_stride;   /* floats: n_heads*max_ctx*64, max_ctx*64 */
    const long long* next_ids;            /* [rows] token to embed (written by the sampler) */
    const int *next_pos_ids, *positions;  /* [rows] learned position index; RoPE / cache position */
    float *x_a, *x_b;                     /* packed residual images [ceil16(rows)][dim] (ping-pong), pad rows zero */
    float *qkv, *att, *g, *pd;            /* [rows][3*dim]; packed [ceil16(rows)][dim]; packed [..][ffn]; partial images [d_ksplit][ceil16(rows)][dim] */
    float* logits;                        /* [rows][ld_logits] */
    long ld_logits;
    const cbx_sampler_t* sampler;         /* sampler descriptor (host struct) run at the end of the step, or NULL */
    int qkv_tile;                         /* ABI v9: cbx_gemv_t.half_tile of the wqkv images (0 or 12) */
    /* ABI v10: the rest of the step's geometry (was process-wide): cbx_decode_attn_t.unroll / pipeline / split_min / split_* of every attention
     * launch, cbx_gemv_t.flags of every GEMV launch */
    int da_unroll, da_pipeline, da_split_min, gemv_flags;
    float* da_ws; int* da_cnt; long da_pairs;
    /* ABI v11: qkv_ksplit = 2 or 4 (dim % (256 qkv_ksplit) == 0; with qkv_ct = column tiles per workgroup, qkv_tile = 0): the q/k/v projection in the split-K column-tile form --
     * qkv then holds [qkv_ksplit][rows][3*dim] partial sums and qkv_ssq [qkv_ksplit][16 * ceil(rows / 16)] sums of squares, which the attention launch folds;
     * head_ct > 0: the speech head in the column-tile form (ksplit 1).  0 = the one-tile forms. */
    int qkv_ksplit, qkv_ct, head_ct;
    float* qkv_ssq;
} cbx_t3_step_t;
int cbx_t3_decode_step(const cbx_t3_step_t* d, void* stream);

/* ---- handle-level entry points: the TOKEN LOOP of T3.inference in C (t3.py:338-386 incl. its EOS test `:366`; SURVEY.md 8b "cbx_t3_generate") ----
 * cbx_t3_loop_create deep-copies the step descriptor (its host arrays: layers, sampler) and captures ONE cbx_t3_decode_step in a hipGraph (thread-local
 * capture on a stream of the library's own -- `stream` may be the legacy default stream --; nothing is allocated on the device); cbx_t3_loop_run replays it up to n_steps times on `stream`.  poll_every > 0: after every
 * poll_every steps the per-utterance done flags (cbx_sampler_t.done) are fetched and the loop ends early once every utterance has sampled its EOS --
 * the reference's per-token host sync, amortised; poll_every = 0: all n_steps are enqueued without any synchronisation (asynchronous use).
 * *steps_run = steps enqueued.  The caller owns every device buffer of the descriptor and keeps it alive until cbx_t3_loop_destroy.  One handle per
 * (descriptor, stream of launches); not thread-safe.  With cbx_t3_prefill a C host runs the whole device side of T3.inference without Python. */
typedef struct cbx_t3_loop cbx_t3_loop_t;
int cbx_t3_loop_create(const cbx_t3_step_t* step, void* stream, cbx_t3_loop_t** out);
int cbx_t3_loop_run(cbx_t3_loop_t* h, int n_steps, int poll_every, void* stream, int* steps_run);
int cbx_t3_loop_destroy(cbx_t3_loop_t* h);

/* ---- stage-level entry point: the PREFILL of T3.inference for every row (t3.py:303-335 -> t3_hf_backend.py:71-111: HF LlamaModel over the S prompt
 * positions, KV cache filled) ----
 * x (rows * S, dim) holds the input embeddings (prepare_input_embeds + the second BOS, t3.py:102-130, 305-313; rows right-padded to S) and returns the last
 * layer's residual stream; the caller applies tfmr.norm + speech_head to the positions it needs (cbx_layernorm_f32 + cbx_gemm_f32).  `layers`: the
 * cbx_t3_layer_t of the decode step with ROW-MAJOR weights (torch Linear layout; wgu = the [32 gate | 32 up]-interleaved image, cbx_gemm_t.swiglu).
 * positions / cache_rows [rows * S]: RoPE position and KV-cache row of every prompt position.  precision: cbx_gemm_t.precision of the plain projections and
 * of the attention (0 / 1 = exact fp32 MFMA, the parity path; 6 = bf16x6).  Sequences kernel-level entry points only: no allocation, no synchronisation,
 * hipGraph-capturable; results bit-identical to issuing the same launches one by one. */
typedef struct cbx_t3_prefill_t {
    int n_layers, rows, S, dim, ffn, n_heads, precision;
    float eps, attn_scale;
    const cbx_t3_layer_t* layers;         /* HOST array [n_layers], row-major weights */
    float* x;                             /* [rows * S][dim] in / out */
    float *h, *qkv, *att, *g;             /* workspaces: [rows * S][dim], [..][3 * dim], [..][dim], [..][ffn] */
    const int *positions, *cache_rows;    /* [rows * S] */
    const float *cos_t, *sin_t;           /* RoPE tables [max_pos][64] */
    float *kc, *vc;                       /* KV cache [n_layers][rows][n_heads][max_ctx][64] */
    long kv_layer_stride, kv_row_stride, kv_head_stride;  /* floats */
} cbx_t3_prefill_t;
int cbx_t3_prefill(const cbx_t3_prefill_t* d, void* stream);

/* ---- ABI v16: the PREFILL of T3.inference_turbo for every row (t3.py:392-468 -> HF GPT2Model over [speaker | prompt tokens | text | start-speech], absolute
 * position embeddings already added to x; KV cache filled) ----
 * x (rows * S, dim) in / out as cbx_t3_prefill_t; per layer ln_1 -> c_attn (+ bias) -> K / V append at positions[] of cache row cache_rows[] -> causal attention ->
 * attention c_proj (+ bias + residual) -> ln_2 -> c_fc (+ bias + gelu_new) -> mlp c_proj (+ bias + residual); weights ROW-MAJOR (N, K) (the checkpoint's Conv1D
 * weights transposed), ffn = 4 * dim.  prefix > 0: the first `prefix` positions of every row are ALREADY in the KV cache (the speaker + prompt-token positions of a
 * voice see only themselves under the causal mask and carry absolute positions: computed once per voice); x then holds the remaining S positions of every row,
 * positions[] start at `prefix`, and the attention reads keys / values [prefix | S] from the cache (cbx_flash_attn_kv_f32).  Sequences kernel-level entry points
 * only (exact fp32): no allocation, no synchronisation; results bit-identical to issuing the same launches one by one. */
typedef struct cbx_gpt2_layer_t {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *wqkv, *bqkv, *wo, *bo, *wfc, *bfc, *wpr, *bpr;
} cbx_gpt2_layer_t;
typedef struct cbx_gpt2_prefill_t {
    int n_layers, rows, S, prefix, dim, n_heads;
    float eps, attn_scale;
    const cbx_gpt2_layer_t* layers;       /* HOST array [n_layers] */
    float* x;                             /* [rows * S][dim] in / out */
    float *h, *qkv, *att, *g;             /* workspaces: [rows * S][dim], [..][3 * dim], [..][dim], [..][4 * dim] */
    const int *positions, *cache_rows;    /* [rows * S] */
    float *kc, *vc;                       /* KV cache [n_layers][rows][n_heads][max_ctx][64] */
    long kv_layer_stride, kv_row_stride, kv_head_stride;  /* floats */
} cbx_gpt2_prefill_t;
int cbx_gpt2_prefill(const cbx_gpt2_prefill_t* d, void* stream);

/* ---- the prefill INPUT of a ragged batch in one launch (added after ABI v16 without a version step) ----
 * Replaces the per-utterance host loop over cbx_embed_f32 + slice copies that builds the (rows, S - pos0, dim) prefill input of T3.inference (prepare_input_embeds +
 * the second BOS, t3.py:102-130,305-313: [conditioning | text_emb[id] (x 0 on the CFG-unconditional row) + text_pos[i] | 2 x (speech_emb[bos] + speech_pos[0])]) and of
 * T3.inference_turbo (t3.py:407-423: [conditioning | text_emb[id] + wpe[p] | speech_emb[bos] + wpe[p]], absolute positions p), zeros in the padding, and writes the
 * index vectors the prefill takes: positions[r * Sx + s] = pos0 + s, cache_rows[r * Sx + s] = r, last[r] = flat index of row r's last prompt position (Sx = S - pos0).
 * Utterance b = r % B; meta[b] = {offset of its ids in `ids`, text length, conditioning slot (-1: none), conditioning length P_b}.  Positions below P_b are copied from
 * cond[slot] (P_b x dim floats) -- or, with pos0 > 0, are not part of x at all (they are in the KV cache: cbx_kv_prefix_paste_f32; then every P_b == pos0).
 * One multiply-add per element in cbx_embed_f32's order: bit-identical to the loop it replaces.  The caller guarantees 0 <= ids < text vocabulary, offsets inside
 * `ids`, slots inside `cond` and P_b + text length + n_bos <= S. */
typedef struct cbx_prefill_embed_t {
    int B, cfg;                           /* utterances; cfg = 1: rows = 2 B, rows B .. 2 B - 1 are the unconditional rows (text embeddings x 0), else rows = B */
    int n_bos, abs_pos;                   /* BOS positions behind the text (Llama 2, GPT-2 1); 1: both position tables are indexed by the absolute position (wpe) */
    int S, pos0, dim;                     /* common (padded) prompt length; first absolute position held in x (0, or the cached prefix length); model width */
    long long bos_id;                     /* start-of-speech id (row of speech_emb) */
    const int* meta;                      /* [B][4] */
    const int* ids;                       /* text ids of all utterances, back to back */
    const float* cond;                    /* [slots][cond_stride] conditioning embeddings, or NULL */
    long cond_stride;                     /* floats */
    const float *text_emb, *text_pos, *speech_emb, *speech_pos;   /* [.][dim] tables (GPT-2: text_pos == speech_pos == wpe) */
    float* x;                             /* [rows][S - pos0][dim] out */
    int *positions, *cache_rows;          /* [rows * (S - pos0)] out */
    long long* last;                      /* [rows] out */
} cbx_prefill_embed_t;
int cbx_prefill_embed(const cbx_prefill_embed_t* d, void* stream);
/* kc / vc[l][r][h][0 .. P - 1][:] = prefix_k / prefix_v[voice_of_row[r]][l][h][0 .. P - 1][:]: the cached conditioning prefixes of a batch that mixes voices, pasted in one
 * launch (replaces one broadcast copy_ pair per voice; the K / V that LlamaModel / GPT2Model would recompute for the conditioning positions of every row, t3.py:326-333,
 * 425-432).  table (device): n_voices pointers to K prefixes [n_layers][n_heads][P][64] contiguous, n_voices pointers to V prefixes, then voice_of_row[rows] (each in
 * [0, n_voices)).  Pure copy. */
int cbx_kv_prefix_paste_f32(const long long* table, int n_voices, float* kc, float* vc, int n_layers, int rows, int n_heads, int P,
                            long kv_layer_stride, long kv_row_stride, long kv_head_stride, void* stream);

/* ---- ONE token step of T3.inference_turbo's loop for every row (t3.py:392-468: the q_len == 1 HF GPT2Model forward over the KV cache, ln_f, speech_head, the
 * Temperature -> TopK -> TopP -> RepetitionPenalty processors and the multinomial draw) ----
 * Issues exactly the launches of chatterbox_amd/t3_turbo.py's token step, with the same arguments (bit-identical tokens and logits), and adds no arithmetic:
 *   row_path = 1 (rows <= 4; the engine uses it for 1 .. 2 rows: T3TurboEngine._forward_decode_row): cbx_embed_f32, n_layers x [cbx_gemv_row_f32 (ln_1 + c_attn),
 *     cbx_decode_attn_parts, cbx_gemv_row_f32 (attention merge + c_proj + residual), cbx_gemv_row_f32 (ln_2 + c_fc + gelu_new), cbx_gemv_row_f32 (mlp c_proj +
 *     residual)], cbx_gemv_row_f32 (ln_f + speech head), cbx_t3_sample; weights row-major (cbx_gpt2_layer_t);
 *   row_path = 0 (rows <= 16: _forward_decode_v2): cbx_embed_f32 (packed), n_layers x [cbx_gemv_f32 (LayerNorm folded into c_attn, the previous layer's split-K
 *     partial images summed into the operand), cbx_decode_attn_rope, cbx_gemv_f32 (c_proj + bias + residual), cbx_gemv_f32 (LayerNorm folded into c_fc + gelu_new),
 *     cbx_gemv_f32 (mlp c_proj: d_ksplit partial images, or + residual in place when d_ksplit == 1)], cbx_gemv_f32 (ln_f folded into the head), cbx_t3_sample;
 *     weights are cbx_pack_gemv_weight_f32 images (cbx_gpt2_packed_layer_t).
 * More than 16 rows (the engine's 7-launch form) are refused.  No allocation, no synchronisation, hipGraph-capturable. */
typedef struct cbx_gpt2_packed_layer_t {
    const float *wqkv, *wo, *wfc, *wpr;            /* packed images: c_attn (qkv_tile columns per tile), attention c_proj (od_tile), c_fc (16), mlp c_proj (od_tile) */
    const float *qkv_cw, *qkv_cb, *fc_cw, *fc_cb;  /* LayerNorm-fold constants of c_attn / c_fc (cbx_gemv_t.ln_cw / ln_cb) */
} cbx_gpt2_packed_layer_t;
typedef struct cbx_gpt2_step_t {
    int n_layers, rows, dim, n_heads, vocab;
    int row_path;                         /* 1: the few-row kernels, 0: the packed 16-row-tile path */
    float eps, attn_scale;
    const cbx_gpt2_layer_t* layers;       /* HOST array [n_layers]: LayerNorm weights / biases, projection biases, row-major weights (row path) */
    const cbx_gpt2_packed_layer_t* packed;/* HOST array [n_layers] (packed path) or NULL */
    const float *speech_emb, *wpe;        /* [V][dim], [n_positions][dim]: the input is speech_emb[next_ids] + wpe[positions] */
    const float *lnf_w, *lnf_b, *head, *head_b;   /* ln_f, row-major speech head [vocab][dim] + bias (row path; head_b unused on the packed path) */
    const float *head_pk, *head_cw, *head_cb;     /* packed path: head image, ln_f-fold constants */
    float *kc, *vc;                       /* KV cache [n_layers][rows][n_heads][max_ctx][64] */
    long kv_layer_stride, kv_row_stride, kv_head_stride;  /* floats */
    int max_ctx;
    const long long* next_ids;            /* [rows] (written by the sampler) */
    const int* positions;                 /* [rows] cache / wpe position of the token to embed */
    float *x, *qkv, *g, *parts;           /* x [rows][dim], qkv [rows][3 dim] (both paths); row path: g [rows][4 dim], parts [rows][n_heads][n_splits][CBX_ATTN_PART_REC] */
    int n_splits, chunks;                 /* row path: cbx_attn_parts_t.n_splits / chunks */
    float *x_a, *x_b, *att, *g_pk, *pd;   /* packed path: residual images [ceil16(rows)][dim] (ping-pong), [..][dim], [..][4 dim], partial images [d_ksplit][..][dim] */
    int qkv_tile, od_tile;                /* cbx_gemv_t.half_tile of the c_attn resp. both c_proj images (0 = 16 columns) */
    int d_ksplit, o_nw, d_nw, head_ct, gemv_flags;  /* mlp c_proj split-K factor (1, 2, 4) and waves, attention c_proj waves, head column tiles, cbx_gemv_t.flags */
    int da_unroll, da_pipeline, da_split_min;       /* cbx_decode_attn_t geometry + split-context workspace of the attention launches */
    float* da_ws; int* da_cnt; long da_pairs;
    float* logits;                        /* [rows][ld_logits] */
    long ld_logits;
    const cbx_sampler_t* sampler;         /* sampler descriptor (host struct, order 1, cfg 0) run at the end of the step, or NULL */
} cbx_gpt2_step_t;
int cbx_gpt2_decode_step(const cbx_gpt2_step_t* d, void* stream);
/* The TOKEN LOOP of T3.inference_turbo in C (t3.py:392-468 incl. its EOS test): the contract of cbx_t3_loop_* -- deep copy of the descriptor (layers, packed,
 * sampler), ONE cbx_gpt2_decode_step captured in a hipGraph on a stream of the library's own (one linear chain of launches), replayed up to n_steps times on
 * `stream`; poll_every > 0 fetches the done flags every poll_every steps and ends early once every row has sampled its EOS, 0 enqueues all n_steps without
 * synchronising; *steps_run = steps enqueued. */
typedef struct cbx_gpt2_loop cbx_gpt2_loop_t;
int cbx_gpt2_loop_create(const cbx_gpt2_step_t* step, void* stream, cbx_gpt2_loop_t** out);
int cbx_gpt2_loop_run(cbx_gpt2_loop_t* h, int n_steps, int poll_every, void* stream, int* steps_run);
int cbx_gpt2_loop_destroy(cbx_gpt2_loop_t* h);

/* ---- stage-level entry points of the S3Gen flow decoder and of the HiFT vocoder (ABI v12) ----
 * A plane-format operand (see PLANE-FORMAT operands above) as the stage descriptors carry it: base of the h plane with any column offset applied, row
 * stride and plane offset in halves. */
typedef struct cbx_planes_t { void* p; long ld, lo; } cbx_planes_t;

/* BasicTransformerBlock of the CFM estimator (matcha/transformer.py:243-316): norm1 -> to_q | to_k | to_v -> attention -> to_out + residual -> norm3 ->
 * FeedForward (GELU) + residual.  wqkv: planes of the (1536, 256) row block [Wq; Wk; Wv]; wo (256, 512); w1 (1024, 256); w2 (256, 1024). */
typedef struct cbx_cfm_tblock_t {
    const float *n1_w, *n1_b, *n3_w, *n3_b, *bo, *b1, *b2;
    cbx_planes_t wqkv, wo, w1, w2;
} cbx_cfm_tblock_t;
/* One down / mid / up stage of ConditionalDecoder (decoder.py:243-333): CausalResnetBlock1D (c1, n1 + Mish + time bias, c2, n2 + Mish, 1x1 res_conv), n_tb
 * transformer blocks and -- down and up stage only -- the trailing CausalConv1d (tail.p == NULL otherwise).  Conv weights: planes of the tap-major
 * (256, taps * cin) image. */
typedef struct cbx_cfm_stage_t {
    cbx_planes_t c1, c2, res, tail;
    const float *c1_b, *n1_w, *n1_b, *c2_b, *n2_w, *n2_b, *res_b, *tail_b;
    int cin, n_tb;
    const cbx_cfm_tblock_t* tb;           /* HOST array [n_tb] */
} cbx_cfm_stage_t;
/* CausalConditionalCFM.solve_euler (models/s3gen/flow_matching.py:78-145, 196-233; meanflow: 196-233 with cfg = 0) around ConditionalDecoder.forward on
 * plane-format operands (the f16x3 numerics, cbx_gemm_t.precision 16): n_steps x [x columns of xinP re-split (steps > 0), estimator -> v, Euler (+ CFG) update
 * of xin].  xin (rows, T, 320) fp32 = [x | mu | spk | cond] per position (rows = 2 B with CFG: the second B rows hold [x | 0 | 0 | 0]); xinP its plane image,
 * split by the caller before the call; on return xin[:B, :, :80] is the mel.  tbias [n_steps][n_stages][256]: every ResNet's time-MLP output per step (a
 * function of the schedule only; the caller computes it once).  dt: HOST array [n_steps] of t_span[k + 1] - t_span[k].  lens [rows]: valid positions per row.
 * Needs T even, rows * T > 32, (rows * T + 512) * 4096 < 2^31.  Sequences kernel-level entry points only (results bit-identical to issuing them one by one):
 * no allocation, no synchronisation, hipGraph-capturable. */
typedef struct cbx_cfm_t {
    int n_stages, rows, B, n_steps, cfg, fused_qkv, fused_ln;    /* fused_ln (ABI v13; the slot of v12's fused_mlp): 1 = norm3 from the attention
                                                                  * out-projection's epilogue (cbx_gemm_pl_t.ln_w), 2 = also the next block's norm1
                                                                  * from ff2's; 0 = LayerNorm launches of their own */
    int b_split;                          /* TWO CHAINS (in the alignment slot in front of T: size and every other offset unchanged, a zeroed descriptor is
                                           * the one-chain call).  0 < b_split < B: the batch is two independent half-batches of b_split and B - b_split
                                           * utterances, each CONTIGUOUS in the rows -- with CFG [cond h0 | uncond h0 | cond h1 | uncond h1], without
                                           * [h0 | h1] -- and on return the mel of utterance b is row b (b < b_split) resp. row (cfg ? 2 : 1) * b_split +
                                           * (b - b_split).  The first half is launched on `stream`, the second on a stream of the library's own (one per
                                           * device and priority, the caller's priority and co-resident attribute) between ONE fork and ONE join event:
                                           * after the call `stream` orders everything, as in the one-chain call.  Each half needs rows * T >= 64 of its
                                           * own (below it a half's LayerNorm launches would take another kernel than the whole batch's).  While
                                           * `stream` is capturing both halves are launched on it, one after the other (no fork: twice the launches of
                                           * the one-chain call at half the rows; a caller that wants the one-chain launches in a capture passes 0).
                                           * The side stream is shared by every caller stream of its device and priority: their second halves queue on
                                           * it in call order, and the library holds a lock of its own from the fork to the join of a call (the whole
                                           * enqueue, several thousand launches), so concurrent two-chain calls at one priority enqueue one after the
                                           * other.  The field occupies bytes that were padding up to now: a descriptor MUST be zero-initialised
                                           * (memset / `= {0}`) before it is filled. */
    long T;
    float cfg_rate;
    const float* dt;                      /* HOST [n_steps] */
    const cbx_cfm_stage_t* stages;        /* HOST [n_stages]: down, mid ..., up */
    cbx_planes_t fin_c, fin_proj;         /* final_block conv (256, 3 * 256), final_proj (80, 256) */
    const float *fin_c_b, *fin_n_w, *fin_n_b, *fin_proj_b;
    const float* tbias;
    const int* lens;
    float* xin;
    cbx_planes_t xinP;                    /* (rows * T, 320) */
    float *ra, *rb, *x, *v;               /* workspaces (rows, T, 256) x 3, estimator output (rows, T, 80) */
    cbx_planes_t aP, hP, qkP, attP, ffP, xP, yP, catP;   /* plane workspaces over rows * T rows: 256, 256, 1024, 512, 1024, 256, 256, 512 columns */
    cbx_planes_t vtP;                     /* V^T: (rows * 512) rows x (T rounded up to 8) columns, the padding zero */
    int gemm_tile, attn_version;          /* ABI v13: cbx_gemm_pl_t.tile of every plane GEMM / version of every attention launch (0, 0 = the defaults;
                                           * CBX_PL_TILE_CORESIDENT, 5 = the co-resident forms of the throughput schedule) */
} cbx_cfm_t;
int cbx_cfm_solve(const cbx_cfm_t* d, void* stream);

/* ConformerEncoderLayer of the S3Gen token encoder (transformer/encoder_layer.py:160-236 with RelPositionMultiHeadedAttention, attention.py:249-330):
 * w4 / b4 = the fused projection [q + pos_bias_u | q + pos_bias_v | k | v] (2048, 512); wpos = linear_pos (512, 512, no bias). */
typedef struct cbx_conformer_t {
    const float *ln_mha_w, *ln_mha_b, *w4, *b4, *wpos, *wo, *bo, *ln_ff_w, *ln_ff_b, *w1, *b1, *w2, *b2;
} cbx_conformer_t;
/* UpsampleConformerEncoder.forward + encoder_proj (transformer/upsample_encoder.py:237-304, flow.py:161-169) for B rows of N tokens: input_embedding
 * gather (ids < 0 = padded position: zero vector), embed (Linear + LayerNorm * sqrt(512)), PreLookaheadLayer, n_enc conformer layers, Upsample1D (nearest x2
 * + conv k5, fused in the conv's address map), up_embed, n_up conformer layers over 2 N positions, after_norm, encoder_proj -> mu (B, 2 N, 80).  The rel-pos
 * attention runs in its flash form (cbx_flash_relpos_f32).  pe / pe2: EspnetRelPositionalEncoding tables of N resp. 2 N positions ((2 T - 1) x 512, row r <->
 * relative position T - 1 - r), constants of the length.  precision: cbx_gemm_t.precision of every Linear / conv.  Workspaces: x0, xa, y1, x2 (B N x 512);
 * xu, xb, h, att (B 2N x 512); q4, ff (B 2N x 2048); pp (4 N x 512).  Same contract as cbx_cfm_solve. */
typedef struct cbx_s3enc_t {
    int B, N, n_enc, n_up, precision;
    const long long* ids;                 /* [B * N] */
    const int *lens, *lens2;              /* [B]: valid tokens per row, twice that */
    const float *emb, *e_w, *e_b, *e_lnw, *e_lnb, *u_w, *u_b, *u_lnw, *u_lnb, *pl1_w, *pl1_b, *pl2_w, *pl2_b, *up_w, *up_b, *after_w, *after_b, *proj_w, *proj_b;
    const cbx_conformer_t *enc, *up_enc;  /* HOST arrays [n_enc], [n_up] */
    const float *pe, *pe2;
    float *x0, *xa, *y1, *x2, *xu, *xb, *h, *q4, *pp, *att, *ff;
    float* mu;
} cbx_s3enc_t;
int cbx_s3gen_encode(const cbx_s3enc_t* d, void* stream);

/* The front half of HiFTGenerator.inference (hifigan.py:462-469): ConvRNNF0Predictor (f0_predictor.py:52-55: 5 x Conv1d k3 + ELU, Linear, abs; always exact
 * fp32 -- its output is integrated into a phase over ~10^5 samples) -> f0 (B, T), then f0_upsamp + SourceModuleHnNSF (hifigan.py:201-231, 267-283) with the
 * caller's initial phases (B, 9) and noise (B, 9, 480 T) -> s (B, 480 T).  buf0 / buf1: (B, T, 512) workspaces; cum: (B, 9, T) doubles.  lens: NULL or [B]. */
typedef struct cbx_hift_f0_t {
    int B;
    long T;
    const float* mel;                     /* (B, T, 80) */
    const int* lens;
    const float *f0_w[5], *f0_b[5], *cls_w, *cls_b, *src_w;
    float src_b;
    const float *phase, *noise;
    float *buf0, *buf1, *f0, *s;
    double* cum;
} cbx_hift_f0_t;
int cbx_hift_f0_source(const cbx_hift_f0_t* d, void* stream);
/* cbx_hift_f0_source for a WINDOW of a longer signal (hifigan.py:201-231, 467-472: the reference keeps the excitation continuous across chunks by pasting the
 * earlier chunk's source, `cache_source`; beyond it the phase has to continue too): cum_in = NULL or (B, 9) doubles, see cbx_hift_source_carry_f32.  NULL
 * or zeros: the bits of cbx_hift_f0_source.  d->cum of this call stays readable: the next window takes its carry from it. */
int cbx_hift_f0_source_carry(const cbx_hift_f0_t* d, const double* cum_in, void* stream);

/* ResBlock of HiFT (hifigan.py:118-161): three (Snake, dilated conv, Snake, conv, + x) rounds; conv weights tap-major (C, k * C), weight_norm folded */
typedef struct cbx_hift_resblock_t {
    const float *c1_w[3], *c1_b[3], *c2_w[3], *c2_b[3], *a1[3], *a2[3];
} cbx_hift_resblock_t;
/* HiFTGenerator.decode (hifigan.py:412-444) for B rows: STFT of the source s, conv_pre, 3 x [leaky ReLU, ConvTranspose1d (phase-packed 3-tap form, cbx_gemm_t),
 * + source_resblock(source_down(STFT)), mean of 3 ResBlocks], conv_post, iSTFT (+ S3Gen's trim_fade when fade).  mel (B, T, 80) channel-last, s (B, 480 T),
 * wav (B, 480 T).  lens: NULL or [5][B] = valid rows of {mel, stage 1, stage 2, stage 3 = STFT frames, source samples} = {n, 8 n, 40 n, 120 n + 1, 480 n}.
 * With lens, wav[b][m] for m >= 480 n is 0 and every sample below equals the B = 1 call on the cut row (cbx_hift_istft_rows_f32).
 * precision: cbx_gemm_t.precision of every conv.  Workspaces: spec, post (B, 120 T + 1, 32); x0 (B, T, 512); xs .. nxt[1]: (B, 120 T + 1, 64) floats each
 * (the widest stage; stages 1 and 2 use a prefix).  Same contract as cbx_cfm_solve. */
typedef struct cbx_hift_t {
    int B, precision, fade;
    long T;
    const float *mel, *s;
    float* wav;
    const int* lens;
    const float *conv_pre_w, *conv_pre_b, *ups_w[3], *ups_b[3], *src_down_w[3], *src_down_b[3], *conv_post_w, *conv_post_b;
    cbx_hift_resblock_t src_rb[3], rb[9];
    float *spec, *post, *x0, *xs, *t1, *xa, *xb, *an, *si, *sa, *acc, *a0, *nxt[2];
} cbx_hift_t;
int cbx_hift_decode(const cbx_hift_t* d, void* stream);

/* ---- HiFT source + (i)STFT (hifigan.py:201-231,267-283,396-410) ---- */
int cbx_hift_source_f32(const float* f0, const float* phase, const float* noise, const float* lin_w, float lin_b,
                        float* s, double* frame_cum, int B, int T, int up, float sr, void* stream);
/* SourceModuleHnNSF with a phase carry-in (hifigan.py:201-231, 467-472): cum_in = NULL or (B, 9) doubles, the cumulative cycles `cumsum(f0 (h + 1) / sr)` with
 * which the frame scan of (b, h) starts in place of 0.  Run over frames [w0, T) of a signal with cum_in = frame_cum[:, :, w0] of the full-length call and the
 * matching slices of f0 and noise, s is bit-identical to samples [up w0, up T) of the full-length source.  NULL or zeros: the bits of cbx_hift_source_f32. */
int cbx_hift_source_carry_f32(const float* f0, const float* phase, const float* noise, const float* lin_w, float lin_b,
                              float* s, double* frame_cum, const double* cum_in, int B, int T, int up, float sr, void* stream);
/* End of a round of chunked synthesis, one launch for B utterances (the schedule is this build's own; it extends the reference's one streaming hook, the
 * `cache_source` of hifigan.py:467-472).  wav (B, ld_wav): the round's waveform, wav[b][q] = absolute sample origin + q of utterance b.  emitted / end / avail
 * [B] ints, absolute samples: out[b][i] = sample emitted[b] + i for i < end[b] - emitted[b] (out (B, max_new)); the first min(tail_len[b], fade) of them are
 * tail_in[b][i] * (1 - ramp[i]) + new * ramp[i], rounded product by product as the torch expression is (no fma); tail_out[b][j] = sample end[b] + j for
 * j < min(avail[b], end[b] + fade) - end[b] (tail_in, tail_out (B, fade), distinct buffers; ramp [fade]).  A row with end == emitted == avail is left alone.
 * Positions outside the window read as 0 / are not written. */
int cbx_stream_emit_f32(const float* wav, long ld_wav, long origin, const int* emitted, const int* end, const int* avail, const float* tail_in,
                        const int* tail_len, const float* ramp, int fade, float* out, long max_new, float* tail_out, int B, void* stream);
/* sample_lens[b] (or NULL): per-row signal length; the centre-reflect padding mirrors at that row's own end */
int cbx_hift_stft_f32(const float* s, float* spec, const int* sample_lens, int B, long L, long ld_spec, void* stream);
/* x[b][frame][0..8] log-magnitude, [9..17] phase pre-sin (conv_post output); fade_n>0 applies S3Gen trim_fade. */
int cbx_hift_istft_f32(const float* x, float* wav, int B, long frames, long ldx, float clamp, int fade_n,
                       void* stream);
/* The same for a RAGGED batch (added after ABI v16 without a version step: a new function only; cbx_hift_istft_f32 is this call with frame_lens = NULL).
 * frame_lens: NULL (every row has `frames` frames) or [B] ints in device memory.  Row b owns frames [0, frame_lens[b]) and samples [0, 4 (frame_lens[b] - 1)):
 *   - an owned sample overlap-adds, in the signal and in the window envelope, the frames of its own row only; frames at or beyond frame_lens[b] and columns
 *     18 .. ldx - 1 are never read, whatever they hold.  It therefore has the bits of a B = 1 call on the row cut to frame_lens[b] frames -- torch.istft of the
 *     cut row -- up to and including its last three samples, which a neighbour frame beyond the row would otherwise reach;
 *   - wav[b][m] for 4 (frame_lens[b] - 1) <= m < 4 (frames - 1) is written as exactly 0.0f.  frame_lens[b] < 2: the row owns no sample (all 0.0f);
 *     frame_lens[b] > frames counts as frames.  (The values live in device memory and the callee never synchronises, so none of them can be refused.)
 * wav (B, 4 (frames - 1)).  fade_n is 0 or >= 2 (the ramp divides by fade_n - 1): 1 is refused with CBX_EINVAL before anything is launched, by both entries.
 * cbx_hift_decode passes its lens row 3 (120 n + 1), so the tail of a shorter row of a batch equals its batch-1 synthesis. */
int cbx_hift_istft_rows_f32(const float* x, float* wav, const int* frame_lens, int B, long frames, long ldx, float clamp, int fade_n, void* stream);

/* ---- counter-based device RNG: per-request seeds (added after ABI v16 without a version step: a new function only) ----
 * Replaces, for a request that carries a seed, the draws the reference takes from torch's sequential generator: the draw inside torch.multinomial of the
 * sampling loops (t3.py:360,430,455), torch.randn_like of the CFM noise (flow_matching.py:63,216), and the Uniform(-pi, pi) phase / torch.randn_like noise
 * of SineGen and SourceModuleHnNSF (hifigan.py:212-213,226,282).  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 * 0x9E3779B9 / 0xBB67AE85).
 * out (rows, ld_out >= n): out[r][j - col0] for j in [col0, col0 + n) is defined by the ABSOLUTE column j alone; elements [n, ld_out) are not written.
 * keys (rows, 4) 32-bit words in device memory: seed_lo, seed_hi, substream, stream.  Philox key = (seed_lo, seed_hi); counter = (blk & 0xffffffff, blk >> 32,
 * substream, stream) with blk = j / 4; column j takes output word x = j % 4 of that block.  So a slice equals the same slice of a longer fill for ANY col0.
 *   CBX_RNG_UNIFORM: (x >> 8) * 2^-24, in [0, 1), exact in fp32 (the sampler's inverse CDF takes it as it takes uniform_'s).
 *   CBX_RNG_NORMAL:  Box-Muller over the word pairs (0, 1) and (2, 3) of a block: u1 = ((xa >> 8) + 1) * 2^-24 in (0, 1], u2 = (xb >> 8) * 2^-24,
 *                    r = sqrtf(-2 logf(u1)); the even word gives r cosf(2 pi u2), the odd word r sinf(2 pi u2) (precise libm forms). */
#define CBX_RNG_UNIFORM 0
#define CBX_RNG_NORMAL 1
/* the `stream` key word: what the number is for */
#define CBX_RNG_STREAM_T3_UNIFORMS 0 /* substream 0; column = token step */
#define CBX_RNG_STREAM_CFM_Z 1       /* substream 0; one row per request, column = frame * 80 + channel (the request's own frame index) */
#define CBX_RNG_STREAM_VOC_PHASE 2   /* substream 0; 9 columns (harmonics) */
#define CBX_RNG_STREAM_VOC_NOISE 3   /* substream = harmonic 0 .. 8; column = absolute sample */
int cbx_rng_fill_f32(float* out, long ld_out, const unsigned* keys, int rows, long n, unsigned long long col0, int dist, void* stream);

/* ---- speed control: the mel stretched along time between the flow decoder and the vocoder (added after ABI v16 without a version step: a new function only) ----
 * The reference leaves it out (models/s3gen/s3gen.py:289: "ignoring the speed control (mel interpolation) ... for now"); the F0 predictor runs on the stretched
 * mel, so the pitch is kept.  in (B, T_in, C) and out (B, T_out, C) channel-last with batch strides in_sb / out_sb and row strides in_ld / out_ld (floats, >= C).
 * Row b has M = in_lens[b] valid frames (in_lens NULL: T_in) and rate s = rate[b] (s > 1: faster, fewer frames); the caller supplies out_lens[b] =
 * max(1, floor(M / s)).  Output frame j < out_lens[b] samples the input at x = max(0, (j + 0.5) s - 0.5), evaluated in fp64:
 *   i0 = min(floor(x), M - 1), i1 = min(i0 + 1, M - 1), l = x - i0, out[b][j] = (1 - l) in[b][i0] + l in[b][i1] in fp32
 * -- F.interpolate(mode="linear", align_corners=False, scale_factor=1 / s, recompute_scale_factor=False) with the position in fp64 and no copy shortcut when
 * out_lens[b] == M.  Frames [out_lens[b], T_out) are written as zeros (out_lens[b] is cut to T_out), columns [C, out_ld) are not touched, input frames from
 * in_lens[b] on are never read.  in_lens, rate, out_lens: device memory.  One thread per output float4 when every pointer and stride allows 16-byte access, per
 * float otherwise. */
int cbx_mel_time_scale_f32(const float* in, long in_sb, long in_ld, int T_in, const int* in_lens, const double* rate, float* out, long out_sb, long out_ld,
                           int T_out, const int* out_lens, int B, int C, void* stream);
/* A WINDOW of that map, for the rounds of a stream at a speaking rate (added after ABI v16 without a version step: a new function only; the reference has neither
 * the stretch, models/s3gen/s3gen.py:289, nor a streaming schedule).  The layout arguments are those of cbx_mel_time_scale_f32; `rate` is one host double for every
 * row, j0 the ABSOLUTE index of output frame 0 and i_org the ABSOLUTE index of input frame 0; in_lens / out_lens are relative to the window (in_lens NULL: T_in).
 * Output frame jj < out_lens[b] is frame j = j0 + jj of the whole map: x = max(0, (j + 0.5) rate - 0.5) through the same device function (one fp64 multiply-add),
 * i0 = floor(x) - i_org, i1 = i0 + 1, both clamped into [0, in_lens[b] - 1] whatever the caller passed, l = x - floor(x) cut to [0, 1].  Where both taps lie inside
 * the window the result is bit for bit the frame j of one cbx_mel_time_scale_f32 launch over the whole row; j0 = i_org = 0 gives that launch's bits.  Frames
 * [out_lens[b], T_out) are written as zeros, columns [C, out_ld) are not touched.  rate must be finite and > 0, j0 and i_org in [0, 2^40): else -22 before a launch. */
int cbx_mel_time_scale_win_f32(const float* in, long in_sb, long in_ld, int T_in, const int* in_lens, double rate, long j0, long i_org, float* out, long out_sb,
                               long out_ld, int T_out, const int* out_lens, int B, int C, void* stream);
/* ---- timing control: a PIECEWISE-LINEAR time map of the mel, in the place of cbx_mel_time_scale_f32 (added after ABI v16 without a version step: a new function
 * only; the reference has no time map at all, models/s3gen/s3gen.py:289).  The layout arguments are those of cbx_mel_time_scale_f32.  Row b owns segments
 * [seg_off[b], seg_off[b + 1]) of a packed table of n_seg segments: seg_off is a HOST array of B + 1 ints (it travels by value: B <= 64), seg_o (int32: the first
 * output frame of each segment, increasing, the row's first 0), seg_a (fp64: the input position that output EDGE seg_o maps to) and seg_s (fp64: the rate inside the
 * segment) are DEVICE arrays of n_seg entries, in_lens / out_lens device arrays as ever.  Output frame j < out_lens[b], in the last segment k of its row with
 * seg_o[k] <= j (the row's first when there is none), samples the input at, in fp64,
 *   x = max(0, seg_a[k] + (((j - seg_o[k]) + 0.5) seg_s[k] - 0.5))
 * with the taps of cbx_mel_time_scale_f32: i0 = min(floor(x), M - 1), i1 = min(i0 + 1, M - 1), l = x - i0 cut to [0, 1], out = (1 - l) in[i0] + l in[i1] in fp32.
 * The product term is the same contracted multiply-add: a one-segment table (0, 0.0, s) reproduces cbx_mel_time_scale_f32 at rate s bit for bit.  The map is
 * continuous when seg_a[k + 1] = seg_a[k] + (seg_o[k + 1] - seg_o[k]) seg_s[k].  Memory safety does not depend on the table: the taps are clamped into [0, M - 1]
 * whatever it holds and the search stays inside the row's range.  Frames [out_lens[b], T_out) are written as zeros (out_lens[b] is cut to T_out), columns
 * [C, out_ld) are not touched, input frames from in_lens[b] on are never read.  A null pointer, C <= 0, a stride below C, B outside [0, 64], a negative T_in /
 * T_out / n_seg / seg_off[0], or a row without a segment inside the table (seg_off[b + 1] <= seg_off[b] or > n_seg): -22 before any launch. */
int cbx_mel_time_warp_f32(const float* in, long in_sb, long in_ld, int T_in, const int* in_lens, const int* seg_off, int n_seg, const int* seg_o,
                          const double* seg_a, const double* seg_s, float* out, long out_sb, long out_ld, int T_out, const int* out_lens, int B, int C, void* stream);

/* ---- long-form synthesis: trim and join the waveforms of one sub-batch of text chunks on the device (added after ABI v16 without a version step: new functions
 * only).  The reference stops at 1000 speech tokens (tts.py:249, mtl_tts.py:328) and has no chunking.  Rows: R in [1, 64] waveforms in text order, row r = the
 * row_len[r] floats at wav + row_off[r]; row_off, row_len and gaps are HOST arrays (they travel to the kernels by value).  Frame = 480 samples.
 * cbx_wave_edges_f32: which part of each row is kept.  Frame f of row r covers [480 f, min(480 (f + 1), n_r)), m_f is its mean square, peak = max_f m_f; a frame is
 * live iff m_f > peak * ratio and m_f > 0 (ratio = 10^(-trim_db / 10), computed by the caller in fp64).  With f0 / f1 the first / last live frame: start =
 * 480 max(0, f0 - pad), stop = min(n_r, 480 (f1 + 1 + pad)); no live frame or n_r = 0: (0, 0).  edges: (R, 2) int32 device table {start, stop}.  Squares and sums
 * in fp64, one wave per frame in a fixed order that does not depend on the grid or on the row's alignment, no floating-point atomics: the table is reproducible
 * run to run.  ws: device workspace of ws_cap >= R * ceil(max_r n_r / 480) doubles (the per-frame results; a second launch of this entry reduces them per row).
 * -22 before any launch: a null pointer, R outside [1, 64], a negative length or offset, ratio negative / not finite, pad < 0, a workspace that is too small. */
int cbx_wave_edges_f32(const float* wav, const long* row_off, const int* row_len, int R, double ratio, int pad, int* edges, double* ws, long ws_cap, void* stream);
/* cbx_wave_join_f32: ONE launch lays the kept parts out in `out`.  edges: the (R, 2) device table of cbx_wave_edges_f32, or {0, n_r} written by the caller (no
 * trimming); every entry is cut into [0, n_r] by the kernel.  L_r = stop_r - start_r; off_0 = 0, off_(r+1) = off_r + L_r + gap_r with gap_r = gaps[r] iff L_r > 0 and
 * not (last and r = R - 1), else 0; total = off_R.  out[off_r + i] = wav_r[start_r + i] for i < L_r, times ramp[i] for i < F (fade-in; not when first and r = 0 and
 * start_r = 0), times ramp[L_r - 1 - i] for i >= L_r - F (fade-out; not when last and r = R - 1 and stop_r = n_r), F = min(fade, L_r / 2): one fp32 multiply.
 * ramp: `fade` device floats, (2 i + 1) / (2 fade) by convention (NULL when fade = 0).  The gap behind a row is written as zeros; nothing at or beyond `total` is
 * written.  layout: R + 1 device ints, off_0 .. off_(R-1) and total.  first / last: this piece begins / ends the whole text.
 * -22 before any launch: a null pointer, R outside [1, 64], a negative gap, fade, length or offset, out_cap below sum n_r + sum gaps[r] (or that sum >= 2^31). */
int cbx_wave_join_f32(const float* wav, const long* row_off, const int* row_len, const int* gaps, int R, const int* edges, const float* ramp, int fade, int first,
                      int last, float* out, long out_cap, int* layout, void* stream);

/* ---- pause control: shorten long silences INSIDE the rows of a batch on the device (added after ABI v16 without a version step: a new function only).  The
 * reference returns the waveform with whatever holes T3 sampled (tts.py:272, mtl_tts.py:352, tts_turbo.py:320, vc.py:104) and has no such step.  Rows as
 * cbx_wave_join_f32 takes them: R in [1, 64] rows of row_len[r] floats at wav + row_off[r]; row_off, row_len and keep are HOST arrays (by value).  Row r has n samples x.
 * Frames: frame f covers [480 f, min(480 (f + 1), n)); m_f = its mean square in fp64, computed by the frame kernel of cbx_wave_edges_f32 itself (one source: the
 *   same bits); peak = max_f m_f as that entry takes it (fmax from 0: a NaN frame is ignored by the peak).
 * Silent: frame f is silent iff m_f <= peak * ratio or m_f == 0 (ratio = 10^(-pause_db / 10), computed by the caller in fp64).  A frame whose m_f is NaN is NOT
 *   silent and is never removed -- this differs from cbx_wave_edges_f32, where a NaN frame is not live (there NaN counts as silence, here as signal).
 * Runs: f0 / f1 = the first / last non-silent frame; none: nothing is removed.  A pause is a maximal run [a, b) of silent frames with f0 < a and b <= f1, P = b - a
 *   frames long.  Leading and trailing silence is not a pause (cbx_wave_edges_f32 trims that).
 * Cut: K = keep[r]; 0: row r is copied unchanged; else K >= 2, and of every pause with P > K the frames [a + h, b - t) are removed, h = K - K / 2, t = K / 2 (integer
 *   division): in samples [c0, c1) = [480 (a + h), 480 (b - t)).  Only whole frames are removed; the row's partial last frame is never removed and is never the
 *   frame ahead of a cut.
 * Output: row r of the result lives at out + row_off[r] (same layout, another buffer; out overlapping wav is refused).  n' = n - 480 sum (P - K); y[0, n') = the
 *   kept samples in order, y[n', n) is written as zeros, nothing outside [0, n) of the row is written.
 * Seam: with F = fade in [0, 480] and ramp[i] = (2 i + 1) / (2 fade) by convention (`fade` device floats; NULL when fade = 0), for each cut with q = map(c0), i < F:
 *   y[q - F + i] = fmaf(ramp[i], x[c1 - F + i] - x[c0 - F + i], x[c0 - F + i]) -- one fp32 subtraction and one fmaf.  Both operands lie in silent frames of the
 *   same run (the kept head frame a + h - 1, the removed frame b - t - 1); no sample is blended twice.
 * Map: map(p) = the number of kept samples in [0, p), p in [0, n].  edges (NULL, or an (R, 2) int32 device table, in / out): each entry {start, stop} is cut into
 *   [0, n] as the join cuts it and rewritten as {map(start), map(stop)} -- the table cbx_wave_edges_f32 wrote for the ORIGINAL rows, or {0, n} written by the
 *   caller (which becomes {0, n'}), so that cbx_wave_join_f32 over the result, with the host-side lengths n, never sees the zero tail: no host round trip.
 * Record: stats = (R, 4) int32 device table {n', pauses cut, frames removed, n}.
 * Three launches (the frame pass, one workgroup per row that plans, one wave per output frame that gathers); integer scans in a fixed order, no atomics: the
 * result does not depend on the grid or on a row's alignment; 16-byte accesses where a row's addresses allow, 4-byte accesses elsewhere; positions are 64-bit.
 * ws: device workspace of ws_cap BYTES on an 8-byte boundary, ws_cap >= 16 * R * ceil(max_r n_r / 480): per frame one double (m_f) and two ints (the next
 * non-silent frame; the source frame of each output frame).  out_cap: floats in `out`, at least max_r (row_off[r] + n_r).
 * -22 before any launch, nothing written: a null pointer (edges may be NULL), R outside [1, 64], a negative length or offset, keep[r] = 1 or negative, ratio
 * negative / not finite, fade outside [0, 480], fade > 0 without a ramp, out overlapping wav, out_cap short of the furthest row end, a workspace that is too
 * small. */
int cbx_wave_squeeze_f32(const float* wav, const long* row_off, const int* row_len, const int* keep, int R, double ratio, const float* ramp, int fade, float* out,
                         long out_cap, int* edges, int* stats, void* ws, long ws_cap, void* stream);

/* ---- pitch control: read the rows of a batch back at an arbitrary real step, one launch (added after ABI v16 without a version step: a new function only).  The
 * reference vocodes the flow's mel as it is (models/s3gen/s3gen.py:289) and returns the result (tts.py:272, mtl_tts.py:352, tts_turbo.py:320, vc.py:104); it has
 * no transpose.  Here a pitch of p semitones, p in [-12, 12], is the ratio r = 2^(p / 12): with the speaking rate s the mel is stretched at s_eff = s / r
 * (cbx_mel_time_scale_f32; s_eff in [0.5, 2]), the vocoder runs on the stretched mel, and this entry reads its cut row -- the source, n_src = 480 scaled_len(K,
 * s_eff) samples for the K frames of the unscaled call -- at step = r into N = 480 scaled_len(K, s) samples: exactly the length of the call without a pitch, every
 * frequency multiplied by r.  The formants move with the pitch (varispeed with the duration restored); nothing here preserves them.
 * Rows as cbx_wave_format_f32 takes them: R in [1, 64] rows of row_len[r] floats at wav + row_off[r]; row_off, row_len, step, out_len and out_off are HOST arrays
 * (by value; 4-byte alignment of a row is enough).  step[r]: source samples per output sample, a finite double in [0.5, 2]; c = min(1.0, 1.0 / step), computed
 * here in fp64: the cutoff relative to the source's Nyquist rate, and the gain.
 * Filter: Z zero crossings per side, L table steps per crossing, h(t) = sinc(t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta) for |t| < Z, else 0 (the project uses Z = 16,
 *   L = 256, Kaiser beta = 9.0).  tab: Z L + 2 device floats built by the CALLER in fp64, tab[k] = h(k / L); tab[0] = 1, and tab[k] = 0 exactly at every other
 *   multiple of L and for k >= Z L.
 * Output j < out_len[r] of a row x of n = row_len[r] samples:
 *   x_j = j * step in fp64; for i ascending over max(0, ceil(x_j - Z / c)) .. min(n - 1, floor(x_j + Z / c)):
 *     u = |x_j - i| * c * L in fp64; the tap is skipped if u >= Z L; k = (long)u, a = (float)(u - k);
 *     w = fmaf(a, tab[k + 1] - tab[k], tab[k]); acc = fmaf(w, x[i], acc) starting from 0;
 *   y[j] = (float)c * acc.
 *   Taps outside the row read nothing: an output whose taps all lie outside [0, n) is 0.  At most floor(2 Z / c) + 2 taps per output (66 at step 2).  step = 1
 *   returns the input's bits for finite samples (a -0 comes back as +0); h is continuous, so how the compiler rounds x_j - i does not matter beyond the bound.
 * out: ONE buffer of out_cap floats; row r's outputs go to out + out_off[r].  Nothing else is written.  One workgroup per 256 outputs of a row; the result does not
 * depend on the grid or on a row's alignment; 16-byte loads where a row's addresses allow, 4-byte accesses elsewhere; positions are 64-bit.
 * -22 before any launch, nothing written: a null pointer, R outside [1, 64], a negative length or offset, a step that is not finite or outside [0.5, 2], Z or L < 1
 * or Z L + 2 > 4098 (or a reach 2 Z / c beyond the kernel's staging), a row that would write outside [0, out_cap), out_cap below the sum of the rows' outputs, out
 * overlapping wav. */
int cbx_wave_pitch_f32(const float* wav, const long* row_off, const int* row_len, const double* step, const int* out_len, int R, const float* tab, int Z, int L,
                       float* out, const long* out_off, long out_cap, void* stream);

/* ---- word timestamps: the attention mass selected heads put on the text columns, and the monotonic path through it (added after ABI v16 without a version
 * step: new functions only).  The reference returns a waveform and nothing about when a word is spoken (tts.py:272, mtl_tts.py:352); its later alignment analyser
 * reads a few heads of T3 -- a decoder over [34 conditioning | text | BOS BOS | speech ..] -- through forward hooks that materialise whole attention rows.  Here
 * the rows never exist.  Plain C++ kernels: no inline assembly, no atomics, every output element written by exactly one thread per launch in a fixed summation
 * order.
 * cbx_attn_text_mass_f32: attention probability restricted to a column range, summed over selected heads.  q, k addressed as cbx_flash_attn_kv_f32 addresses them
 * (head_dim 64): q = base + z q_sb + (q0[z] + i) q_st + head 64 (q0: the row's first query in its q block; NULL = zeros), k = base + z k_sb + j k_st + head k_sh -- T3's KV cache [row][head][max_ctx][64] has k_st = 64, k_sh =
 * max_ctx 64; both read with 16-byte loads (pointers on 16-byte boundaries, strides multiples of 4 floats).  HOST arrays, by value to the kernel: heads[n_sel],
 * 1 <= n_sel <= 16, each in [0, n_heads), the heads of THIS layer (a repeated head counts twice); per row z < nz, nz in [1, 64]: q0[z], q_len[z] valid queries (0: the
 * row writes nothing), ctx0[z] (query i sees the keys j <= ctx0 + i), t0[z] / t_len[z] (the text columns [t0, t0 + t_len), t0 + t_len <= ctx0 + 1: visible to
 * every query).
 *   s_h[i][j] = scale * sum_(d = 0 .. 63) q_i[d] k_j[d], by fmaf in the order d = 0 .. 63 from 0;
 *   p_h[i][j] = expf(s_h[i][j] - M) / L with M = max_j s_h[i][j] and L = sum_j expf(s_h[i][j] - M) over ALL visible keys j <= ctx0 + i: the normaliser covers
 *     the whole causal row, not the text columns alone (running maximum and sum per lane over the keys j = lane mod 64, joined by the xor butterfly 32 .. 1);
 *   mass[z][i][t] = (accumulate ? mass[z][i][t] : 0) + weight * sum_(h in heads, in list order) p_h[i][t0 + t],   mass = base + z m_sb + i m_si + t, fp32.
 * Elements with i >= q_len[z] or t >= t_len[z] are not written.  A key beyond ctx0 + i never reaches query i's result, whatever the cache holds there (NaN
 * included), and no key beyond ctx0 + q_len - 1 is loaded.  One launch (none when no row has a query and a text column): one wave per 4 queries of a row.
 * Caps: ctx0 + q_len <= 4608 (the RoPE table), t_len <= 1024.
 * -22 before any launch, nothing written: a null pointer, nz outside [1, 64], n_sel outside [1, 16], a head outside [0, n_heads), a negative length, offset or
 * stride, a context or text range over the caps, t0 + t_len > ctx0 + 1, q / k not 16-byte addressable, m_si < t_len or (nz > 1) m_sb < q_len m_si. */
int cbx_attn_text_mass_f32(const float* q, const float* k, float* mass, const int* heads, int n_sel, int n_heads, const int* q0, const int* q_len, const int* ctx0,
                           const int* t0, const int* t_len, int nz, long q_sb, long q_st, long k_sb, long k_st, long k_sh, long m_sb, long m_si, float scale, float weight,
                           int accumulate, void* stream);
/* cbx_align_path_f32: the best monotonic path through a score matrix, on the LINEAR scores (as DTW over attention weights is usually done: no log is taken);
 * exact: fp32 adds and compares only.  score = base + z s_sb + i s_si + t, any finite fp32; n[z] frames (1 .. 4096) and m[z] text tokens (1 .. 1024) per row
 * z < nz, nz in [1, 64] (HOST arrays, by value).
 *   D[0][0] = score[0][0]; D[0][t > 0] = -inf
 *   D[i][t] = score[i][t] + max(D[i-1][t], D[i-1][t-1]) (t = 0: D[i-1][0] only); move[i][t] = (D[i-1][t-1] > D[i-1][t]) -- a tie stays
 *   end e = m - 1 if n >= m, else the lowest t <= n - 1 with the largest D[n-1][t]
 *   walk back from (n - 1, e): frame_tok[i] = t; t -= move[i][t]
 *   spans[t] = (first frame, last frame + 1) of the frames with frame_tok == t for t <= e; (n, n) for t > e (never reached)
 * The path starts at token 0 and moves by 0 or 1 per frame; when n >= m it ends at m - 1 and every span is non-empty.
 * spans: int32 pairs at base + z sp_sb + 2 t (sp_sb in ints); frame_tok: int32 at base + z ft_sb + i.  Nothing beyond m[z] pairs / n[z] frames of a row is
 * written.  One launch for the rows of a batch: one workgroup per row, thread t owns column t, one barrier per frame, one thread walks back.
 * ws: device workspace of ws_cap BYTES on an 8-byte boundary for the move bits, ws_cap >= 8 * nz * max_z n[z] * ceil(max_z m[z] / 64).
 * -22 before any launch, nothing written: a null pointer, nz outside [1, 64], n outside [1, 4096], m outside [1, 1024], s_si < m, (nz > 1) a row stride
 * short of the row (s_sb < n s_si, sp_sb < 2 m, ft_sb < n), a workspace that is misaligned or too small. */
int cbx_align_path_f32(const float* score, long s_sb, long s_si, const int* n, const int* m, int nz, int* spans, long sp_sb, int* frame_tok, long ft_sb, void* ws,
                       long ws_cap, void* stream);

/* ---- alignment guard: the text mass of the CURRENT decode query and a per-utterance state machine on it, both inside the captured token step (added after ABI
 * v16 without a version step: new functions only; no existing struct changes).  T3 sometimes never samples its end-of-speech token, or samples it too early; the
 * reference project's later alignment analyser watches a few heads for that on the host.  Here the two launches ride in the step: nothing is allocated, nothing
 * synchronises, and everything that varies per step or per request is read from DEVICE memory (positions, step, done, t_len, thresholds), so a new request replays
 * the same captured graph.  Plain C++ kernels: no inline assembly, no atomics, every output element written by exactly one thread in a fixed summation order; two
 * runs are bit-identical.
 * cbx_guard_text_mass_f32: launched right after the cbx_decode_attn_rope launch of one layer (the new position's K is in the cache, the step's q/k/v buffer still
 * live), for the conditional rows b < B and the heads[n_sel] of THAT layer (HOST array, by value; 1 <= n_sel <= 16, each in [0, n_heads), a repeated head is
 * computed twice).
 *   q: as the attention launch sees it (cbx_decode_attn_t): qkv + b ld_qkv + head 64 + d; qkv_nparts 2 or 4: the parts at multiples of qkv_part_stride added in part
 *     order, times rsqrtf(ssq / rms_dim + rms_eps) with ssq = sum over parts, in part order, of qkv_ssq[part 16 + b] (then B <= 16); qkv_nparts 0 or 1: the row as it
 *     is, qkv_ssq may be NULL and parts beyond qkv_nparts are never read; rotated by cos_t / sin_t ([pos][64]) at pos = positions[b]: q[d] cos[d] -/+ q[d ^ 32]
 *     sin[d] (- for d < 32); cos_t = sin_t = NULL: no rotation.
 *   k_j = kc + b k_row_stride + head k_head_stride + j 64 (one layer of T3's KV cache; 16-byte loads).
 *   s[j] = scale * sum_(d = 0 .. 63) q[d] k_j[d], by fmaf in the order d = 0 .. 63 from 0, over ALL visible keys j <= positions[b];
 *   p[j] = expf(s[j] - M) / L, M = max_j s[j], L = sum_j expf(s[j] - M): the normaliser covers the whole causal row (a thread adds its keys j = tid mod 256 in
 *     order, a wave's 64 lanes by the xor butterfly 32 .. 1, the 4 waves in wave order);
 *   stored: p[t0 + t] for t < t_len[b] at p + s p_ss + b p_sb + t, s the head's index in `heads` (the caller offsets p by the slots of earlier layers).
 * A key beyond positions[b] is never loaded.  A row with done[b] != 0 writes nothing; neither does a row outside the caps, which are checked on the device because
 * the numbers live there: t_len[b] in [1, t_cap], positions[b] in [0, max_ctx), t0 + t_len[b] <= positions[b] + 1.  Columns t >= t_len[b] are not written.
 * Caps: max_ctx <= 4608 (the RoPE table; also the keys a head of kc holds), t_cap <= 1024, n_sel <= 16, B <= 64.
 * One launch: one workgroup of 256 threads per (row, selected head), that head's K streamed once, the row's scores kept in LDS.
 * -22 before any launch, nothing written: a null pointer (cos_t / sin_t: one without the other), B outside [1, 64], n_sel outside [1, 16], a head outside
 * [0, n_heads), qkv_nparts not 0, 1, 2 or 4 (or > 1 without qkv_ssq, rms_dim > 0, B <= 16), ld_qkv < 64 n_heads, a negative stride, kc not 16-byte addressable,
 * max_ctx outside [1, 4608] or beyond k_head_stride, t0 < 0, t_cap outside [1, 1024], p_sb < t_cap or (n_sel > 1) p_ss short of B rows. */
int cbx_guard_text_mass_f32(const float* qkv, long ld_qkv, int qkv_nparts, long qkv_part_stride, const float* qkv_ssq, int rms_dim, float rms_eps, const int* positions,
                            const float* cos_t, const float* sin_t, const float* kc, long k_row_stride, long k_head_stride, int max_ctx, const int* heads, int n_sel,
                            int n_heads, int B, const int* done, const int* t_len, int t0, int t_cap, float scale, float* p, long p_ss, long p_sb, void* stream);
/* cbx_guard_update_f32: once per step, between the head GEMV and cbx_t3_sample; one workgroup (1024 threads, thread t owns text column t) per utterance b < B.
 * Device state per utterance: state[b][8] int32 = {pos, complete, completed_at, fired, fired_at, 0, 0, 0}, sums[b][4] fp32 = {tail_sum[3], rep_sum}, all zero at
 * the start of a request.  thresholds[b][8] fp32 = {back, ahead, end_tokens, tail, repeat, repeat_skip, token_run, hold_min}; end_tokens is clamped to 1 .. 3
 * (tail_sum has three entries); hold_min: hold the end token back for texts of at least hold_min tokens, < 0: never.
 * A row with done[b] != 0 or fired != 0 does nothing; neither does one with m = t_len[b] outside [1, min(1024, m_si)] or i = step[b] outside [0, max_steps).
 * Otherwise, with p_h[s][b][t] = p[s p_ss + b p_sb + t] the slots the mass launches of this step filled:
 *   1. a[t] = weight * sum_(s = 0 .. n_sel-1, in order) p_h[s][b][t], weight = 1.0f / n_sel, stored to mass[b m_sb + i m_si + t] (the history), t < m.
 *   2. cur = the lowest t with the largest a[t]; if -back <= cur - pos <= ahead then pos = cur (a jump outside the window is ignored).
 *   3. if not complete and pos >= m - end_tokens: complete = 1, completed_at = i.
 *   4. if complete (the latching step included): tail_sum[j] += a[max(0, m - end_tokens) + j] for j < min(end_tokens, m) -- the last min(end_tokens, m) columns --;
 *      rep_sum += max_(t < m - repeat_skip) a[t], or 0 when there is no such column.  fp32 adds in step order.
 *   5. run = token_run > 0 and i >= token_run and out_tokens[b max_steps + i-1 .. i-token_run] are all equal.
 *   6. reason = the first that holds: 1 (tail) complete and max_(j < min(end_tokens, m)) tail_sum[j] >= tail; 2 (repeat) complete and rep_sum >= repeat; 3 (run);
 *      else 0.  The two sums exist once complete (they are 0 before: `complete` matters for a threshold of 0 alone, which then means "at completion").
 *   7. reason != 0: fired = reason, fired_at = i; logits[b ld_logits + v] and logits[(B + b) ld_logits + v], v < V, become 0 and 32768 at v = eos -- the sampler's
 *      c + w (c - u) is then this pattern for every w, every processor order leaves probability 1 on eos for every uniform, and cbx_t3_sample itself writes the
 *      token, sets done and stops the row --; dev_params[b][6] (the sampler's ban token) = -1.  Columns v >= V of a padded row are not touched.
 *      reason == 0: dev_params[b][6] = eos when hold_min >= 0 and m >= hold_min and not complete, else -1 (the sampler's existing per-utterance ban).
 *   8. trace[b max_steps + i] = pos | complete << 16 | ban << 17 | reason << 18 (ban: 1 when dev_params[b][6] was set to eos).
 * Frame 0 is sampled from the prefill logits and passes no step: the first call sees i = 1 and pos = 0; the host writes the first ban into dev_params.
 * -22 before any launch, nothing written: a null pointer, B outside [1, 64], n_sel outside [1, 1024], max_steps < 1, V < 1, eos outside [0, V), ld_logits < V, a
 * negative stride of p, m_si < 1, (B > 1) m_sb < max_steps m_si. */
int cbx_guard_update_f32(const float* p, long p_ss, long p_sb, int n_sel, const int* t_len, const int* step, const int* done, const float* thresholds,
                         const long long* out_tokens, int max_steps, float* mass, long m_sb, long m_si, int* state, float* sums, int* trace, float* logits, long ld_logits,
                         int V, int B, int eos, float* dev_params, void* stream);

/* ---- output formats: resample 24 kHz fp32 to the delivery rate and encode it, one launch for the rows of a batch or of a stream's round (added after ABI v16
 * without a version step: a new function only).  The reference returns 24 kHz fp32 and leaves this to its caller (tts.py:272, mtl_tts.py:352, tts_turbo.py:320,
 * vc.py:104).  Rows as cbx_wave_join_f32 takes them: R in [1, 64] pieces of row_len[r] floats at wav + row_off[r] (HOST arrays; 4-byte alignment is enough).
 * rate: 8000, 16000, 22050, 24000, 32000, 44100 or 48000; U / D = rate / 24000 reduced.  The filter is scipy.signal.resample_poly's default design, built by the
 * CALLER in fp64: hl = 10 max(U, D), h = U firwin(2 hl + 1, 1 / max(U, D), window = ("kaiser", 5.0)); tab: its fp32 phase table in device memory, tab[p * T + j] =
 * h[p + j U] (zero past 2 hl), T = ceil((2 hl + 1) / U) taps per output; the U and T of the table are passed and must be the rate's.  Output m of a row of n samples:
 *   c = m D + hl, p = c mod U, k_hi = c div U, y[m] = sum_(j = 0 .. T - 1) tab[p][j] x[k_hi - j], x[k] = 0 outside [0, n), m in [0, ceil(n U / D))
 * accumulated in fp32 by fmaf in the order j = 0 .. T - 1, starting from 0 -- resample_poly(x, U, D) to fp32 rounding.  24000: no filter, y = x (tab may be NULL,
 * U = T = 1).  encoding, fused into the store: 0 fp32 y as it is; 1 int16 clamp(rintf(y * 32768), -32768, 32767), ties to even, NaN -> 0; 2 / 3 one byte, the
 * G.711 mu-law / A-law code of that int16 (audioop.lin2ulaw / lin2alaw at width 2).  The y under an encoded store is bit for bit the y encoding 0 stores.  No dither.
 * out: ONE buffer of out_cap elements of the encoding's type; row r's outputs go to out + out_off[r] (HOST array, elements).
 * Continuation (n0, m0, fin: HOST arrays of R entries, all three or none; none = {0, 0, 1}: the one-shot call).  Row r's piece holds absolute samples
 * [n0[r], n0[r] + L) of its signal, m0[r] outputs exist already, and the launch produces m0 <= m < m1: m1 = ceil((n0 + L) U / D) when fin[r], else
 * floor(((n0 + L - 1) U - hl) / D) + 1, the outputs all of whose taps lie below n0 + L (never less than m0; 0 when the numerator is negative).  Sample k is read from
 * hist_in[r * H + k - (n0 - H)] for n0 - H <= k < n0 (H = ceil(2 hl / U), the last H samples before the piece; NULL when every n0 is 0), from the piece for
 * n0 <= k < n0 + L, as zero elsewhere; hist_out (NULL: not kept) receives the last H samples before n0 + L, and is another buffer than hist_in (ping-pong).  Pieces
 * of 0 samples or of fewer than H are fine.  For finite samples the concatenated outputs of ANY split of a row are bit for bit its one-shot outputs.  All positions
 * are 64-bit.
 * -22 before any launch: a null pointer, R outside [1, 64], a negative length, offset, n0 or m0, an unknown rate or encoding, U / T that are not the rate's, a
 * continued row without a history, hist_out == hist_in, a row that would write outside [0, out_cap), out_cap below the sum of the rows' outputs. */
int cbx_wave_format_f32(const float* wav, const long* row_off, const int* row_len, int R, int rate, int encoding, const float* tab, int U, int T, const long* n0,
                        const long* m0, const int* fin, const float* hist_in, float* hist_out, void* out, const long* out_off, long out_cap, void* stream);

/* ---- loudness: measure the integrated loudness of the rows of a batch, derive the gain to a LUFS target, apply it in place (added after ABI v16 without a
 * version step: new functions only).  The reference levels only Turbo's voice prompt, on the host with pyloudnorm (tts_turbo.py:223-239: norm_loudness to -27 LUFS);
 * its outputs keep whatever level the vocoder gives them.  Rows as cbx_wave_join_f32 takes them: R in [1, 64] rows of row_len[r] floats at wav + row_off[r] (HOST
 * arrays; 4-byte alignment is enough).
 * Definition: ITU-R BS.1770-4 integrated loudness of one channel at sample rate fs.
 *   K-weighting: two biquads in cascade, coefficients built by the CALLER in fp64 with the RBJ forms pyloudnorm.Meter uses -- high shelf G = +4 dB, Q = 1 / sqrt 2,
 *     fc = 1500 Hz; high pass Q = 0.5, fc = 38 Hz; both normalised by a0 --, coef[10] = b0 b1 b2 a1 a2 of the shelf, then of the high pass (HOST doubles).  At 24 kHz
 *     the high pass has a double pole at ~0.9901: state and sums are fp64 (an fp32 recurrence loses ~5e-3 LU).
 *   Segments: hop = fs / 10 samples (an integer); segment s covers [s hop, (s + 1) hop) for s < S = floor(n / hop); E_s = the fp64 sum of squares of the filtered
 *     signal over segment s.
 *   Blocks: z_j = (E_j + E_(j+1) + E_(j+2) + E_(j+3)) / (4 hop) for j <= S - 4, l_j = -0.691 + 10 log10(z_j).  The incomplete block at the end is not used (the
 *     Recommendation's rule; pyloudnorm counts round() blocks and may add a partial one -- we follow the Recommendation; the difference is not measured).
 *   Gates: absolute l_j >= -70; relative G = -0.691 + 10 log10(mean z over the absolute gate) - 10; L = -0.691 + 10 log10(mean z over the blocks with l_j >= -70
 *     and l_j > G); L = -inf when no block passes or n < 4 hop.
 *   Peak: max |x| over [0, n) (0 for n = 0; NaN when the row holds a NaN).
 *   Gain, in fp64: g = 10^((target - L) / 20); if ceiling > 0 and peak g > ceiling then g = ceiling / peak; g = 1 when target is NaN (measure only) or when L,
 *     peak or g is not finite.  The stored gain is (float)g; the applied signal is x[i] * g, one fp32 multiply, in place.
 * cbx_wave_loudness_f32: target: R HOST doubles.  stats: (R, 4) device doubles {L, peak, g, blocks used}; gain: R device floats.  The filter is run exactly, not
 * from a warm-up: every 1/64th of a segment from zero state, a wave-level scan of the 4-vector states with powers of the 4 x 4 transition matrix (built by the entry
 * on the host, passed by value), a chain over each row's segments, then a second pass from the true states (wave_loudness.hip).  A row's segments from the first one
 * whose E is not finite on count as NaN, and a block with a NaN passes no gate.  Fixed reduction order, independent of the grid and of the rows' alignment, no
 * floating-point atomics: the numbers are reproducible run to run.  Four launches (one when every row is empty), nothing synchronises the host.
 * ws: device workspace of ws_cap >= 6 * R * ceil(max_r n_r / hop) doubles (not NULL).
 * -22 before any launch: a null pointer, R outside [1, 64], a negative length or offset, hop < 1, a coefficient that is not finite, a workspace that is too small. */
int cbx_wave_loudness_f32(const float* wav, const long* row_off, const int* row_len, int R, const double* coef, int hop, const double* target, double ceiling,
                          double* stats, float* gain, double* ws, long ws_cap, void* stream);
/* cbx_wave_loudness_push_f32: the same meter fed piece by piece (a running / streaming loudness; new function, no version step).  The reference has no counterpart:
 * it levels only Turbo's voice prompt, on the host (tts_turbo.py:223-239).
 * State of a meter of R rows, R in [1, 64], all of it on the device and owned by the caller:
 *   rec: R records of 8 + seg_cap doubles: [0..3] the cascade's state on entry to the first segment that is not yet complete, [4] the running sample peak (NaN once
 *     a NaN was seen), [5..7] zero, then E_0 .. E_(seg_cap-1).  A new meter is all zeros.
 *   tail_in / tail_out: two buffers of R x hop floats that alternate from push to push (as the histories of cbx_wave_format_f32); row r's n0[r] mod hop samples of
 *     the unfinished segment are at tail + r hop.  tail_in is only read.
 *   n0: R HOST longs, the samples row r has consumed so far (the sum of its earlier piece lengths), by value like row_off / row_len.
 * A push over pieces of L_r = row_len[r] >= 0 samples at wav + row_off[r] (0: nothing new).  With t = n0 mod hop, S0 = n0 div hop and the virtual signal
 * v = tail_in[0, t) ++ piece[0, L): the K = (t + L) div hop whole segments of v get E_(S0 + k) by the three phases and the per-lane partition of
 * cbx_wave_loudness_f32 (lane l owns samples [l c, (l + 1) c) of its segment, c = ceil(hop / 64); the zero-state pass; the chain s_(k+1) = A^hop s_k + v_k, which
 * starts from rec[0..3] instead of 0; the true-state pass with the same xor butterfly) -- one source for both entries, so one arithmetic.  rec[0..3] becomes the state
 * on entry to segment S0 + K, the last (t + L) mod hop samples of v go to tail_out, rec[4] becomes max(rec[4], max |piece|).  Then the row step of
 * cbx_wave_loudness_f32 (blocks, both gates, L, gain, ceiling) runs over E_0 .. E_(S0 + K - 1) with the running peak and writes stats (R, 4) and gain (R) as there; a
 * NaN target is measure only, gain 1.
 * CONTRACT: after any sequence of pushes, stats, gain and the E table are bit for bit those of cbx_wave_loudness_f32 over each row's concatenated pieces (same
 * coefficients, target and ceiling).  No floating-point atomics, a fixed order whatever the grid and the rows' alignment, 4-byte accesses at ragged ends; nothing
 * outside the records, tail_out, stats, gain and the workspace is written.  Four launches (two when no row completes a segment), nothing synchronises the host.
 * ws: device workspace of ws_cap >= 4 * R * max_r K_r doubles (not NULL; K_r the whole segments this push completes in row r).
 * -22 before any launch, nothing written: a null pointer, tail_out == tail_in, R outside [1, 64], a negative length, offset or n0, hop < 1, a coefficient that is
 * not finite, S0 + K > seg_cap for any row, a workspace that is too small. */
int cbx_wave_loudness_push_f32(const float* wav, const long* row_off, const int* row_len, const long* n0, int R, const double* coef, int hop, const double* target,
                               double ceiling, double* rec, long seg_cap, const float* tail_in, float* tail_out, double* stats, float* gain, double* ws, long ws_cap,
                               void* stream);
/* cbx_wave_gain_f32: wav_r[i] = wav_r[i] * gain[r] for i < n_r, ONE launch (none when every row is empty); gain: R device floats (cbx_wave_loudness_f32's).
 * 16-byte accesses inside a row where alignment allows, 4-byte accesses at the ragged ends; nothing outside the rows is touched.
 * -22 before any launch: a null pointer, R outside [1, 64], a negative length or offset. */
int cbx_wave_gain_f32(float* wav, const long* row_off, const int* row_len, int R, const float* gain, void* stream);

/* ---- true-peak limiter: hold the rows of a batch under a dBTP ceiling (added after ABI v16 without a version step: new function only).  The reference has no
 * counterpart: it returns the vocoder's output as is (tts.py:272, mtl_tts.py:352, tts_turbo.py:320, vc.py:104).  Rows as cbx_wave_gain_f32 takes them: R in
 * [1, 64] rows of row_len[r] floats at wav + row_off[r] (HOST arrays; 4-byte alignment is enough).
 * Inputs per row r: x, n fp32 samples; a pre-gain gamma = gain[r] (R device floats; NULL: 1); a linear ceiling C = ceiling[r] > 0 (R HOST doubles; NaN: the row
 * is not limited), used as C32 = (float)C.  Two tables built by the CALLER in fp64, in device memory:
 *   tab: the oversampler.  hl = 10 U, h = U firwin(2 hl + 1, 1 / U, window = ("kaiser", 5.0)) -- cbx_wave_format_f32's design --, tab[p * T + j] = h[p + j U] (zero
 *     past 2 hl), T = ceil((2 hl + 1) / U).  The product uses U = 4, T = 21.
 *   win: the smoothing window, 2 H + 1 floats w_k proportional to 0.5 (1 + cos(pi k / (H + 1))), k = -H .. H, normalised to sum 1 in fp64 (win[k + H]).  H is the
 *     look-ahead in samples; the product uses H = 120 (5 ms at 24 kHz).
 * Definition, in fp32:
 *   1. u[i] = x[i] * gamma: one multiply, the bits cbx_wave_gain_f32 would store.
 *   2. y[k] = sum_i u[i] h[k - U i + hl] for k = 0 .. U n - 1 (scipy.signal.resample_poly's alignment: y[U i] is centred on u[i]); samples outside [0, n) are 0.
 *      With k = U i + p: y[k] = sum_(j = 0 .. T - 1) tab[p][j] u[i + 10 - j], by fmaf in the order j = 0 .. T - 1 from 0 (the taps of h ascending).
 *   3. m[i] = max(|u[i]|, |y[U i]|, .., |y[U i + U - 1]|); NaN when one of them is.
 *   4. c[i] = C32 / m[i] (one IEEE division) where m[i] is finite and > C32, else 1; c = 1 outside [0, n).
 *   5. a[i] = min over |j - i| <= H of c[j], for i in [-H, n + H).
 *   6. s[i] = sum_(k = -H .. H) w_k (1 - a[i + k]), 1 - a rounded once, then fmaf in the order k = -H .. H from 0; g[i] = min(1 - s[i], c[i]).
 *   7. out[i] = u[i] * g[i].
 * Properties: |out[i]| <= C32 up to the two roundings of steps 4 and 7, at the samples and at the U - 1 oversampled points between them of u c; every a[i + k] of
 * step 6 has i inside its window, so 1 - s[i] <= c[i] holds in exact arithmetic and the min only absorbs rounding.  A row with m <= C32 everywhere returns u bit for
 * bit: every term of s is exactly 0.  A row with C = NaN likewise returns u (the bits cbx_wave_gain_f32 gives), so a batch that mixes limited and other rows needs no
 * launch of cbx_wave_gain_f32.  The result does not depend on the grid, the tile a sample falls into or the row's alignment, bit for bit.
 * stats: (R, 4) device doubles {the true peak of u = max_i m[i] (NaN when an m is NaN; 0 for an empty row), min_i g[i], the samples with g < 1, the samples with
 * m > C32 (an infinite m counts)}.  out: one fp32 buffer of out_cap floats, row r's n_r outputs at out + out_off[r] (HOST array); NULL (out_off may then be NULL):
 * measure only, stats alone are written.  wav is only read; out must not overlap it; nothing outside the rows of out is written.  16-byte loads and stores inside a
 * row where alignment allows, 4-byte accesses at the ragged ends.
 * One workgroup per tile of 1024 outputs of a row (wave_limit.hip): u over tile +- 2 H plus the filter's reach in LDS, the sliding minimum by doubling passes, the
 * smoothing sum in the order above.  Per-tile partial stats go to ws; a second launch folds them per row (max, min and integer counts: exact in any order).  No
 * floating-point atomics.  Two launches; ONE, the fold, when every row is empty: it writes {0, 1, 0, 0} per row.  Nothing synchronises the host.
 * ws: device workspace of ws_cap >= 4 * R * ceil(max_r n_r / 1024) doubles (not NULL).
 * -22 before any launch, nothing written: a null pointer other than gain / out (out_off may be NULL only with out), R outside [1, 64], a negative length or
 * offset, U outside [1, 8], T < 1 or U T > 1024, H outside [1, 480], a ceiling that is <= 0 or infinite (or whose float is), a row that would write outside
 * [0, out_cap), out overlapping wav, a workspace that is too small. */
int cbx_wave_limit_f32(const float* wav, const long* row_off, const int* row_len, int R, const float* gain, const double* ceiling, const float* tab, int U, int T,
                       const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap, void* stream);

/* ---- dialogue: SUM the rows of a batch into one waveform, each at a position of its own (added after ABI v16 without a version step: new function only).  The
 * reference has no counterpart: it returns one utterance of one voice (tts.py:272, mtl_tts.py:352, tts_turbo.py:320).  cbx_wave_join_f32 lays rows one after
 * another; here two rows may sound at the same time -- the next speaker comes in before the last one has finished -- and every row has a gain.
 * Rows as the other delivery entries take them: R in [1, 64] rows of row_len[r] >= 0 floats at wav + row_off[r]; row_off, row_len, start, flags and gain_idx are
 * HOST arrays that travel to the kernel by value.  start[r] >= 0 is the output index of row r's first sample, start[r] + row_len[r] <= out_len.
 * gain: G device floats, or NULL: every row at 1.  gain_idx[r] in [0, G): the gain row r uses (one per voice serves all of that voice's rows); NULL: r, G >= R.
 * ramp: `fade` device floats, cbx_wave_join_f32's ramp[i] = (2 i + 1) / (2 fade); NULL only when fade == 0.  flags[r] bit 0: row r fades in over its first
 * F_r = min(fade, n_r / 2) samples; bit 1: it fades out over its last F_r -- the rules of cbx_wave_join_f32.
 * Definition, in fp32, for every p in [0, out_len), the rows that cover p (start_r <= p < start_r + n_r) taken in ASCENDING r -- the order of summation:
 *   1. i = p - start_r; s_r = x_r[i] * g_r: one rounded multiply (no multiply at all when gain is NULL).
 *   2. bit 0 set and i < F_r: s_r = s_r * ramp[i];
 *   3. else bit 1 set and i >= n_r - F_r: s_r = s_r * ramp[n_r - 1 - i] (as in the join, the fade-in wins where the two meet).
 *   4. acc = out[p] when `accumulate` is set, else the first covering row's s_r itself;
 *   5. every further row: acc = acc + s_r, one rounded add each.  Products and sums are rounded separately: nothing is fused.
 *   6. out[p] = acc.  A sample that no row covers is written as +0.0 when accumulate == 0 and is not written when accumulate == 1.
 * Consequences: a sample covered by one row with a NULL gain holds exactly the bits cbx_wave_join_f32 would store.  Rows given in groups over several launches
 * (the first with accumulate = 0, the others with 1) give the values of one launch over all of them; only the sign of a zero may differ, where the first launch
 * covers nothing.  The result does not depend on the grid, the tile a sample falls into, or the alignment of wav, a row or out.  There are no atomics.  wav is
 * only read, and out must not overlap it.  Nothing outside out[0, out_len) is written.
 * Layout rule of a conversation (ops.mix_layout: the caller's, on the host): with front = pending = 0, an empty row gets start = front and changes nothing;
 * otherwise start_r = max(0, front + pending), front = max(front, start_r + n_r), pending = after[r] (a signed count of samples; negative: an overlap);
 * out_len = front.  With every after >= 0 this is cbx_wave_join_f32's layout with last = 1.
 * One workgroup of 256 threads per tile of 4096 outputs (wave_mix.hip), counted from the 16-byte boundary at or below out: a uniform loop over the rows finds
 * those that meet the tile, the sums are kept in registers in row order; 16-byte stores, 4-byte stores at the ragged ends; 16-byte loads where a row's source
 * address allows, else 4-byte.  A tile that no row meets writes zeros when accumulate == 0 and returns when accumulate == 1.  One launch; none, rc 0, when
 * out_len == 0.  Nothing synchronises the host.
 * -22 before any launch, nothing written: a null wav / row_off / row_len / start / flags / out, R outside [1, 64], a negative length, offset or start,
 * start + len > out_len, out_len < 0, fade < 0 or fade > 0 with ramp NULL, gain NULL with gain_idx given, G < 1 with gain given, an index outside [0, G), NULL
 * gain_idx with G < R, flags outside 0 .. 3, accumulate outside {0, 1}, out overlapping a non-empty row. */
int cbx_wave_mix_f32(const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, int R, const float* gain, int G,
                     const int* gain_idx, const float* ramp, int fade, float* out, long out_len, int accumulate, void* stream);

/* ---- stereo dialogue: the rows of a conversation summed into TWO planes, each voice at a place between left and right, then metered and limited as ONE
 * two-channel signal (added after ABI v16 without a version step: new functions only).  The reference has no counterpart: it returns one mono utterance of one
 * voice (tts.py:272, mtl_tts.py:352, tts_turbo.py:320).  Two steps cannot be had from the mono entries run once per channel: BS.1770-4 gates on the SUM of the
 * channels' block energies, and a limiter must apply ONE gain envelope to both channels, or a peak on the left moves the image.
 * cbx_wave_pan_mix_f32: cbx_wave_mix_f32 with two output planes, out (left) and out + plane_stride (right), out_len floats each, plane_stride >= out_len.  Rows,
 * start, flags, gain, gain_idx, ramp, fade, accumulate: the mono entry's.  pan: R x 2 HOST floats, pan[2 r] / pan[2 r + 1] the left / right gain of row r
 * (finite; the constant-power law is the caller's, ops.pan_gains), by value to the kernel like the other host arrays.
 * Definition, in fp32, for every p in [0, out_len), the rows that cover p taken in ASCENDING r -- the order of summation:
 *   1. - 3. of cbx_wave_mix_f32 give s_r: the balance gain, then the fade-in, else the fade-out.
 *   4. t_c = s_r * pan[r][c] for c = 0, 1: one rounded multiply per plane.
 *   5. acc_c = plane_c[p] when `accumulate` is set, else the first covering row's t_c itself; every further row: acc_c = acc_c + t_c, one rounded add each.
 *      Products and sums are rounded separately: nothing is fused.
 *   6. plane_c[p] = acc_c.  A sample that no row covers is written as +0.0 in both planes when accumulate == 0 and is not written when accumulate == 1.
 * Properties: pan[r] = {1, 1} for every row gives cbx_wave_mix_f32's bits in both planes (x * 1 is x).  Equal left and right gains give L == R bit for bit.  A
 * gain of 0 gives a plane of zeros (of either sign) for finite rows.  Rows given in groups over several launches behave as in the mono entry.  The result does
 * not depend on the grid, the tile a sample falls into, or the alignment of wav, a row, out or the right plane.  There are no atomics.  wav is only read; neither
 * plane may overlap it.  Nothing outside the two planes is written.
 * One launch reads every source sample once and writes both planes: one workgroup of 256 threads per tile of 4096 outputs per plane (wave_mix.hip, P = 2), counted
 * from the 16-byte boundary at or below out, both planes' sums in registers in row order; 16-byte accesses where the plane's own address allows, 4-byte accesses
 * at the ragged ends and in a plane that sits off the boundary.  None, rc 0, when out_len == 0.  Nothing synchronises the host.
 * -22 before any launch, nothing written: every refusal of cbx_wave_mix_f32, a null pan, a pan gain that is not finite, plane_stride < out_len, a plane
 * overlapping a non-empty row. */
int cbx_wave_pan_mix_f32(const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, const float* pan, int R, const float* gain,
                         int G, const int* gain_idx, const float* ramp, int fade, float* out, long plane_stride, long out_len, int accumulate, void* stream);
/* cbx_wave_loudness_ch_f32: cbx_wave_loudness_f32 for R / C signals of C consecutive rows each, C in {1, 2}: rows [g C, g C + C) are the channels of signal g and
 * have ONE length.  target: R / C HOST doubles; stats (R / C, 4) and gain (R / C), per signal.
 * Definition: the K-weighting, the segments and every segment energy E_(c,s) of channel c are cbx_wave_loudness_f32's, bit for bit -- the same three phases over
 * all R rows: one source, one arithmetic.  The row step runs once per signal:
 *   e_s = E_(0,s) + E_(1,s): one fp64 add in channel order, channel weights 1 (L and R of BS.1770-4); C = 1: e_s = E_(0,s) itself.
 *   z_j = (e_j + e_(j+1) + e_(j+2) + e_(j+3)) / (4 hop), then l_j, both gates, L and the gain exactly as written for cbx_wave_loudness_f32; a signal's segments
 *   from the first one whose e_s is not finite on count as NaN.
 *   Peak: the maximum over the channels of max |x| (NaN when a channel holds one); the ceiling limits peak g as there.
 * Properties: C = 1 is cbx_wave_loudness_f32 bit for bit.  Two equal channels read the mono loudness + 10 log10 2 (3.01 LU) up to rounding.  Swapped channels
 * give identical bits (an fp64 add commutes).  Fixed reduction order, no floating-point atomics.  Four launches, nothing synchronises the host.
 * ws: device workspace of ws_cap >= 6 * R * ceil(max_r n_r / hop) doubles (not NULL).
 * -22 before any launch, nothing written: every refusal of cbx_wave_loudness_f32, C outside {1, 2}, R no multiple of C, two channels of one signal of different
 * lengths. */
int cbx_wave_loudness_ch_f32(const float* wav, const long* row_off, const int* row_len, int R, int C, const double* coef, int hop, const double* target,
                             double ceiling, double* stats, float* gain, double* ws, long ws_cap, void* stream);
/* cbx_wave_limit_ch_f32: cbx_wave_limit_f32 with LINKED channels, for R / C signals of C consecutive rows of one length, C in {1, 2}.  gain: R / C device floats
 * (NULL: 1), ceiling: R / C HOST doubles (NaN: the signal is not limited), stats (R / C, 4): ONE pre-gain, ONE ceiling and one stats row per signal.  out_off:
 * R HOST longs, one per row.  tab, U, T, win, H: the mono entry's.
 * Definition, the steps of cbx_wave_limit_f32:
 *   1. - 2. per channel: u_c[i] = x_c[i] * gamma, y_c the oversampled u_c.
 *   3. m[i] = the maximum over the channels of the per-channel m_c[i]; NaN when any of them is.
 *   4. - 6. once per signal: c[i], the sliding minimum a[i], the smoothed g[i].
 *   7. out_c[i] = u_c[i] * g[i] per channel: both channels under the same envelope, the image does not move.
 * stats per signal: {max_i m[i], min_i g[i], the samples with g < 1, the samples with m > C32}.
 * Properties: C = 1 is cbx_wave_limit_f32 bit for bit.  Two equal channels return the mono limiter's output in both planes, bit for bit.  A peak in one channel
 * lowers the other by the same g.  The bound on |out_c| and the locality of cbx_wave_limit_f32 hold per channel.
 * One workgroup per tile of 1024 samples of a signal (wave_limit.hip, the mono kernel with C as a template parameter): the channels pass through the staging
 * buffer one after the other, the running maximum of m and every channel's own tile of u wait in LDS (8 KiB more for two channels); the fold launch is the mono
 * entry's.  Two launches, nothing synchronises the host.
 * ws: device workspace of ws_cap >= 4 * (R / C) * ceil(max_r n_r / 1024) doubles (not NULL).
 * -22 before any launch, nothing written: every refusal of cbx_wave_limit_f32, C outside {1, 2}, R no multiple of C, two channels of one signal of different
 * lengths. */
int cbx_wave_limit_ch_f32(const float* wav, const long* row_off, const int* row_len, int R, int C, const float* gain, const double* ceiling, const float* tab, int U,
                          int T, const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap, void* stream);

/* ---- music bed: lay the finished speech over a background and pull the background down while someone talks (added after ABI v16 without a version step: new
 * functions only).  The reference has no counterpart: it returns one utterance of one voice as the vocoder left it (tts.py:272, mtl_tts.py:352,
 * tts_turbo.py:320).  All signals are 24 kHz mono fp32.  Rows: R in [1, 64]; speech row r = s_len[r] floats at speech + s_off[r], its bed source b_len[r] floats
 * at bed + b_off[r], its output at out + out_off[r] (HOST arrays that travel to the kernels by value; 4-byte alignment is enough).  One set of control numbers
 * serves the call.
 * Inputs per row: s, n samples of speech; b, nb samples of bed source; lead, tail >= 0 samples of bed alone before and after the speech; L = gain[r], the bed
 * gain (R device floats; NULL: 1); thr = (float)threshold, threshold = 10^(threshold_db / 20) > 0; d = (float)duck, duck = 10^(duck_db / 20) in (0, 1]; pre,
 * post >= 0 control frames; S >= 1, the smoothing half-width in frames; loop (0 / 1) and xf, the cross-fade samples at the loop seam; fi, fo, the fade-in and
 * fade-out samples.  Two tables built by the CALLER in device memory: win = cbx_wave_limit_f32's window for H = S (2 S + 1 floats, w_k at win[k + S]) and ramp =
 * cbx_wave_join_f32's ramp[i] = (2 i + 1) / (2 xf), xf floats (NULL only when loop == 0 or xf == 0).
 * Definition, in fp32.  The output has N = lead + n + tail samples; s'[i] = s[i - lead] inside the speech, else 0.
 *   1. Control frames: Q = 240 samples (10 ms), F = ceil(N / Q).  p[f] = the max of |s'[i]| over frame f, NaN if the frame holds a NaN; act[f] = !(p[f] <= thr):
 *      a NaN frame is active.  A comparison of exact values: the same decision in every implementation.
 *   2. Hold: A[f] = the OR of act[j] for j in [f - post, f + pre], frames outside [0, F) inactive: the bed goes down pre frames before a word and stays down
 *      post frames after it (the whole signal is known).
 *   3. Smoothing: t[f] = d if A[f] else 1, and 1 outside [0, F); G[f] = 1 - sum_(k = -S .. S) w_k (1 - t[f + k]), 1 - t rounded once, then fmaf in the order
 *      k = -S .. S from 0.
 *   4. Per-sample gain: j = i - Q / 2, f0 = floor(j / Q), a = (float)(j - f0 Q) / 240.0f; g[i] = fmaf(a, G[f0 + 1] - G[f0], G[f0]) with G[-1] = G[0] and
 *      G[F] = G[F - 1].
 *   5. Bed read bed'(i): nb == 0: 0 (in either mode).  No loop: b[i] for i < nb, else 0; end = min(N, nb).  Loop: P = nb - xf, k = i / P, r = i % P; where
 *      k > 0 and r < xf the value is fmaf(ramp[r], b[r] - b[P + r], b[P + r]), else b[r]; end = N.  (end = 0 when nb == 0.)
 *   6. Envelope: up = i < fi ? (float)(i + 1) / (float)(fi + 1) : 1; dn = end - 1 - i < fo ? (float)(end - i) / (float)(fo + 1) : 1; e = up * dn, and 0 for
 *      i >= end.
 *   7. out[i] = fmaf((bed'(i) * e) * g[i], L, s'[i]): two rounded products, one fma.
 * Properties: with duck == 1 (0 dB) every 1 - t is exactly 0, so G and g are exactly 1; for a row with no active frame likewise (as the limiter's g is 1 wherever
 * nothing within its window is limited).  With L == 0 or nb == 0 the non-zero samples of out are s' bit for bit (a -0 may come back as +0).  Every value depends
 * on the row's samples alone, not on the tile, the grid or the rows' alignment, bit for bit.
 * stats: (R, 4) device doubles {L as applied, the frames with A[f], F, max |out| (NaN if the output row holds one; 0 for an empty row)}.
 * speech and bed are only read; the output rows may overlap neither; nothing outside the rows of out is written.  16-byte loads and stores inside a row where
 * the addresses allow, 4-byte accesses at the ragged ends; a quad that meets the loop seam is read sample by sample.
 * Three launches (wave_duck.hip): frames -- one WAVE per control frame, the wave maximum by cbx_xor_lane butterflies, the activity as 1.0f / 0.0f in ws --, apply
 * -- one workgroup of 256 threads per 1024 outputs of a row: the activity of the tile's frames +- 1 +- S and pre / post in LDS, then A, 1 - t and G for its <= 7
 * frames in the order above, then the stream --, fold -- the tiles' {max |out|, NaN flag, frames with A} per row (max and integer counts: exact in any order).
 * No floating-point atomics.  ONE launch, the fold, when every output row is empty.  Nothing synchronises the host.
 * ws: device workspace of ws_cap >= R * (ceil(max_r N_r / 240) + 4 * ceil(max_r N_r / 1024)) floats (not NULL).
 * -22 before any launch, nothing written: a null pointer other than gain / ramp / bed (bed may be NULL only when every bed row is empty, ramp only when loop == 0
 * or xf == 0), R outside [1, 64], a negative length, offset, lead or tail, more than 2^31 - 1 outputs in a row, a threshold that is not a positive finite float,
 * duck outside (0, 1], pre or post outside [0, 200], S outside [1, 100], xf, fi or fo outside [0, 24000], loop outside {0, 1}, a looped bed row with
 * 0 < nb <= 2 xf, a row that would write outside [0, out_cap), an output row overlapping a speech or bed row, a workspace that is too small. */
int cbx_wave_duck_f32(const float* speech, const long* s_off, const int* s_len, const float* bed, const long* b_off, const int* b_len, int R, const float* gain,
                      long lead, long tail, double threshold, double duck, int pre, int post, int S, const float* win, int loop, int xf, const float* ramp, int fi,
                      int fo, float* out, const long* out_off, long out_cap, double* stats, float* ws, long ws_cap, void* stream);
/* cbx_wave_duck_level_f32: the bed gain from two readings of the BS.1770-4 meter.  stats_speech / stats_bed: two (R, 4) stats blocks of cbx_wave_loudness_f32 in
 * measure-only mode (device doubles; column 0 = L in LUFS); level: R HOST doubles, the bed's level in LU relative to the speech (finite, within +- 200).
 * gain[r] = (float)10^((Ls_r + level_r - Lb_r) / 20), evaluated in fp64; where Ls_r or Lb_r is not finite (silence, or shorter than 0.4 s) gain[r] =
 * (float)10^(level_r / 20).  One small launch; nothing is synchronised.  -22 before the launch: a null pointer, R outside [1, 64], a level that is not finite. */
int cbx_wave_duck_level_f32(const double* stats_speech, const double* stats_bed, const double* level, int R, float* gain, void* stream);

/* ---- audio in: decode, mix down and resample the raw sample bytes of voice prompts and conversion sources, and find the silence at their ends, on the device
 * (added after ABI v16 without a version step: new functions only).  The mirror image of cbx_wave_format_f32.  It replaces frontend.load_wav / resample /
 * trim_silence (NumPy / SciPy on the host), which restate librosa.load, librosa.resample and librosa.effects.trim of the reference (tts.py:184-187,
 * s3gen.py:139, vc.py:88, voice_encoder.py:224).
 * cbx_wave_ingest: rows: R in [1, 64] rows of interleaved frames in ONE device allocation `raw`; row r = row_frames[r] frames of `channels` samples from the
 * byte raw + row_off[r] (HOST arrays, by value to the kernel).  encoding (CBX_WAVE_IN_*), decoded to fp32 as load_wav does: u8 (v - 128) / 128; s16 v / 32768;
 * s24 three bytes little-endian, v / 2^23; s32 (float)v / 2^31; f32 the bits; mulaw / alaw the ITU-T G.711 expansion to the 16-bit value, / 32768.  Mixdown: the
 * fp32 sum over the channels in channel order, then one IEEE division by (float)channels (one channel: the decoded value's bits).  Resampling by U / D = rate_out /
 * rate_in reduced, cbx_wave_format_f32's definition: hl = 10 max(U, D), h = U firwin(2 hl + 1, 1 / max(U, D), window = ("kaiser", 5.0)) built by the CALLER in
 * fp64, tab[p * T + j] = h[p + j U] (zero past 2 hl) in device memory, T = ceil((2 hl + 1) / U);
 *   c = m D + hl, p = c mod U, k = c div U, y[m] = sum_(j = 0 .. T - 1) tab[p][j] x[k - j], x = 0 outside [0, n), m in [0, ceil(n U / D))
 * by fmaf in the order j = 0 .. T - 1 from 0.  U = D = 1 (T = 1, tab may be NULL): decode and mixdown only.  No continuation state: a row is a whole signal.
 * out: ONE fp32 buffer of out_cap floats; row r's ceil(n_r U / D) outputs go to out + out_off[r] (HOST array); nothing else is written, nothing outside a row's
 * bytes is read.  16-byte loads where a row's address allows, byte loads at the ragged ends.  All positions are 64-bit.  One launch (none when every row is empty).
 * Caps: a tile's span 255 D / U + T + 1 <= CBX_WAVE_INGEST_MAX_SPAN frames and U T <= CBX_WAVE_INGEST_MAX_TAB floats -- every pair of {8000, 11025, 12000, 16000,
 * 22050, 24000, 32000, 44100, 48000, 88200, 96000} -> {16000, 24000} fits (largest span 96000 -> 16000: 1652; largest table 11025 -> 16000: 640 x 21).
 * -22 before any launch: a null pointer, R outside [1, 64], a negative frame count or offset, an offset (or `raw`) that is not a multiple of the sample size (1
 * for u8 / mulaw / alaw / s24, 2 for s16, 4 for s32 / f32), channels outside [1, 8], an unknown encoding, U / D not reduced, T not that of U / D, a span or table
 * over the caps, a row that would write outside [0, out_cap), out_cap below the sum of the rows' outputs. */
#define CBX_WAVE_IN_U8 0
#define CBX_WAVE_IN_S16 1
#define CBX_WAVE_IN_S24 2
#define CBX_WAVE_IN_S32 3
#define CBX_WAVE_IN_F32 4
#define CBX_WAVE_IN_MULAW 5
#define CBX_WAVE_IN_ALAW 6
#define CBX_WAVE_INGEST_MAX_SPAN 2048
#define CBX_WAVE_INGEST_MAX_TAB 16384
int cbx_wave_ingest(const void* raw, const long* row_off, const long* row_frames, int R, int encoding, int channels, const float* tab, int U, int D, int T, float* out,
                    const long* out_off, long out_cap, void* stream);
/* cbx_wave_trim_edges_f32: frontend.trim_silence (librosa.effects.trim) for R in [1, 64] fp32 rows, rows as cbx_wave_join_f32 takes them.  Frames of 2048 samples
 * at hop 512 over the row padded by 1024 zeros on either side: F = 1 + n / 512 frames, frame f covers samples [512 f - 1024, 512 f + 1024).  ms_f = the fp64 sum
 * of squares / 2048, floored at 1e-20 (trim_silence floors the RMS at 1e-10: in an all-zero row every frame is level with the loudest, and all of it is kept,
 * as librosa keeps it); a frame passes iff ms_f > max_f ms_f * ratio, compared in fp64 (ratio = 10^(-top_db / 10), computed by the caller in fp64).  With f0 / f1
 * the first / last passing frame: start = 512 f0, stop = min(n, 512 (f1 + 1)); no passing frame: (0, 0).  edges: (R, 2) int32 device table {start, stop}.  Sums
 * per block of 512 samples, one wave per block in a fixed order, a frame = its four blocks added in ascending order: no floating-point atomics, independent of
 * the grid and of the row's alignment.  Two launches.  ws: device workspace of ws_cap >= R * ceil(max_r n_r / 512) doubles (not NULL).
 * -22 before any launch: a null pointer, R outside [1, 64], a negative length or offset, ratio negative / not finite, a workspace that is too small. */
int cbx_wave_trim_edges_f32(const float* wav, const long* row_off, const int* row_len, int R, double ratio, int* edges, double* ws, long ws_cap, void* stream);

/* ---- voice-prompt / voice-conversion front-end ----
 * Contractions (framed DFT as a GEMM over overlapping waveform rows, mel filterbanks, Conv1d/Conv2d-as-Toeplitz, attention, LSTM
 * projections) use cbx_gemm_f32 / cbx_flash_attn_f32 / cbx_gemv_f32; these are the remaining element-wise / reduction passes. */
/* depthwise Conv1d, channel-last: y[b][t][c] = sum_k w[c][k] x[b][t+k-pad_left][c] (+ x[b][t][c]); rows >= lens[b] are zero.
 * S3TokenizerV2 FSMN memory block (third-party s3tokenizer.model_v2, Conv1d k31 groups=C; parity unpinned). */
int cbx_dwconv1d_f32(const float* x, const float* w, float* y, const int* lens, int B, int T, int C, int taps, int pad_left,
                     long ldx, long ldy, long x_sb, long y_sb, int add_input, void* stream);
/* torch.nn.LSTM cell, gates (i,f,g,o) = pre + hh (voice_encoder.py:139-163: nn.LSTM(40, 256, 3 layers)) */
int cbx_lstm_cell_f32(const float* pre, const float* hh, float* c, float* h, int B, int H, long ld_pre, long ld_hh, long ldc,
                      long ldh, void* stream);
/* y = act(x * scale[c] + shift[c]): eval BatchNorm + ReLU that PRECEDES a conv in CAMPPlus (xvector.py:136-151,262-266) */
int cbx_affine_act_f32(const float* x, float* y, const float* scale, const float* shift, long rows, int C, long ldx, long ldy,
                       int act, void* stream);
/* spec row [re(0..F-1) | im(0..F-1)] -> |.|^2 (mode 0: s3tokenizer.py:161, voice_encoder/melspec.py:35-39) or
 * sqrt(|.|^2 + eps) (mode 1: s3gen/utils/mel.py:80) */
int cbx_cplx_power_f32(const float* spec, float* out, long rows, int F, long ld_spec, long ld_out, int mode, float eps, void* stream);
#define CBX_UN_LOG_CLAMP 1     /* log(max(x, a))                 utils/mel.py:18-19 */
#define CBX_UN_LOG10_CLAMP 2   /* log10(max(x, a))               s3tokenizer.py:165 */
#define CBX_UN_FLOOR_AFFINE 3  /* (max(x, *dev_scalar - a) + b) / b   s3tokenizer.py:166-167 */
#define CBX_UN_AFFINE 4        /* a x + b */
int cbx_unary_f32(const float* x, float* y, long rows, int C, long ldx, long ldy, int op, float a, float b, const float* dev_scalar,
                  void* stream);
/* out[0] = max over a 2-D strided block (log_spec.max() of s3tokenizer.py:166, kept on the device as CBX_UN_FLOOR_AFFINE's dev_scalar) */
int cbx_reduce_max_f32(const float* x, float* out, long rows, int C, long ldx, void* stream);
/* CAMLayer context (xvector.py:204-231): ctx[s][c] = mean_t x + mean over segment s (avg_pool1d ceil_mode), s = t / seg_len */
int cbx_seg_context_f32(const float* x, float* ctx, int T, int C, int seg_len, long ldx, long ldc, void* stream);
/* y[t][c] *= sigmoid(m[t / seg_len][c])  (xvector.py:209-213) */
int cbx_seg_gate_mul_f32(float* y, const float* m, int T, int C, int seg_len, long ldy, long ldm, void* stream);
/* StatsPool (xvector.py:153-165): out = [mean_t | unbiased std_t] */
int cbx_stats_pool_f32(const float* x, float* out, int T, int C, long ldx, void* stream);
/* FSQ codebook index of S3TokenizerV2 (third-party; restated: tanh * 0.999 -> round -> +1 -> base-3 digits) */
int cbx_fsq_index(const float* h, long long* idx, long rows, long ldh, void* stream);

#ifdef __cplusplus
}
#endif
#endif
