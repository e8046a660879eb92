// Stage-level C entry points of the T3-Turbo / Nano decode loop (GPT-2 backbone; reference models/t3/t3.py:392-468, T3.inference_turbo): one token step
// for every row (cbx_gpt2_decode_step) and the token loop around it (cbx_gpt2_loop_*), the GPT-2 counterparts of cbx_t3_decode_step / cbx_t3_loop_*
// (t3_step.hip).  The step issues the launches chatterbox_amd/t3_turbo.py issues one by one (T3TurboEngine._forward_decode_row resp. _forward_decode_v2,
// then _sample), in the same order and with the same arguments: it only sequences kernel-level entry points of this library, all state is caller-owned
// device memory described by cbx_gpt2_step_t.
#include "cbx_common.h"

static int gpt2_step_row(const cbx_gpt2_step_t* d, void* stream) {
    const int D = d->dim, H = d->n_heads, B = d->rows;
    int rc = cbx_embed_f32(d->next_ids, d->speech_emb, d->wpe, d->positions, d->x, B, D, D, 1.0f, 1, stream);
    if (rc) return rc;
    cbx_gemv_row_t g;
    // ops.gemv_row: eps only travels with a LayerNorm operand, ldx / ldr only with their operands
    auto row = [&](const float* x, long ldx, const float* W, const float* bias, const float* res, float* out, long ldo, int N, int K, const float* ln_w,
                   const float* ln_b, int act) {
        g = cbx_gemv_row_t{};
        g.x = x, g.ldx = x ? ldx : 0, g.W = W, g.bias = bias, g.res = res, g.ldr = res ? ldo : 0, g.out = out, g.ldo = ldo;
        g.ln_w = ln_w, g.ln_b = ln_b, g.eps = ln_w ? d->eps : 0.0f;
        g.N = N, g.K = K, g.ldw = K, g.act = act, g.M = B;
    };
    cbx_attn_parts_t ap{};
    ap.qkv = d->qkv, ap.positions = d->positions, ap.parts = d->parts, ap.rows = B, ap.n_heads = H, ap.n_splits = d->n_splits, ap.chunks = d->chunks;
    ap.max_ctx = d->max_ctx, ap.ld_qkv = 3 * D, ap.cache_row_stride = d->kv_row_stride, ap.cache_head_stride = d->kv_head_stride, ap.scale = d->attn_scale;
    for (int i = 0; i < d->n_layers; ++i) {
        const cbx_gpt2_layer_t& L = d->layers[i];
        row(d->x, D, L.wqkv, L.bqkv, nullptr, d->qkv, 3 * D, 3 * D, D, L.ln1_w, L.ln1_b, CBX_ACT_NONE);
        if ((rc = cbx_gemv_row_f32(&g, stream))) return rc;
        ap.kc = d->kc + i * d->kv_layer_stride, ap.vc = d->vc + i * d->kv_layer_stride;
        if ((rc = cbx_decode_attn_parts(&ap, stream))) return rc;
        row(nullptr, 0, L.wo, L.bo, d->x, d->x, D, D, D, nullptr, nullptr, CBX_ACT_NONE);
        g.parts = d->parts, g.n_parts = d->n_splits, g.n_heads = H, g.parts_row_stride = (long)H * d->n_splits * CBX_ATTN_PART_REC;
        if ((rc = cbx_gemv_row_f32(&g, stream))) return rc;
        row(d->x, D, L.wfc, L.bfc, nullptr, d->g, 4 * D, 4 * D, D, L.ln2_w, L.ln2_b, CBX_ACT_GELU_TANH);
        if ((rc = cbx_gemv_row_f32(&g, stream))) return rc;
        row(d->g, 4 * D, L.wpr, L.bpr, d->x, d->x, D, D, 4 * D, nullptr, nullptr, CBX_ACT_NONE);
        if ((rc = cbx_gemv_row_f32(&g, stream))) return rc;
    }
    row(d->x, D, d->head, d->head_b, nullptr, d->logits, d->ld_logits, d->vocab, D, d->lnf_w, d->lnf_b, CBX_ACT_NONE);
    return cbx_gemv_row_f32(&g, stream);
}

static int gpt2_step_packed(const cbx_gpt2_step_t* d, void* stream) {
    const int D = d->dim, H = d->n_heads, B = d->rows;
    float* cur = d->x_a;
    float* nxt = d->x_b;
    int rc = cbx_embed_f32(d->next_ids, d->speech_emb, d->wpe, d->positions, cur, B, D, D, 1.0f, 3, stream);
    if (rc) return rc;
    cbx_gemv_t g;
    auto base = [&](const float* x, long ldx, const float* W, float* out, long ldo, int N, int K, int nw) {
        g = cbx_gemv_t{};
        g.x = x, g.W = W, g.out = out, g.M = B, g.N = N, g.K = K, g.ksplit = 1, g.nw = nw, g.ldx = ldx, g.ldw = K, g.ldo = ldo;
        g.w_packed = g.x_packed = 1, g.eps = d->eps, g.flags = d->gemv_flags;
    };
    cbx_decode_attn_t da{};
    da.qkv = d->qkv, da.positions = d->positions, da.o = d->att, da.rows = B, da.n_heads = H, da.ld_qkv = 3 * D, da.o_ld = D, da.o_packed = 1;
    da.cache_row_stride = d->kv_row_stride, da.cache_head_stride = d->kv_head_stride, da.scale = d->attn_scale;
    da.unroll = d->da_unroll, da.pipeline = d->da_pipeline, da.split_min = d->da_split_min;
    da.split_ws = d->da_ws, da.split_cnt = d->da_cnt, da.split_pairs = d->da_pairs;
    const long img = (long)((B + 15) / 16 * 16) * D;  // floats per packed residual / partial image
    bool pending = false;                             // split-K partial images of the previous mlp c_proj waiting to be summed
    for (int i = 0; i < d->n_layers; ++i) {
        const cbx_gpt2_layer_t& L = d->layers[i];
        const cbx_gpt2_packed_layer_t& P = d->packed[i];
        base(cur, D, P.wqkv, d->qkv, 3 * D, 3 * D, D, 8);
        g.norm_w = L.ln1_w, g.ln_cw = P.qkv_cw, g.ln_cb = P.qkv_cb, g.half_tile = d->qkv_tile;
        if (pending) g.n_xpart = d->d_ksplit, g.xpart = d->pd, g.xpart_stride = img, g.x_out = nxt;
        if ((rc = cbx_gemv_f32(&g, stream))) return rc;
        if (pending) {
            float* t = cur;
            cur = nxt, nxt = t;
        }
        da.kc = d->kc + i * d->kv_layer_stride, da.vc = d->vc + i * d->kv_layer_stride;
        if ((rc = cbx_decode_attn_rope(&da, stream))) return rc;
        base(d->att, D, P.wo, cur, D, D, D, d->o_nw);
        g.bias = L.bo, g.res = cur, g.out_packed = 1, g.half_tile = d->od_tile;
        if ((rc = cbx_gemv_f32(&g, stream))) return rc;
        base(cur, D, P.wfc, d->g_pk, 4 * D, 4 * D, D, 8);
        g.norm_w = L.ln2_w, g.ln_cw = P.fc_cw, g.ln_cb = P.fc_cb, g.act = CBX_ACT_GELU_TANH, g.out_packed = 1;
        if ((rc = cbx_gemv_f32(&g, stream))) return rc;
        if (d->d_ksplit > 1) {
            base(d->g_pk, 4 * D, P.wpr, d->pd, D, D, 4 * D, d->d_nw);
            g.ksplit = d->d_ksplit, g.part_stride = img;
        } else {  // no partial images: the projection adds bias + residual in its epilogue, in place
            base(d->g_pk, 4 * D, P.wpr, cur, D, D, 4 * D, d->d_nw);
            g.res = cur;
        }
        g.bias = L.bpr, g.out_packed = 1, g.half_tile = d->od_tile;
        if ((rc = cbx_gemv_f32(&g, stream))) return rc;
        pending = d->d_ksplit > 1;
    }
    base(cur, D, d->head_pk, d->logits, d->ld_logits, d->vocab, D, 8);
    g.norm_w = d->lnf_w, g.ln_cw = d->head_cw, g.ln_cb = d->head_cb, g.col_tiles = d->head_ct;
    if (pending) g.n_xpart = d->d_ksplit, g.xpart = d->pd, g.xpart_stride = img, g.x_out = nullptr;
    return cbx_gemv_f32(&g, stream);
}

extern "C" int cbx_gpt2_decode_step(const cbx_gpt2_step_t* d, void* stream) {
    CBX_REQUIRE(d && d->layers && d->n_layers > 0, "gpt2_decode_step: null descriptor");
    CBX_REQUIRE(d->rows >= 1 && d->rows <= 16, "gpt2_decode_step: rows=%d (more than 16 rows run the 7-launch form, which this entry point does not serve)", d->rows);
    CBX_REQUIRE(d->dim == d->n_heads * 64 && d->vocab > 0 && d->next_ids && d->positions && d->kc && d->vc && d->qkv && d->logits,
                "gpt2_decode_step: bad shape (head_dim 64) or null buffer");
    int rc;
    if (d->row_path) {
        CBX_REQUIRE(d->rows <= 4 && d->x && d->g && d->parts && d->head && d->n_splits >= 1, "gpt2_decode_step: the row path serves <= 4 rows (x, g, parts, head)");
        rc = gpt2_step_row(d, stream);
    } else {
        CBX_REQUIRE(d->packed && d->x_a && d->x_b && d->att && d->g_pk && d->head_pk && d->head_cw && d->head_cb,
                    "gpt2_decode_step: the packed path needs packed layers, x_a / x_b / att / g_pk and the packed head");
        CBX_REQUIRE(d->d_ksplit == 1 || ((d->d_ksplit == 2 || d->d_ksplit == 4) && d->pd), "gpt2_decode_step: d_ksplit must be 1, 2 or 4 (2, 4: pd)");
        rc = gpt2_step_packed(d, stream);
    }
    if (rc) return rc;
    return d->sampler ? cbx_t3_sample(d->sampler, stream) : 0;
}

// ---- The token loop in C (include/cbx.h): the contract of cbx_t3_loop_* (t3_step.hip) -- cbx_loop<> of cbx_common.h around cbx_gpt2_decode_step; the handle
// owns a copy of the descriptor's `packed` array as well.
struct cbx_gpt2_loop : cbx_loop<cbx_gpt2_step_t> {
    std::vector<cbx_gpt2_packed_layer_t> packed;
    void adopt_arrays() {
        if (!step.packed) return;
        packed.assign(step.packed, step.packed + step.n_layers);
        step.packed = packed.data();
    }
};

extern "C" int cbx_gpt2_loop_create(const cbx_gpt2_step_t* step, void* stream, cbx_gpt2_loop_t** out) {
    (void)stream;  // the capture runs on a stream of the library's own
    return cbx_loop_create("gpt2", cbx_gpt2_decode_step, step, out);
}

extern "C" int cbx_gpt2_loop_run(cbx_gpt2_loop_t* h, int n_steps, int poll_every, void* stream, int* steps_run) {
    return cbx_loop_run("gpt2", cbx_gpt2_decode_step, h, n_steps, poll_every, stream, steps_run);
}

extern "C" int cbx_gpt2_loop_destroy(cbx_gpt2_loop_t* h) { return cbx_loop_destroy(h); }
