// End of a round of chunked ("streaming") synthesis: one launch for all B utterances hands out the round's NEW samples, cross-fades their head with the
// tail the previous round kept back, and keeps this round's tail for the next one.  The schedule is this build's own (engine.py synthesize_stream; the
// reference is non-streaming, of its hooks only `cache_source` works: hifigan.py:467-472); the kernel replaces the per-utterance slice / clone / lerp of
// the host loop and is bit-identical to it.
#include "cbx_common.h"

namespace {

// torch: tail * (1.0 - ramp) + new * ramp -- four roundings, no fma (both builds compile with -ffp-contract=on, which would fuse the one-line form)
__device__ __forceinline__ float crossfade(float tail, float x, float ramp) {
#pragma clang fp contract(off)
    const float om = 1.0f - ramp;
    const float a = tail * om;
    const float c = x * ramp;
    return a + c;
}

// grid (ceil(max(max_new, fade) / 256), B).  All positions are ABSOLUTE samples of the utterance; wav[b][q] holds sample origin + q.
__global__ __launch_bounds__(256) void stream_emit_kernel(const float* __restrict__ wav, long L, long origin, const int* __restrict__ emitted,
                                                          const int* __restrict__ end, const int* __restrict__ avail, const float* __restrict__ tail_in,
                                                          const int* __restrict__ tail_len, const float* __restrict__ ramp, int fade,
                                                          float* __restrict__ out, long max_new, float* __restrict__ tail_out) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long em = emitted[b], en = end[b], av = avail[b];
    const float* w = wav + (long)b * L;
    if (i < en - em && i < max_new) {  // new samples [emitted, end)
        const long q = em - origin + i;
        float v = (q >= 0 && q < L) ? w[q] : 0.0f;
        if (i < fade && i < (long)tail_len[b]) v = crossfade(tail_in[(long)b * fade + i], v, ramp[i]);
        out[(long)b * max_new + i] = v;
    }
    if (i < fade) {  // the next tail [end, min(avail, end + fade))
        const long stop = av < en + fade ? av : en + fade;
        const long q = en - origin + i;
        if (en + i < stop && q >= 0 && q < L) tail_out[(long)b * fade + i] = w[q];
    }
}

}  // namespace

extern "C" int cbx_stream_emit_f32(const float* wav, long ld_wav, long origin, const int* emitted, const int* end, const int* avail,
                                   const float* tail_in, const int* tail_len, const float* ramp, int fade, float* out, long max_new,
                                   float* tail_out, int B, void* stream) {
    CBX_REQUIRE(wav && emitted && end && avail && B > 0 && ld_wav > 0 && origin >= 0 && fade >= 0 && max_new >= 0, "stream_emit: bad args");
    CBX_REQUIRE(max_new == 0 || out, "stream_emit: no output for %ld new samples", max_new);
    CBX_REQUIRE(fade == 0 || (tail_in && tail_len && ramp && tail_out && tail_in != tail_out), "stream_emit: a fade needs tail_in, tail_len, ramp and a distinct tail_out");
    const long n = max_new > fade ? max_new : fade;
    if (n == 0) return 0;
    hipLaunchKernelGGL(stream_emit_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, wav, ld_wav, origin, emitted, end,
                       avail, tail_in, tail_len, ramp, fade, out, max_new, tail_out);
    return cbx_check_launch("stream_emit");
}
