// Speed control (cbx_mel_time_scale_f32, include/cbx.h): linear interpolation of the mel along time between the flow decoder and the vocoder.  The reference
// leaves it out -- models/s3gen/s3gen.py:289 reads "ignoring the speed control (mel interpolation) ... for now" -- and hands the flow's mel to the vocoder as it
// is; the upstream S3Gen family stretches the mel there, and the F0 predictor then runs on the stretched mel, so the pitch is kept.
//
// For a row of M valid frames and rate s, output frame j samples the input at x = max(0, (j + 0.5) s - 0.5), EVALUATED IN FP64 (one fp64 multiply-add per
// thread): i0 = min(floor(x), M - 1), i1 = min(i0 + 1, M - 1), l = x - i0, out = (1 - l) in[i0] + l in[i1] in fp32.  That is F.interpolate(mode="linear",
// align_corners=False, scale_factor=1 / s, recompute_scale_factor=False) with the position in fp64 (torch's fp32 position is off by 3.9e-3 at 4000 frames and
// s = 0.9) and without its copy shortcut when the lengths agree.  The map depends on j and s only, not on M.
//
// Memory-bound and tiny: one thread per output float4 (two 16-byte loads, one 16-byte store) when pointers and strides allow 16-byte access, one thread per
// float otherwise; plain loads and stores, no LDS.  Frames [out_lens[b], T_out) are written as zeros; columns [C, row stride) are not touched; input frames from
// in_lens[b] on are never read.
//
// cbx_mel_time_scale_win_f32 evaluates a WINDOW of the same map for the streaming rounds (engine._stream_rounds(speed=)): output frame jj is absolute frame
// j0 + jj, the input's frame 0 is absolute frame i_org, the position comes from the one device function both kernels share (mel_taps), and the tap indices are
// clamped into the window whatever the host passes.
#include <math.h>

#include "cbx_common.h"

namespace {

// The taps of ABSOLUTE output frame j at rate s, for an input whose frame 0 is absolute frame i_org and which holds M frames: THE position expression of both
// kernels -- x = max(0, (j + 0.5) s - 0.5) as one contracted fp64 multiply-add -- so a window of the map (mel_time_scale_win_kernel) reproduces the whole map's
// bits.  The tap rule and the blend live in cbx_common.h, where mel_warp.hip (a piecewise-linear map) shares them.
typedef cbx_mel_taps_t mel_taps_t;
__device__ __forceinline__ mel_taps_t mel_taps(long j, double s, long i_org, int M) {
    const double x = fmax(0.0, ((double)j + 0.5) * s - 0.5);  // (a NaN rate gives 0; an infinite one is cut by the clamp of the taps)
    return cbx_mel_taps_at(x, i_org, M);
}

template <int VEC>
__device__ __forceinline__ void blend_store(float* o, const float* r0, const float* r1, float l) {
    cbx_mel_blend_store<VEC>(o, r0, r1, l);
}

// grid (ceil(T_out * CV / 256), B): thread = (output frame j, channel group c) of batch row blockIdx.y; CV = C / VEC channel groups of VEC floats
template <int VEC>
__global__ __launch_bounds__(256) void mel_time_scale_kernel(const float* __restrict__ in, long in_sb, long in_ld, int T_in, const int* __restrict__ in_lens,
                                                             const double* __restrict__ rate, float* __restrict__ out, long out_sb, long out_ld, int T_out,
                                                             const int* __restrict__ out_lens, int CV) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)T_out * CV) return;
    const int b = blockIdx.y;
    const int j = (int)(t / CV), c = (int)(t - (long)j * CV) * VEC;
    int M = in_lens ? in_lens[b] : T_in;
    M = M < T_in ? M : T_in;  // never read past the buffer, whatever in_lens holds
    int O = out_lens[b];
    O = O < T_out ? O : T_out;  // the host entry cannot see out_lens: clamped here
    float* o = out + (long)b * out_sb + (long)j * out_ld + c;
    if (j >= O || M <= 0) {
        blend_store<VEC>(o, nullptr, nullptr, 0.0f);
        return;
    }
    const mel_taps_t p = mel_taps(j, rate[b], 0, M);
    const float* row = in + (long)b * in_sb + c;
    blend_store<VEC>(o, row + (long)p.i0 * in_ld, row + (long)p.i1 * in_ld, p.l);
}

// A WINDOW of the same map (cbx_mel_time_scale_win_f32): output frame jj is absolute frame j0 + jj, input frame 0 is absolute frame i_org, one rate for all rows.
// Same grid, same dispatch, same loads and stores as the kernel above.
template <int VEC>
__global__ __launch_bounds__(256) void mel_time_scale_win_kernel(const float* __restrict__ in, long in_sb, long in_ld, int T_in, const int* __restrict__ in_lens,
                                                                 double rate, long j0, long i_org, float* __restrict__ out, long out_sb, long out_ld, int T_out,
                                                                 const int* __restrict__ out_lens, int CV) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)T_out * CV) return;
    const int b = blockIdx.y;
    const int jj = (int)(t / CV), c = (int)(t - (long)jj * CV) * VEC;
    int M = in_lens ? in_lens[b] : T_in;
    M = M < T_in ? M : T_in;  // never read past the buffer, whatever in_lens holds
    int O = out_lens[b];
    O = O < T_out ? O : T_out;
    float* o = out + (long)b * out_sb + (long)jj * out_ld + c;
    if (jj >= O || M <= 0) {
        blend_store<VEC>(o, nullptr, nullptr, 0.0f);
        return;
    }
    const mel_taps_t p = mel_taps(j0 + jj, rate, i_org, M);  // indices into the window, clamped to [0, M - 1] whatever the host passed
    const float* row = in + (long)b * in_sb + c;
    blend_store<VEC>(o, row + (long)p.i0 * in_ld, row + (long)p.i1 * in_ld, p.l);
}

}  // namespace

extern "C" int cbx_mel_time_scale_f32(const float* in, long in_sb, long in_ld, int T_in, const int* in_lens, const double* rate, float* out, long out_sb,
                                      long out_ld, int T_out, const int* out_lens, int B, int C, void* stream) {
    CBX_REQUIRE(in && rate && out && out_lens, "mel_time_scale: null pointer");
    CBX_REQUIRE(C > 0, "mel_time_scale: C = %d", C);
    CBX_REQUIRE(in_ld >= C && out_ld >= C && in_sb >= C && out_sb >= C, "mel_time_scale: a stride is below C = %d (in %ld / %ld, out %ld / %ld)", C, in_sb, in_ld,
                out_sb, out_ld);
    CBX_REQUIRE(B >= 0 && B <= 65535 && T_in >= 0 && T_out >= 0, "mel_time_scale: bad shape (B %d, T_in %d, T_out %d)", B, T_in, T_out);
    if (B == 0 || T_out == 0) return 0;
    const bool vec = C % 4 == 0 && in_ld % 4 == 0 && out_ld % 4 == 0 && in_sb % 4 == 0 && out_sb % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const int CV = vec ? C / 4 : C;
    const long n = (long)T_out * CV, gx = (n + 255) / 256;
    CBX_REQUIRE(gx <= 0x7fffffffl, "mel_time_scale: T_out * C too large for one launch");
    if (vec)
        hipLaunchKernelGGL(mel_time_scale_kernel<4>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, in_sb, in_ld, T_in, in_lens, rate, out,
                           out_sb, out_ld, T_out, out_lens, CV);
    else
        hipLaunchKernelGGL(mel_time_scale_kernel<1>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, in_sb, in_ld, T_in, in_lens, rate, out,
                           out_sb, out_ld, T_out, out_lens, CV);
    return cbx_check_launch("mel_time_scale");
}

extern "C" int cbx_mel_time_scale_win_f32(const float* in, long in_sb, long in_ld, int T_in, const int* in_lens, double rate, long j0, long i_org, float* out,
                                          long out_sb, long out_ld, int T_out, const int* out_lens, int B, int C, void* stream) {
    CBX_REQUIRE(in && out && out_lens, "mel_time_scale_win: null pointer");
    CBX_REQUIRE(C > 0, "mel_time_scale_win: C = %d", C);
    CBX_REQUIRE(in_ld >= C && out_ld >= C && in_sb >= C && out_sb >= C, "mel_time_scale_win: a stride is below C = %d (in %ld / %ld, out %ld / %ld)", C, in_sb,
                in_ld, out_sb, out_ld);
    CBX_REQUIRE(B >= 0 && B <= 65535 && T_in >= 0 && T_out >= 0, "mel_time_scale_win: bad shape (B %d, T_in %d, T_out %d)", B, T_in, T_out);
    CBX_REQUIRE(rate > 0.0 && rate < INFINITY && j0 >= 0 && i_org >= 0 && j0 < (1l << 40) && i_org < (1l << 40),
                "mel_time_scale_win: bad window (rate %g, j0 %ld, i_org %ld)", rate, j0, i_org);
    if (B == 0 || T_out == 0) return 0;
    const bool vec = C % 4 == 0 && in_ld % 4 == 0 && out_ld % 4 == 0 && in_sb % 4 == 0 && out_sb % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const int CV = vec ? C / 4 : C;
    const long n = (long)T_out * CV, gx = (n + 255) / 256;
    CBX_REQUIRE(gx <= 0x7fffffffl, "mel_time_scale_win: T_out * C too large for one launch");
    if (vec)
        hipLaunchKernelGGL(mel_time_scale_win_kernel<4>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, in_sb, in_ld, T_in, in_lens, rate, j0,
                           i_org, out, out_sb, out_ld, T_out, out_lens, CV);
    else
        hipLaunchKernelGGL(mel_time_scale_win_kernel<1>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, in_sb, in_ld, T_in, in_lens, rate, j0,
                           i_org, out, out_sb, out_ld, T_out, out_lens, CV);
    return cbx_check_launch("mel_time_scale_win");
}
