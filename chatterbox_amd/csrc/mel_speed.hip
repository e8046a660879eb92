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
#include <math.h>

#include "cbx_common.h"

namespace {

// (1 - l) a + l b: 1 - l, l b and the fma round once each
__device__ __forceinline__ float blend(float a, float b, float l) { return fmaf(1.0f - l, a, l * b); }

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
        if (VEC == 4) {
            *reinterpret_cast<f32x4*>(o) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        } else {
            *o = 0.0f;
        }
        return;
    }
    const double x = fmax(0.0, ((double)j + 0.5) * rate[b] - 0.5);  // (a NaN rate gives 0; an infinite one is cut by the min below)
    const double fx = floor(x);
    const int i0 = fx < (double)(M - 1) ? (int)fx : M - 1;
    const int i1 = i0 + 1 < M ? i0 + 1 : M - 1;
    const float l = (float)fmin(x - (double)i0, 1.0);
    const float* r0 = in + (long)b * in_sb + (long)i0 * in_ld + c;
    const float* r1 = in + (long)b * in_sb + (long)i1 * in_ld + c;
    if (VEC == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(r0), bb = *reinterpret_cast<const f32x4*>(r1);
        *reinterpret_cast<f32x4*>(o) = f32x4{blend(a[0], bb[0], l), blend(a[1], bb[1], l), blend(a[2], bb[2], l), blend(a[3], bb[3], l)};
    } else {
        *o = blend(*r0, *r1, l);
    }
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
