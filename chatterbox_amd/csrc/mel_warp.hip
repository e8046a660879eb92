// Timing control (cbx_mel_time_warp_f32, include/cbx.h): a PIECEWISE-LINEAR time map of the mel between the flow decoder and the vocoder, where mel_speed.hip
// applies one rate per row.  The reference has neither -- models/s3gen/s3gen.py:289 reads "ignoring the speed control (mel interpolation) ... for now" -- and the
// F0 predictor runs on the warped mel, so the pitch is kept, as with speed=.
//
// Row b carries segments [seg_off[b], seg_off[b + 1]) of a packed table: segment k starts at output frame seg_o[k] (increasing, the first 0), output EDGE seg_o[k]
// maps to input EDGE seg_a[k] (fp64), and inside the segment the rate is seg_s[k] (fp64).  Output frame j belongs to the last segment k with seg_o[k] <= j and
// samples the input at, IN FP64,
//     x = max(0, seg_a[k] + (((j - seg_o[k]) + 0.5) seg_s[k] - 0.5))
// -- the pixel-centre convention of mel_speed.hip made piecewise; the product term is written as mel_speed.hip writes it, one contracted fp64 multiply-add (the
// build contracts inside an expression only, so the sum with seg_a stays a separate add), and the taps and the blend are cbx_mel_taps_at / cbx_mel_blend_store of
// cbx_common.h, which both files share: a one-segment table (0, 0.0, s) gives 0.0 + that term, which is that term, and so reproduces cbx_mel_time_scale_f32 at
// rate s bit for bit.  The map is continuous when seg_a[k + 1] = seg_a[k] + (seg_o[k + 1] - seg_o[k]) seg_s[k];
// the kernel does not need it to be.
//
// MEMORY SAFETY does not depend on the table: the taps are clamped into [0, M - 1] whatever x is (NaN, infinite, negative), and the segment search never leaves
// [seg_off[b], seg_off[b + 1]), a range the host entry has checked against the table's length (seg_off is a HOST array and travels by value, as wave_join.hip's
// row table does: at most 64 rows).  A malformed table (decreasing seg_o, a negative or NaN rate) gives finite output from valid frames, nothing else.
//
// HOW A THREAD FINDS ITS SEGMENT: a per-thread binary search of seg_o in global memory.  The table of the workload (8 rows x 100 segments x 20 bytes = 16 KB) is
// L2-resident after its first touch, a search is ceil(log2 n) <= 7 dependent loads of ~200 cycles each (L2 hit), and the threads of a wave cover at most 4
// consecutive frames (20 float4 groups per frame of 80 channels), so the loads of a wave fall into one or two cache lines.  Staging the block's slice of seg_o in
// LDS would need the same search once per block to find the slice, a barrier, and then a second, shorter search -- more code and a barrier for a kernel that
// moves a few MB and is bound by its launch.  Measured beside cbx_mel_time_scale_f32: DESIGN.md section 6.
//
// Everything else is mel_time_scale_kernel: one thread per output float4 when pointers and strides allow 16-byte access, per float otherwise; plain loads and
// stores, no LDS, no atomics; frames [out_lens[b], T_out) written as zeros (out_lens cut to T_out here); columns [C, row stride) not touched; input frames from
// in_lens[b] on never read.
#include <math.h>

#include "cbx_common.h"

namespace {

constexpr int MW_MAX_ROWS = 64;

// seg_off, by value (host-checked: 0 <= off[0], off[b] < off[b + 1], off[B] <= n_seg)
struct mw_rows_t {
    int off[MW_MAX_ROWS + 1];
};

// grid (ceil(T_out * CV / 256), B): thread = (output frame j, channel group c) of batch row blockIdx.y; CV = C / VEC channel groups of VEC floats
template <int VEC>
__global__ __launch_bounds__(256) void mel_time_warp_kernel(const float* __restrict__ in, long in_sb, long in_ld, int T_in, const int* __restrict__ in_lens,
                                                            const mw_rows_t rows, const int* __restrict__ seg_o, const double* __restrict__ seg_a,
                                                            const double* __restrict__ seg_s, float* __restrict__ out, long out_sb, long out_ld, int T_out,
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
        cbx_mel_blend_store<VEC>(o, nullptr, nullptr, 0.0f);
        return;
    }
    // the last segment k of the row with seg_o[k] <= j (the first one when there is none): k stays in [lo, hi) whatever seg_o holds
    int k = rows.off[b], hi = rows.off[b + 1];
    while (hi - k > 1) {
        const int m = k + ((hi - k) >> 1);
        if (seg_o[m] <= j)
            k = m;
        else
            hi = m;
    }
    const long jj = (long)j - (long)seg_o[k];
    const double s = seg_s[k];
    const double x = fmax(0.0, seg_a[k] + (((double)jj + 0.5) * s - 0.5));  // (a NaN gives 0; an infinite x is cut by the clamp of the taps)
    const cbx_mel_taps_t p = cbx_mel_taps_at(x, 0, M);
    const float* row = in + (long)b * in_sb + c;
    cbx_mel_blend_store<VEC>(o, row + (long)p.i0 * in_ld, row + (long)p.i1 * in_ld, p.l);
}

}  // namespace

extern "C" int cbx_mel_time_warp_f32(const float* in, long in_sb, long in_ld, int T_in, const int* in_lens, const int* seg_off, int n_seg, const int* seg_o,
                                     const double* seg_a, const double* seg_s, float* out, long out_sb, long out_ld, int T_out, const int* out_lens, int B, int C,
                                     void* stream) {
    CBX_REQUIRE(in && seg_off && seg_o && seg_a && seg_s && out && out_lens, "mel_time_warp: null pointer");
    CBX_REQUIRE(C > 0, "mel_time_warp: C = %d", C);
    CBX_REQUIRE(in_ld >= C && out_ld >= C && in_sb >= C && out_sb >= C, "mel_time_warp: a stride is below C = %d (in %ld / %ld, out %ld / %ld)", C, in_sb, in_ld,
                out_sb, out_ld);
    CBX_REQUIRE(B >= 0 && B <= MW_MAX_ROWS && T_in >= 0 && T_out >= 0, "mel_time_warp: bad shape (B %d outside [0, %d], T_in %d, T_out %d)", B, MW_MAX_ROWS, T_in,
                T_out);
    mw_rows_t rows;
    for (int b = 0; b <= MW_MAX_ROWS; ++b) rows.off[b] = 0;
    CBX_REQUIRE(seg_off[0] >= 0 && n_seg >= 0, "mel_time_warp: seg_off[0] = %d, n_seg = %d", seg_off[0], n_seg);
    rows.off[0] = seg_off[0];
    for (int b = 0; b < B; ++b) {
        CBX_REQUIRE(seg_off[b + 1] > seg_off[b] && seg_off[b + 1] <= n_seg, "mel_time_warp: row %d has segments [%d, %d) of a table of %d: every row needs at least one", b,
                    seg_off[b], seg_off[b + 1], n_seg);
        rows.off[b + 1] = seg_off[b + 1];
    }
    if (B == 0 || T_out == 0) return 0;
    const bool vec = C % 4 == 0 && in_ld % 4 == 0 && out_ld % 4 == 0 && in_sb % 4 == 0 && out_sb % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const int CV = vec ? C / 4 : C;
    const long n = (long)T_out * CV, gx = (n + 255) / 256;
    CBX_REQUIRE(gx <= 0x7fffffffl, "mel_time_warp: T_out * C too large for one launch");
    if (vec)
        hipLaunchKernelGGL(mel_time_warp_kernel<4>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, in_sb, in_ld, T_in, in_lens, rows, seg_o,
                           seg_a, seg_s, out, out_sb, out_ld, T_out, out_lens, CV);
    else
        hipLaunchKernelGGL(mel_time_warp_kernel<1>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, in, in_sb, in_ld, T_in, in_lens, rows, seg_o,
                           seg_a, seg_s, out, out_sb, out_ld, T_out, out_lens, CV);
    return cbx_check_launch("mel_time_warp");
}
