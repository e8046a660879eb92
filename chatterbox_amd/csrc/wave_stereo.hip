// Stereo dialogue (cbx_wave_pan_mix_f32, cbx_wave_loudness_ch_f32, cbx_wave_limit_ch_f32, include/cbx.h): the turns of a conversation summed into TWO planes, each
// voice at a place of its own between left and right, then metered and limited as ONE two-channel signal.  The reference has no counterpart: it returns one mono
// utterance of one voice (tts.py:272, mtl_tts.py:352, tts_turbo.py:320).
//
// This file holds the three entries and no kernel: each mono kernel takes the plane or channel count as a template parameter, and each entry here is a call of
// the shared host side that wave_common.h declares.
//   * The panned mix is wave_mix_kernel<2> behind cbx_wave_mix_run (wave_mix.hip, whose header states the tile, the order of the sums and the planes' alignment).
//   * The meter's per-row phases and the limiter's oversampler are the mono entries' code; the step that sees both channels -- the sum of the segment energies,
//     the maximum of the m -- is the channel count C of wave_loud_row_kernel (wave_loudness.hip) and wave_limit_kernel (wave_limit.hip).  Here: C and the groups'
//     lengths are checked, then the shared launchers run.
#include "cbx_common.h"
#include "../../chatterbox_amd/csrc/wave_common.h"  // (by its path from the root: the header says why)

extern "C" int cbx_wave_pan_mix_f32(const float* wav, const long* row_off, const int* row_len, const long* start, const int* flags, const float* pan, int R,
                                    const float* gain, int G, const int* gain_idx, const float* ramp, int fade, float* out, long plane_stride, long out_len,
                                    int accumulate, void* stream) {
    return cbx_wave_mix_run("wave_pan_mix", 2, wav, row_off, row_len, start, flags, pan, R, gain, G, gain_idx, ramp, fade, out, plane_stride, out_len, accumulate,
                            stream);
}

extern "C" int cbx_wave_loudness_ch_f32(const float* wav, const long* row_off, const int* row_len, int R, int C, const double* coef, int hop, const double* target,
                                        double ceiling, double* stats, float* gain, double* ws, long ws_cap, void* stream) {
    if (const int rc = cbx_wave_groups("wave_loudness_ch", row_off, row_len, R, C)) return rc;
    return cbx_wave_loudness_run("wave_loudness_ch", wav, row_off, row_len, R, C, coef, hop, target, ceiling, stats, gain, ws, ws_cap, stream);
}

extern "C" int cbx_wave_limit_ch_f32(const float* wav, const long* row_off, const int* row_len, int R, int C, const float* gain, const double* ceiling, const float* tab,
                                     int U, int T, const float* win, int H, float* out, const long* out_off, long out_cap, double* stats, double* ws, long ws_cap,
                                     void* stream) {
    if (const int rc = cbx_wave_groups("wave_limit_ch", row_off, row_len, R, C)) return rc;
    return cbx_wave_limit_run("wave_limit_ch", wav, row_off, row_len, R, C, gain, ceiling, tab, U, T, win, H, out, out_off, out_cap, stats, ws, ws_cap, stream);
}
