// dec_fold.hip -- the decoder's weight fold: host code only (no device call, no HIP header), so that it also links into a plain C++
// program (tools/micro/dec_fold_main.cpp runs it under the host sanitizers).
//
// UpSampling3D(2) followed by a 3^3 `same` convolution is eight parity-specific 2^3 convolutions on the zero-padded SOURCE grid.
// Output voxel u = 2s + p (p in {0,1} per axis) reads upsampled voxel u + t - 1 for tap t in {0,1,2}, which is source cell
// (u + t - 1) >> 1 = s + ((p + t - 1) >> 1): cell s + o + p - 1 with o = ((p + t - 1) >> 1) - (p - 1) in {0,1}.  p = 0: taps 0 | 1,2 fall on
// o = 0 | 1; p = 1: taps 0,1 | 2.  Taps that share a source cell are summed -- in float64, rounded to float32 once.  A tap that leaves the
// upsampled grid leaves the source grid by the same step, so zero padding there is zero padding here.
#include <stddef.h>

#include "../../include/caelo.h"

void caelo_set_error(const char *fmt, ...);

extern "C" __attribute__((visibility("default")))
int caelo_host_decoder_fold(const float *w, int cin, int cout, float *folded) {
    if (!w || !folded || cin < 1 || cout < 1) {
        caelo_set_error("caelo_host_decoder_fold: null argument or a channel count below 1");
        return CAELO_ERR_ARG;
    }
    const size_t cc = (size_t)cin * (size_t)cout;
    for (int p = 0; p < 8; ++p)
        for (int o = 0; o < 8; ++o)
            for (size_t e = 0; e < cc; ++e) {
                double acc = 0.0;
                for (int t = 0; t < 27; ++t) {   // taps in ascending order (x slowest)
                    const int ta[3] = {t / 9, (t / 3) % 3, t % 3}, pa[3] = {p >> 2, (p >> 1) & 1, p & 1}, oa[3] = {o >> 2, (o >> 1) & 1, o & 1};
                    bool hit = true;
                    for (int a = 0; a < 3; ++a) hit = hit && (((pa[a] + ta[a] - 1) >> 1) - (pa[a] - 1) == oa[a]);
                    if (hit) acc += (double)w[(size_t)t * cc + e];
                }
                folded[((size_t)p * 8 + (size_t)o) * cc + e] = (float)acc;
            }
    return CAELO_OK;
}
