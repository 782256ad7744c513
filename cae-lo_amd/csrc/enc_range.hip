// enc_range.hip -- the encoder's range guard: host code only (no device call, no HIP header), so that it also links into a plain C++
// program (tools/micro/enc_range_main.cpp runs it under the host sanitizers).
//
// The fast encoder kernels evaluate f32 products from 2-way f16 splits x = hi + lo, hi = f16(x) (enc_stage1x.inc, k_enc_conv3,
// k_enc_dense1p); f16(x) is inf above 65504.  Behind a tanh every activation lies in [-1, 1]; behind a relu it is bounded only by the
// weights.  The bounds here are the worst case over BINARY patches in float64, kept per channel: b_1[c] = sum |w1[.][c]| + |b1[c]|,
// b_l[c] = sum_k |w_l[k][c]| b_{l-1}[channel of k] + |b_l[c]|, 1 behind a tanh layer; B_l = max_c b_l[c] is what is reported (pooling and
// Flatten move values, they do not change a channel's bound).  Which of them bind:
//   B1  D = P1 - BG, |D| <= B1 under relu (both terms lie in [0, B1])   split by k_enc_stage1x for conv2
//   B2  P2                                                              split by k_enc_conv3
//   B3  F3                                                              split by k_enc_dense1p
//   B4, B5  the hidden vector and the code stay f32 (k_enc_head_mfma runs f32-input MFMAs): reported, never refused.
#include <math.h>
#include <stddef.h>

#include "../../include/caelo.h"

void caelo_set_error(const char *fmt, ...);

#define ENC_F16_MAX 65504.0

#define ENC_RANGE_MAX_CH 200
// cur[c] = sum_k |w[k][c]| prev[k % n_prev] + |b[c]|  (w [n_in][n_out], Keras order: the output channel is innermost and the input
// channel is the fastest index of k -- [tap][cin] for a convolution, (x, y, z, c) behind Flatten); returns max_c cur[c]
static double enc_layer_bound(const float *w, const float *b, size_t n_in, size_t n_out, const double *prev, size_t n_prev, double *cur) {
    double worst = 0.0;
    for (size_t c = 0; c < n_out; ++c) {
        double acc = 0.0;
        for (size_t k = 0; k < n_in; ++k) acc += fabs((double)w[k * n_out + c]) * prev[k % n_prev];
        cur[c] = acc + fabs((double)b[c]);
        if (!(cur[c] <= worst)) worst = cur[c];   // (a NaN weight makes the bound NaN, which no comparison below passes)
    }
    return worst;
}

extern "C" __attribute__((visibility("default")))
int caelo_host_encoder_range(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                             const float *wd1, const float *bd1, const float *wd2, const float *bd2, int hidden, int code,
                             double out[5]) {
    if (!(w1 && b1 && w2 && b2 && w3 && b3 && wd1 && bd1 && wd2 && bd2 && out)) {
        caelo_set_error("caelo_host_encoder_range: null argument");
        return CAELO_ERR_ARG;
    }
    if ((hidden != CAELO_ACT_TANH && hidden != CAELO_ACT_RELU) || (code != CAELO_ACT_TANH && code != CAELO_ACT_LINEAR)) {
        caelo_set_error("caelo_host_encoder_range: hidden activation tanh or relu, code activation tanh or linear");
        return CAELO_ERR_ARG;
    }
    const struct { const float *w, *b; size_t n_in, n_out; const char *name; } layer[5] = {
        {w1, b1, 27, 8, "conv3d_1"}, {w2, b2, 27 * 8, 16, "conv3d_2"}, {w3, b3, 27 * 16, 32, "conv3d_3"},
        {wd1, bd1, 2048, 200, "dense_1"}, {wd2, bd2, 200, 20, "dense_2"}};
    double bound[2][ENC_RANGE_MAX_CH] = {{1.0}};   // per channel, of the layer's input / output; a voxel is 0 or 1
    size_t n_prev = 1;
    for (int l = 0; l < 5; ++l) {
        const int act = l < 4 ? hidden : code;
        const double *prev = bound[l & 1];
        double *cur = bound[(l & 1) ^ 1];
        if (act == CAELO_ACT_TANH) {
            for (size_t c = 0; c < layer[l].n_out; ++c) cur[c] = 1.0;
            out[l] = 1.0;
        } else
            out[l] = enc_layer_bound(layer[l].w, layer[l].b, layer[l].n_in, layer[l].n_out, prev, n_prev, cur);
        n_prev = layer[l].n_out;
    }
    for (int l = 0; l < 3; ++l)   // the tensors a kernel converts to f16 halves
        if (!(out[l] <= ENC_F16_MAX)) {
            caelo_set_error("encoder model out of range: the output of %s can reach %.6g under relu, beyond the f16 range (65504) of the "
                            "halves the next layer's kernel splits it into", layer[l].name, out[l]);
            return l + 1;
        }
    return 0;
}
