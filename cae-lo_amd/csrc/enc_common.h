// enc_common.h -- what the 16^3 encoder (encoder.hip and its enc_*.inc) and the 32^3 stress case (config5.hip) share: the fast tanh,
// the 2-way f16 operand split with its host-side packing, and the tap pairing of the conv3 kernels.
#pragma once
#include "caelo_internal.h"

// tanh x = 1 - 2 / (exp(2x) + 1) on v_exp_f32 + v_rcp_f32: 5 instructions instead of libm's ~50 (the encoder
// evaluates 6.9 M tanh per frame; in k_enc_conv3 alone they were ~8 us).  Absolute error < 6e-7 over the whole
// range (saturates to +-1 through exp -> inf / 0), against a parity budget of 1e-4 on the descriptors.
__device__ inline float enc_tanh(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);  // exp(2x)
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// ---- f16 x 2: an f32 operand as two f16 terms, x = hi + lo with hi = RNE f16(x), lo = RNE f16(x - hi):
// |x - hi - lo| <= max(2^-22 |x|, 2^-25) (the MFMA honours f16 subnormals, tools/micro/f16_mfma_subnormal.hip)
__host__ __device__ inline uint16_t enc_f16_bits(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
__host__ __device__ inline float enc_f16_val(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
__host__ __device__ inline void enc_split2h(float x, uint16_t &hi, uint16_t &lo) {
    hi = enc_f16_bits(x);
    lo = enc_f16_bits(x - enc_f16_val(hi));
}
// device: two values -> their (hi, lo) terms, packed (value 0 in the low half)
__device__ inline void enc_split2h_pk(float x0, float x1, uint32_t &hi, uint32_t &lo) {
    const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
    const _Float16 l0 = (_Float16)(x0 - (float)h0), l1 = (_Float16)(x1 - (float)h1);
    hi = (uint32_t)__builtin_bit_cast(uint16_t, h0) | ((uint32_t)__builtin_bit_cast(uint16_t, h1) << 16);
    lo = (uint32_t)__builtin_bit_cast(uint16_t, l0) | ((uint32_t)__builtin_bit_cast(uint16_t, l1) << 16);
}
// host: eight f16 bit patterns -> the 16 bytes of a B fragment's lane (element 0 in the low half of .x)
static inline uint4 enc_pack_h8(const uint16_t h[8]) {
    return make_uint4(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16, h[4] | (uint32_t)h[5] << 16, h[6] | (uint32_t)h[7] << 16);
}

// host: the five events around the four launches of a profiled encode (caelo_encode_profile, caelo_encode32_profile); whatever was
// created is destroyed on every way out
struct enc_prof_events {
    hipEvent_t ev[5];
    int n = 0;
    hipError_t create() {
        for (; n < 5; ++n) {
            const hipError_t e = hipEventCreate(&ev[n]);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    ~enc_prof_events() {
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
    }
};

// ---- the 27 taps of a 3^3 kernel as 14 pairs (A, B) for a K = 32 MFMA over 16 channels (k_enc_conv3, k5_conv3_x3): lanes g < 2
// carry tap A, lanes g >= 2 tap B, and B - A is one of three constant position offsets -- class 0: +1 z (9 pairs, kc 0,1), class 1:
// +1 y (3 pairs, kb 0,1 at kc 2), class 2: +1 x (ka 0,1 at kb 2, kc 2); class 3: tap 26 alone (B = -1, its operand zero)
__host__ __device__ constexpr int enc_pairA(int p) { return p < 9 ? p * 3 : (p < 12 ? (p - 9) * 9 + 2 : (p == 12 ? 8 : 26)); }
__host__ __device__ constexpr int enc_pairB(int p) { return p < 9 ? p * 3 + 1 : (p < 12 ? (p - 9) * 9 + 5 : (p == 12 ? 17 : -1)); }
__host__ __device__ constexpr int enc_pairClass(int p) { return p < 9 ? 0 : (p < 12 ? 1 : (p == 12 ? 2 : 3)); }
