// enc_head.inc -- k_enc_head_mfma: Dense(200)'s bias and activation, then Dense(20) and the code's activation; part of encoder.hip.
//
// The hidden layer is bias + Dense(200)'s k slices in slice order, then the activation; Dense(20) runs for SIXTEEN patches per
// workgroup on v_mfma_f32_16x16x4_f32 (an exact fmaf chain over k ascending).  The four wavefronts of a workgroup split the 13
// groups of 16 hidden columns (j = wave, wave + 4, ...); everything a wavefront needs after the row lookup is requested at once --
// its slices of the partial sums, the bias, its fragments of the weights (enc_wd2q, pre-arranged) -- so a tile is two memory
// round trips deep; the four partial products meet in LDS and are added in wavefront order.
//   A[m][k]: lane (m = lane & 15, g = lane >> 4) holds hidden columns 16 j + 4 g .. + 3 of patch m; MFMA (j, i) contracts
//   k = 16 j + 4 g + i over g.  B[k][n] = wd2 zero-padded to [208][32].
//   C[4 g + i][n]: lane (g, n) holds outputs n (n-tile 0) and 16 + n (n-tile 1: four live columns) of patches 4 g .. 4 g + 3.
// The sum over the 200 hidden units is four chains in ascending k, added in wavefront order.  De-duplicated launches: a patch
// takes the row of its representative (slot_of, dedup.hip), so every key point that owns a copy gets the result.
#define HEAD_WQ_FLOATS (13 * 2 * 64 * 4)   // Dense(20) as the B operand: head_weight_fragments -> enc_wd2q
#define HM_JW ((D1_NT + 3) / 4)   // hidden-column groups per wavefront (4, the last wavefront's fourth is empty)
// host: wd2 [200][20] -> [j 13][n-tile 2][lane 64] x float4 (i = 0 .. 3): w[16 j + 4 g + i][16 nt + n], zero beyond 200 / 20
static void head_weight_fragments(const float *wd2, float *out) {
    for (int j = 0; j < D1_NT; ++j)
        for (int nt = 0; nt < 2; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 4; ++i) {
                    const int k = 16 * j + 4 * (lane >> 4) + i, col = 16 * nt + (lane & 15);
                    out[(((size_t)j * 2 + nt) * 64 + lane) * 4 + i] = (k < DENSE_N && col < 20) ? wd2[k * 20 + col] : 0.0f;
                }
}

// H: dense_1's activation, C: dense_2's.  The self-check on the way out follows C: a tanh code lies within [-1, 1], a linear code is finite.
template <int SPLIT, int H, int C>
static __device__ __forceinline__ void enc_head_body(const float *__restrict__ part, int64_t n_patches, int64_t n_rows_pad,
                                                     const float *__restrict__ bd1p, const float4 *__restrict__ wd2q,
                                                     const float *__restrict__ bd2, int group, const caelo_enc_out &outs,
                                                     int out_stride, const caelo_enc_in &in, int32_t *faults) {
    __shared__ f32x4 s_c[3][2][64];   // partial products of wavefronts 1 .. 3
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, g = lane >> 4;
    const unsigned n_all = (unsigned)n_patches, per_in = (unsigned)in.per_frame, per_out = (unsigned)outs.per_frame;
    const unsigned tile = blockIdx.x;
    const unsigned p_raw = tile * 16u + (unsigned)m;
    const unsigned p = p_raw < n_all ? p_raw : n_all - 1u;   // (a lane past the end repeats the last patch; its outputs are not stored)
    // ---- requests that do not depend on the patch: this wavefront's weight fragments and bias
    float4 wq[HM_JW][2], b1[HM_JW];
#pragma unroll
    for (int c = 0; c < HM_JW; ++c) {
        const int j = wave + 4 * c;
        if (j < D1_NT) {
            wq[c][0] = wd2q[((size_t)j * 2 + 0) * 64 + lane];
            wq[c][1] = wd2q[((size_t)j * 2 + 1) * 64 + lane];
            b1[c] = *(const float4 *)(bd1p + 16 * j + 4 * g);
        }
    }
    // ---- the row that holds the patch's result: its representative's with de-duplication
    unsigned row = p;
    if (in.dedup) {
        const unsigned f_ = p / per_in;
        int r_ = enc_tables(in, (int)f_)->slot_of[p - f_ * per_in];        // a row of the whole launch set ...
        if (r_ < 0) {                                                       // ... or -(representative + 1): its row
            const unsigned g_ = (unsigned)(-r_ - 1), fr_ = g_ / per_in;
            r_ = enc_tables(in, (int)fr_)->slot_of[g_ - fr_ * per_in];
        }
        row = (unsigned)r_;
    }
    const float *src = part + (size_t)row * DENSE_NP + 4 * g;
    float4 v[HM_JW][SPLIT];
#pragma unroll
    for (int c = 0; c < HM_JW; ++c)
#pragma unroll
        for (int sp = 0; sp < SPLIT; ++sp)
            if (wave + 4 * c < D1_NT) v[c][sp] = *(const float4 *)(src + (size_t)sp * n_rows_pad * DENSE_NP + 16 * (wave + 4 * c));
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < HM_JW; ++c) {
        if (wave + 4 * c < D1_NT) {
            float4 sum = b1[c];
#pragma unroll
            for (int sp = 0; sp < SPLIT; ++sp) { sum.x += v[c][sp].x; sum.y += v[c][sp].y; sum.z += v[c][sp].z; sum.w += v[c][sp].w; }
            const float hv[4] = {enc_act<H>(sum.x), enc_act<H>(sum.y), enc_act<H>(sum.z), enc_act<H>(sum.w)};
            const float w0[4] = {wq[c][0].x, wq[c][0].y, wq[c][0].z, wq[c][0].w}, w1[4] = {wq[c][1].x, wq[c][1].y, wq[c][1].z, wq[c][1].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[i], w0[i], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[i], w1[i], acc1, 0, 0, 0);
            }
        }
    }
    if (wave > 0) {
        s_c[wave - 1][0][lane] = acc0;
        s_c[wave - 1][1][lane] = acc1;
    }
    __syncthreads();
    if (wave > 0) return;
    // ---- wavefront 0: the four partial products in wavefront order, bias, tanh; C row 4 g + i = patch tile * 16 + 4 g + i
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        acc0 += s_c[w][0][lane];
        acc1 += s_c[w][1][lane];
    }
    const float bo0 = bd2[m], bo1 = m < 4 ? bd2[16 + m] : 0.0f;   // output bias of this lane's two C columns
    constexpr float lim = C == CAELO_ACT_TANH ? 1.0f : 3.402823466e+38f;   // (NaN and inf fail `<= lim` either way)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned pp = tile * 16u + 4u * (unsigned)g + (unsigned)i;
        if (pp < n_all) {
            // patches of several frames in one launch: frame f = p / per_frame writes into its own rows
            const unsigned f = pp / per_out, q = pp - f * per_out, kp = q / (unsigned)group;
            float *dst = outs.base[f] + (size_t)kp * out_stride + (size_t)(q - kp * (unsigned)group) * 20;
            // the encoder's own invariant: a tanh code is finite and within [-1, 1], a linear one finite; counted per value (caelo_lane_faults)
            const float d0 = enc_act<C>(bo0 + acc0[i]);
            dst[m] = d0;
            if (!(fabsf(d0) <= lim)) atomicAdd(faults, 1);
            if (m < 4) {
                const float d1 = enc_act<C>(bo1 + acc1[i]);
                dst[16 + m] = d1;
                if (!(fabsf(d1) <= lim)) atomicAdd(faults, 1);
            }
        }
    }
}
#define ENC_HEAD_ARGS const float *__restrict__ part, int64_t n_patches, int64_t n_rows_pad, const float *__restrict__ bd1p,      \
                      const float4 *__restrict__ wd2q, const float *__restrict__ bd2, int group, caelo_enc_out outs,             \
                      int out_stride, const caelo_enc_in in, int32_t *faults
template <int SPLIT>
__global__ void __launch_bounds__(256) k_enc_head_mfma(ENC_HEAD_ARGS) {
    enc_head_body<SPLIT, CAELO_ACT_TANH, CAELO_ACT_TANH>(part, n_patches, n_rows_pad, bd1p, wd2q, bd2, group, outs, out_stride, in, faults);
}
template <int SPLIT, int H, int C>   // the three other (hidden, code) pairs
__global__ void __launch_bounds__(256) k_enc_head_mfma_act(ENC_HEAD_ARGS) {
    enc_head_body<SPLIT, H, C>(part, n_patches, n_rows_pad, bd1p, wd2q, bd2, group, outs, out_stride, in, faults);
}
