// enc_conv3.inc -- k_enc_conv3: conv3 (16->32) as an implicit GEMM, M = 64 positions / patch, N = 32, K = 27*16; part of encoder.hip.
//
// f32 products on the f16 matrix pipe: both operands are TWO f16 terms, x = hi + lo (enc_common.h), and a product is the three
// partial products a_lo b_hi + a_hi b_lo + a_hi b_hi -- 3 v_mfma_f32_16x16x32_f16 per K = 32 slab, accumulated in f32, smallest
// terms first.  Each partial product of two f16 is exact in f32; the dropped lo lo term is 2^-22 relative, and measured against the
// f32 oracle the descriptors do not move (tools/enc_layer_errors.py).  (Round 2 ran six bf16 MFMAs on 3-way splits -- 168 instead
// of 112 B registers, three LDS planes instead of two; config5.hip still does, and derives that arithmetic.)
//
// The weights are split once on the host (conv3_split_weights -> enc_w3x, already in register order), the activations once per
// patch while P2 is staged in LDS.  LDS per patch slot: [term 2][channel half 2][pos][8] f16 (16 B per position), pos =
// (xp*6 + yp)*8 + zp over the zero-haloed 6x6x6 volume (z pitch 8).  K = 32 per MFMA = two taps x 16 channels: lanes g < 2 carry
// tap A of a pair, lanes g >= 2 tap B; taps are paired (enc_pairA/B/Class, enc_common.h) so that B - A is one of three constant
// position offsets (+1 z, +1 y, +1 x), which the upper lanes fold into their base address -- every other offset is an instruction
// immediate.  An m-tile is one x plane (lane m -> y = m >> 2, z = m & 3); with the z pitch of 8 and the second channel half
// displaced by 4 positions, each 16-lane group of a ds_read_b128 (MI355X_MICROARCH LDS table) touches all 64 banks once.
#define C3X_NPAIR 14                 // tap pairs
#define C3X_NS 2                     // terms per operand
#define C3X_PLANE 48                 // positions per padded x plane (6 rows of 8)
#define C3X_ARR 292                  // positions per (term, half) array: 288 used, = 4 mod 16 (bank rotation of half 1)
#define C3X_SPLIT (2 * C3X_ARR)
#define C3X_SLOT (C3X_NS * C3X_SPLIT)     // positions (x 16 B) per patch slot
__host__ __device__ constexpr int c3x_tapPos(int t) { return (t / 9) * C3X_PLANE + ((t / 3) % 3) * 8 + (t % 3); }
// x plane X never sees data through the taps of pair P (all of them read the zero halo plane): skipped exactly
__host__ __device__ constexpr bool c3x_dead(int x, int p) {
    return (x == 0 && enc_pairA(p) / 9 == 0 && (enc_pairB(p) < 0 || enc_pairB(p) / 9 == 0)) ||
           (x == 3 && enc_pairA(p) / 9 == 2 && (enc_pairB(p) < 0 || enc_pairB(p) / 9 == 2));
}

// host: W3 [27][16][32] -> [ntile 2][pair 14][term 2][lane 64] uint4, the B operand of lane (n = lane & 15, g = lane >> 4)
static void conv3_split_weights(const float *w3, uint4 *out) {
    for (int nt = 0; nt < 2; ++nt)
        for (int p = 0; p < C3X_NPAIR; ++p)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = lane & 15, g = lane >> 4;
                const int tap = g < 2 ? enc_pairA(p) : enc_pairB(p);
                uint4 *o = out + ((size_t)(nt * C3X_NPAIR + p) * C3X_NS) * 64 + lane;
                uint16_t h[8], l[8];
                for (int i = 0; i < 8; ++i)
                    enc_split2h(tap >= 0 ? w3[(tap * 16 + 8 * (g & 1) + i) * 32 + nt * 16 + n] : 0.0f, h[i], l[i]);
                o[0] = enc_pack_h8(h);
                o[64] = enc_pack_h8(l);
            }
}

#ifndef C3X_WGS
#define C3X_WGS 2   // workgroups per CU the register budget is set for (3 spill at 168 registers: 183 instead of 92 us per 8 frames)
#endif
template <int H>
static __device__ __forceinline__ void enc_conv3_body(const float *__restrict__ p2, int64_t n_patches, const caelo_enc_in &in,
                                                      const uint4 *__restrict__ w3x, const float *__restrict__ b3g,
                                                      float *__restrict__ f3, int *__restrict__ stage1_counter,
                                                      int *__restrict__ xcd_counters) {
    __shared__ uint4 S[2 * C3X_SLOT];
    // stage 1 (the previous kernel on this stream) is complete: hand its work counter back at zero, so that no
    // memset launch sits on the encoder stream's critical path
    if (blockIdx.x == 0 && threadIdx.x == 0) *stage1_counter = 0;
    if (blockIdx.x == 0 && threadIdx.x < 8) xcd_counters[threadIdx.x * ENC_XCD_CSTRIDE] = 0;  // stage 1's per-XCD queues, for the next launch set
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int ntile = wave & 1, slot = __builtin_amdgcn_readfirstlane(wave >> 1);
    uint4 bq[C3X_NPAIR][C3X_NS];
#pragma unroll
    for (int p = 0; p < C3X_NPAIR; ++p)
#pragma unroll
        for (int sp = 0; sp < C3X_NS; ++sp) bq[p][sp] = w3x[((size_t)(ntile * C3X_NPAIR + p) * C3X_NS + sp) * 64 + lane];
    const float bias = b3g[16 * ntile + n];
    for (int i = tid; i < 2 * C3X_SLOT; i += 256) S[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const int n_items = enc_items_total(in, n_patches);
    const int n_pairs = (n_items + 1) / 2;
    // item (wave-uniform) -> row of P2 / F3 (the row stage 1 wrote)
#define C3_ROW(ITEM, ROW)                                     \
    {                                                         \
        ROW = (ITEM);                                         \
        if (in.dedup) {                                       \
            int f_, i_;                                       \
            ROW = enc_item_row(in, (ITEM), f_, i_);           \
        }                                                     \
    }
    // register staging: the next pair's 2 x 4 KB are fetched while this pair's MFMAs run; thread -> (slot, position,
    // channel half): 8 consecutive channels
    const int f_slot = __builtin_amdgcn_readfirstlane(tid >> 7), f_pos = (tid >> 1) & 63, f_h = tid & 1;
    const int f_q = (((f_pos >> 4) + 1) * 6 + ((f_pos >> 2) & 3) + 1) * 8 + (f_pos & 3) + 1;
    float4 pre0, pre1;
#define C3_FETCH(PAIR)                                                                           \
    {                                                                                            \
        const int pa_ = (PAIR) * 2 + f_slot;                                                     \
        pre0 = make_float4(0.f, 0.f, 0.f, 0.f);                                                  \
        pre1 = pre0;                                                                             \
        if ((PAIR) < n_pairs && pa_ < n_items) {                                                 \
            int row_;                                                                            \
            C3_ROW(pa_, row_)                                                                    \
            const float4 *q_ = (const float4 *)(p2 + (size_t)row_ * 1024 + f_pos * 16 + 8 * f_h); \
            pre0 = q_[0];                                                                        \
            pre1 = q_[1];                                                                        \
        }                                                                                        \
    }
#ifdef CAELO_C3_PROF   // make C3PROF=1 (NOT together with PROF=1: stage 1's profile uses the same slots of g_enc_stamp)
    unsigned long long c3_t[4] = {0ull, 0ull, 0ull, 0ull};
    unsigned c3_prev = (unsigned)clock64();
#define C3_STAMP(i) do { if (tid == 0) { const unsigned t_ = (unsigned)clock64(); c3_t[i] += t_ - c3_prev; c3_prev = t_; } } while (0)
#else
#define C3_STAMP(i) do { } while (0)
#endif
    // Work distribution: eight per-XCD queues as in stage 1 (pair p belongs to XCD p % 8; ONE counter for the 12 288 pairs of an
    // 8-frame launch would retire its same-address atomics in ~150 us).  A workgroup's first two queue positions are static (its
    // rank among the XCD's workgroups, then rank + their number), later ones are tickets drawn one iteration before they are needed
    // as `next` (stage 1 zeroes the counters).  Inside the frame pipeline the grid leaves a quarter of the slots free and the other
    // streams' kernels slow the workgroups of SOME CUs: with the static stride every workgroup did the same number of pairs and the
    // launch ended with its slowest CU.
    __shared__ int s_after[2];   // by iteration parity: thread 0 may be an iteration ahead of the slowest reader
    const int xcd = (int)(blockIdx.x & 7u), wgs_of_xcd = ((int)gridDim.x - xcd + 7) >> 3;
    int *const ticket = stage1_counter + C3X_TICKET_INT + 32 * xcd;
    int pair = xcd + 8 * (int)(blockIdx.x >> 3), next = pair + 8 * wgs_of_xcd;
    int drawn = 0;   // thread 0: the ticket drawn in the previous iteration
    if (tid == 0) drawn = atomicAdd(ticket, 1);
    C3_FETCH(pair)
    for (int it = 0; pair < n_pairs; pair = next, next = __builtin_amdgcn_readfirstlane(s_after[it & 1]), ++it) {
        C3_STAMP(3);
        {   // split the staged 8 channels into their two f16 terms: 2 x 16 B into LDS
            const float v[8] = {pre0.x, pre0.y, pre0.z, pre0.w, pre1.x, pre1.y, pre1.z, pre1.w};
            uint4 *d = &S[f_slot * C3X_SLOT + f_h * C3X_ARR + f_q];
            uint32_t h[4], l[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) enc_split2h_pk(v[2 * k], v[2 * k + 1], h[k], l[k]);
            d[0] = make_uint4(h[0], h[1], h[2], h[3]);
            d[C3X_SPLIT] = make_uint4(l[0], l[1], l[2], l[3]);
        }
        if (tid == 0) s_after[it & 1] = xcd + 8 * (2 * wgs_of_xcd + drawn);   // the pair after `next` (read after the loop's second barrier)
        C3_STAMP(0);
        __syncthreads();
        C3_STAMP(1);
        if (tid == 0) drawn = atomicAdd(ticket, 1);
        C3_FETCH(next)
        const int item = pair * 2 + slot;
        int patch;
        C3_ROW(item, patch)
        // lane (m = n, g): output (y = n >> 2, z = n & 3) of x plane X reads padded (X + ka, y + kb, z + kc)
        const uint4 *base = &S[slot * C3X_SLOT + (g & 1) * C3X_ARR + (n >> 2) * 8 + (n & 3)];
        const uint4 *ab[4] = {base + (g >= 2 ? 1 : 0), base + (g >= 2 ? 8 : 0), base + (g >= 2 ? C3X_PLANE : 0), base};
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            f32x4 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = (f32x4){bias, bias, bias, bias};
#pragma unroll
            for (int p = 0; p < C3X_NPAIR; ++p) {
                typedef _Float16 c3_h8 __attribute__((ext_vector_type(8)));
                const c3_h8 bh = __builtin_bit_cast(c3_h8, bq[p][0]), bl = __builtin_bit_cast(c3_h8, bq[p][1]);
                c3_h8 ah[2], al[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (c3x_dead(2 * round + j, p)) continue;
                    const uint4 *a = ab[enc_pairClass(p)] + c3x_tapPos(enc_pairA(p)) + (2 * round + j) * C3X_PLANE;
                    ah[j] = __builtin_bit_cast(c3_h8, a[0]);
                    al[j] = __builtin_bit_cast(c3_h8, a[C3X_SPLIT]);
                }
                // smallest terms first; the two accumulators alternate so that no MFMA waits for its predecessor
#define C3X_MAC(A, B)                                                                                           \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) if (!c3x_dead(2 * round + j, p))                              \
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[j], B, acc[j], 0, 0, 0);
                C3X_MAC(al, bh)
                C3X_MAC(ah, bl)
                C3X_MAC(ah, bh)
            }
            if (item < n_items) {
                // C rows 4g + r -> (y = g, z = r); flatten index (x,y,z,c) = ((x*4 + y)*4 + z)*32 + c
                float *dst = f3 + (size_t)patch * 2048 + 16 * ntile + n;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(((2 * round + j) * 4 + g) * 4 + r) * 32] = enc_act<H>(acc[j][r]);
            }
        }
        C3_STAMP(2);
        __syncthreads();
    }
#ifdef CAELO_C3_PROF
    if (tid == 0) {
        for (int i = 0; i < 4; ++i) atomicAdd(&g_enc_stamp[8 + i], c3_t[i]);
        atomicAdd(&g_enc_stamp[12], 1ull);
    }
#endif
}
#define ENC_CONV3_ARGS const float *__restrict__ p2, int64_t n_patches, const caelo_enc_in in, const uint4 *__restrict__ w3x,     \
                       const float *__restrict__ b3g, float *__restrict__ f3, int *__restrict__ stage1_counter,                   \
                       int *__restrict__ xcd_counters
__global__ void __launch_bounds__(256, C3X_WGS) k_enc_conv3(ENC_CONV3_ARGS) {
    enc_conv3_body<CAELO_ACT_TANH>(p2, n_patches, in, w3x, b3g, f3, stage1_counter, xcd_counters);
}
__global__ void __launch_bounds__(256, C3X_WGS) k_enc_conv3_relu(ENC_CONV3_ARGS) {
    enc_conv3_body<CAELO_ACT_RELU>(p2, n_patches, in, w3x, b3g, f3, stage1_counter, xcd_counters);
}
