// config5.hip -- BASELINE.json configs[4]: "synthetic 128-beam dense scan, 2x voxel-patch resolution".
//
// NOT a reference code path.  The reference has PatchSize = 16 only (Voxel.py:31-33); this stress case keeps
// GetPatchesList's rule (Voxel.py:177-216) and the encoder's layer stack (EncoderModel4VoxelPatch.h5) at twice the
// patch resolution, as SURVEY.md section 8d defines it:
//   * window [-16,16)^3 around the key voxel, wrap-around placement d mod 32 (:213-214);
//   * the 496-nearest cap (:182,:195-196) DISABLED: a 32^3 window holds up to 32768 voxels, n_neighbors=496 would
//     truncate nearly every dense patch and its tie order is sklearn-defined -- every occupied voxel in the
//     window is set;
//   * Conv3D(1->8) tanh, MaxPool2 (16^3), Conv3D(8->16) tanh, MaxPool2 (8^3), Conv3D(16->32) tanh, Flatten
//     (16384), Dense(200) tanh, Dense(20) tanh; conv kernels, biases and dense_2 from the .h5, dense_1 a caller
//     supplied [16384][200] matrix (no trained weights exist at this size).
// Parity is against oracle/caelo_oracle.c (orc_patches32, orc_encode32) and, layer by layer and on edge inputs, against the float64
// network and the set-membership rule of tests/test_config5_gpu.py.
//
// Data layout: a patch is 512 u64 words, voxel (ix,iy,iz) at bit (lin & 63) of word (lin >> 6),
// lin = (ix*32 + iy)*32 + iz; activations are channels-last f32 ([x][y][z][c]) like the 16^3 path.
//
// Kernels: all four GEMM-shaped layers run on the matrix cores -- the three conv stages as dense implicit GEMMs over
// LDS-resident x slabs with f32 products from 3-way bf16 operand splits (k5_conv1pool_x3, k5_conv2_x3, k5_conv3_x3), Dense(200)
// and Dense(20) through the 16^3 path's kernels, Dense(200) instantiated for K = 16384 (k_enc_dense1p<16384, MTW>,
// k_enc_head_mfma: enc_dense32_head_launch, encoder.hip).  Dense scans leave little of the sparsity the 16^3 stage-1 kernel
// lives on, so nothing is skipped here.  See DESIGN.md section 4.5 for measured times.
#include <math.h>
#include <stdlib.h>

#include "enc_common.h"

#define VOX_SIZE 0.02
#define VIS_L 99.84
#define VIS_W 99.84
#define VIS_H 14.72

// ---- patches: one workgroup per (key point, scale); the 5x5x5 bricks the window can touch staged in LDS --------
__global__ void __launch_bounds__(256) k5_patches(const float *__restrict__ pts, int pts_ld, int64_t k_max,
                                                  const int32_t *__restrict__ n_key, caelo_brick_table t0,
                                                  caelo_brick_table t1, caelo_brick_table t2,
                                                  unsigned long long *__restrict__ bits) {
    __shared__ int slot[125];
    __shared__ unsigned long long win[125 * 8];
    const int tid = threadIdx.x;
    const int64_t pw = blockIdx.x;
    const int64_t kp = pw / 3;
    const int scale = (int)(pw % 3);
    uint32_t *out = (uint32_t *)(bits + pw * 512);
    const int K = n_key ? *n_key : (int)k_max;
    if (kp >= K) {
        for (int i = tid; i < 1024; i += 256) out[i] = 0u;
        return;
    }
    const caelo_brick_table tab = scale == 0 ? t0 : (scale == 1 ? t1 : t2);
    const double vs = scale == 0 ? VOX_SIZE : (scale == 1 ? VOX_SIZE * 8 : VOX_SIZE * 32);  // Voxel.py:31
    // Voxel.py:185,:193  KeyVoxels = int32((Pts + Visible*) / VoxelSizes[s])  (f64)
    const int kx = (int)(((double)pts[(size_t)pts_ld * kp] + VIS_L) / vs);
    const int ky = (int)(((double)pts[(size_t)pts_ld * kp + 1] + VIS_W) / vs);
    const int kz = (int)(((double)pts[(size_t)pts_ld * kp + 2] + VIS_H) / vs);
    const int bx0 = (kx - 16) >> 3, by0 = (ky - 16) >> 3, bz0 = (kz - 16) >> 3;
    if (tid < 125) {
        const int bx = bx0 + tid / 25, by = by0 + (tid / 5) % 5, bz = bz0 + tid % 5;
        slot[tid] = (bx >= 0 && by >= 0 && bz >= 0) ? caelo_brick_find(tab, caelo_pack3(bx, by, bz)) : -1;
    }
    __syncthreads();
    for (int i = tid; i < 1000; i += 256) {
        const int sl = slot[i >> 3];
        win[i] = sl >= 0 ? tab.bits[(size_t)sl * 8 + (i & 7)] : 0ull;
    }
    __syncthreads();
    const int zsh = (kz - 16) & 7;
    for (int r = tid; r < 1024; r += 256) {  // one (ix, iy) row of 32 z bits per iteration
        const int ix = r >> 5, iy = r & 31;
        const int x = kx + (ix < 16 ? ix : ix - 32), y = ky + (iy < 16 ? iy : iy - 32);  // :213-214 wrap-around
        const int bxl = (x >> 3) - bx0, byl = (y >> 3) - by0;
        const int ysh = (y & 7) << 3;
        unsigned long long strip = 0ull;  // 40 z bits starting at the first z brick
#pragma unroll
        for (int j = 0; j < 5; ++j)
            strip |= ((win[((bxl * 5 + byl) * 5 + j) * 8 + (x & 7)] >> ysh) & 0xFFull) << (8 * j);
        const uint32_t s32 = (uint32_t)(strip >> zsh);  // bit d <-> dz = d - 16
        out[r] = (s32 >> 16) | (s32 << 16);             // iz = dz mod 32
    }
}

// (Round 1's f32-input MFMA kernels for the three conv layers -- k5_conv1pool, k5_conv_mfma: 1.95 ms per frame against 1.28 ms
// for the split-operand kernels below, DESIGN.md 4.5 -- are gone from the library: one arithmetic, no environment switch.)
// ---- f32 products evaluated on the bf16 matrix pipe (3-way operand split) -----------------------------------------------
// v_mfma_f32_16x16x32_bf16 retires 16x the FLOPs per cycle of the f32-input MFMA (MI355X_MICROARCH: 2.5 PF vs 157 TF).  An f32
// value splits exactly into three bf16 terms, x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)
// (both differences are exact in f32; |x - hi - mid - lo| <= 2^-27 |x|), and a product a b is the sum of the six partial products
// a_hi b_hi + a_hi b_mid + a_mid b_hi + a_mid b_mid + a_hi b_lo + a_lo b_hi up to 2^-27 |a b| -- below the 2^-24
// rounding of an f32 multiply.  Each partial product of two bf16 is exact in f32 and the MFMA accumulates in f32, so
// the result is f32-grade at 6/16 of the f32 MFMA's time.  (The 16^3 encoder ran this arithmetic in round 2 and has since moved
// to two f16 terms and three partial products, enc_common.h; this stress case is the 3-way split's one user.)
typedef __bf16 c5_bf16x8 __attribute__((ext_vector_type(8)));
__device__ inline uint32_t c5_bf16_rne(float x) {  // bf16(x), round to nearest even, as the high half of an f32 bit pattern
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
}
__device__ inline void c5_split3(float x, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
    hi = c5_bf16_rne(x);
    const float r = x - __uint_as_float(hi);
    mid = c5_bf16_rne(r);
    lo = c5_bf16_rne(r - __uint_as_float(mid));
}
// Eight floats -> their three planes of 8 bf16, a uint4 each (element 0 in the low half of .x): OUT[0] = hi, OUT[1] = mid, OUT[2] = lo.
// (Macros, not functions: as force-inlined functions the same steps compile to other registers and code sizes in all three kernels.)
#define C5_PK(A) make_uint4((A[0] >> 16) | A[1], (A[2] >> 16) | A[3], (A[4] >> 16) | A[5], (A[6] >> 16) | A[7])
// the B operands: VALUE is an expression in i = 0 .. 7
#define C5_SPLIT3X8(OUT, VALUE)                                                                    \
    {                                                                                              \
        uint32_t h_[8], m_[8], l_[8];                                                              \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) c5_split3((VALUE), h_[i], m_[i], l_[i]);     \
        (OUT)[0] = C5_PK(h_);                                                                      \
        (OUT)[1] = C5_PK(m_);                                                                      \
        (OUT)[2] = C5_PK(l_);                                                                      \
    }
// staging: the eight channels at Q of one position, or zeros where !LIVE (the halo), to the three planes' addresses D0, D1, D2 in LDS
#define C5_STAGE3X8(LIVE, Q, D0, D1, D2)                                                           \
    {                                                                                              \
        uint32_t h_[8], m_[8], l_[8];                                                              \
        if (LIVE) {                                                                                \
            const float4 *q_ = (const float4 *)(Q);                                                \
            const float4 v0 = q_[0], v1 = q_[1];                                                   \
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};                   \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) c5_split3(v[k], h_[k], m_[k], l_[k]);    \
        } else {                                                                                   \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) h_[k] = m_[k] = l_[k] = 0u;              \
        }                                                                                          \
        *(uint4 *)(D0) = C5_PK(h_);                                                                \
        *(uint4 *)(D1) = C5_PK(m_);                                                                \
        *(uint4 *)(D2) = C5_PK(l_);                                                                \
    }
// one K = 32 slab of NT m-tiles: the six partial products, smallest terms first; the accumulators alternate so that no MFMA waits
// for its predecessor.  Reads the A fragments ah / am / al [NT] and the B fragments bh / bm / bl, adds into acc[NT].
#define C5_MAC(NT, A, B) _Pragma("unroll") for (int j = 0; j < (NT); ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[j], B, acc[j], 0, 0, 0);
#define C5_MAC6(NT) C5_MAC(NT, al, bh) C5_MAC(NT, ah, bl) C5_MAC(NT, am, bm) C5_MAC(NT, am, bh) C5_MAC(NT, ah, bm) C5_MAC(NT, ah, bh)

// ---- conv3 ----------------------------------------------------------------------------------------------------------------
// Layout: the activations are split ONCE, when the x slab is staged in LDS: per split and channel half h (8 channels)
// an array [pos][8] bf16, so a lane's ds_read_b128 is one position's 8 channels and 16 lanes read 256 contiguous
// bytes; an m-tile is 8 z of two x planes, and the plane pitch (104 positions) puts the two 128-byte runs on
// complementary bank halves.  K = 32 per instruction = two taps x 16 channels: lanes g < 2 carry tap A of the pair,
// lanes g >= 2 tap B.  Taps are paired so that B - A is one of three constant position offsets (+1 z, +1 y, +1 x);
// the upper lanes fold that offset into their base address and every other offset is an instruction immediate
// (the pairs: enc_pairA / B / Class, enc_common.h).
#define X3_PLANE 104                 // positions per padded x plane (10 x 10 used)
#define X3_NPOS (6 * X3_PLANE)       // 4 output planes + 2 halo planes
#define X3_ARR (X3_NPOS * 16)        // bytes of one (split, half) array
#define X3_NPAIR 14
__device__ constexpr int c5_tapPos(int t) { return (t / 9) * X3_PLANE + ((t / 3) % 3) * 10 + (t % 3); }

__global__ void __launch_bounds__(256, 2) k5_conv3_x3(const float *__restrict__ in, const float *__restrict__ w,
                                                      const float *__restrict__ b, float *__restrict__ out, int n_items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [split 3][half 2][X3_NPOS][8] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int nt = wave >> 1, xpair = wave & 1;
    // B operand: pair p, split s: 8 bf16 = channels 8 (g & 1) .. + 7 of tap (g < 2 ? A : B), column nt * 16 + m
    uint4 bq[X3_NPAIR][3];
#pragma unroll
    for (int p = 0; p < X3_NPAIR; ++p) {
        const int tap = g < 2 ? enc_pairA(p) : enc_pairB(p);
        C5_SPLIT3X8(bq[p], tap >= 0 ? w[(size_t)(tap * 16 + 8 * (g & 1) + i) * 32 + nt * 16 + m] : 0.0f)
    }
    const float bias = b[nt * 16 + m];
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t patch = item >> 1;
        const int xb = item & 1;
        const float *src = in + (size_t)patch * 512 * 16;
        __syncthreads();
        for (int i = tid; i < X3_NPOS * 2; i += 256) {  // (position, channel half)
            const int h = i & 1, pos = i >> 1;
            const int xl = pos / X3_PLANE, rem = pos % X3_PLANE;
            const int x = xb * 4 - 1 + xl, y = rem / 10 - 1, z = rem % 10 - 1;
            C5_STAGE3X8(rem < 100 && x >= 0 && x < 8 && y >= 0 && y < 8 && z >= 0 && z < 8, src + (((size_t)x * 8 + y) * 8 + z) * 16 + 8 * h,
                        lds + (0 * 2 + h) * X3_ARR + pos * 16, lds + (1 * 2 + h) * X3_ARR + pos * 16, lds + (2 * 2 + h) * X3_ARR + pos * 16)
        }
        __syncthreads();
        // m-tile (xpair, y): lane m -> output (x = 2 xpair + (m >> 3), y, z = m & 7); padded corner of its taps
        const int pos0 = (2 * xpair + (m >> 3)) * X3_PLANE + (m & 7);
        const unsigned char *base = lds + (g & 1) * X3_ARR + pos0 * 16;
        const unsigned char *ab[4] = {base + (g >= 2 ? 1 * 16 : 0), base + (g >= 2 ? 10 * 16 : 0),
                                      base + (g >= 2 ? X3_PLANE * 16 : 0), base};
        for (int round = 0; round < 4; ++round) {
            f32x4 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = (f32x4){bias, bias, bias, bias};
#pragma unroll
            for (int p = 0; p < X3_NPAIR; ++p) {
                const c5_bf16x8 bh = __builtin_bit_cast(c5_bf16x8, bq[p][0]), bm = __builtin_bit_cast(c5_bf16x8, bq[p][1]),
                                bl = __builtin_bit_cast(c5_bf16x8, bq[p][2]);
                c5_bf16x8 ah[2], am[2], al[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned char *a = ab[enc_pairClass(p)] + (c5_tapPos(enc_pairA(p)) + (round * 2 + j) * 10) * 16;
                    ah[j] = __builtin_bit_cast(c5_bf16x8, *(const uint4 *)(a));
                    am[j] = __builtin_bit_cast(c5_bf16x8, *(const uint4 *)(a + 2 * X3_ARR));
                    al[j] = __builtin_bit_cast(c5_bf16x8, *(const uint4 *)(a + 4 * X3_ARR));
                }
                C5_MAC6(2)
            }
            // C row 4 g + r of tile j: output (x = xb*4 + 2 xpair + (row >> 3), y = round*2 + j, z = row & 7)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * g + r;
                    const int x = xb * 4 + 2 * xpair + (row >> 3), y = round * 2 + j, z = row & 7;
                    out[((((size_t)patch * 8 + x) * 8 + y) * 8 + z) * 32 + nt * 16 + m] = enc_tanh(acc[j][r]);
                }
        }
    }
}

// ---- conv2 + pool with the same arithmetic: K = 32 = four taps x 8 channels per MFMA ----------------------------------------
// The 27 taps go into 7 quads in Keras order (taps 4q .. 4q + 3, one empty slot); lane group g carries tap 4q + g, and its
// position offset is a per-lane value computed once (7 address registers per tile row).  LDS per split: [pos][8] bf16 over
// the 4 zero-haloed input planes of a pooled x plane (18 x 18 each, 62 KB for the three splits: two workgroups per CU);
// an m-tile is one 16-voxel z row, a wave owns the 2 x 2 (x, y) rows of a pooled row (MaxPool = register max).
#define X2_DP 18
#define X2_NPOS (4 * X2_DP * X2_DP)
#define X2_ARR (X2_NPOS * 16)
#define X2_NQ 7
__device__ constexpr int c5_tapPos2(int t) { return (t / 9) * X2_DP * X2_DP + ((t / 3) % 3) * X2_DP + (t % 3); }

__global__ void __launch_bounds__(256, 2) k5_conv2_x3(const float *__restrict__ in, const float *__restrict__ w,
                                                      const float *__restrict__ b, float *__restrict__ out, int n_items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [split 3][X2_NPOS][8] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, g = lane >> 4;
    // B operand: quad q, split s: the 8 input channels of tap 4 q + g, output column m
    uint4 bq[X2_NQ][3];
    int aoff[X2_NQ];  // byte offset of this lane's tap within quad q
#pragma unroll
    for (int q = 0; q < X2_NQ; ++q) {
        const int tap = 4 * q + g;
        C5_SPLIT3X8(bq[q], tap < 27 ? w[(size_t)(tap * 8 + i) * 16 + m] : 0.0f)
        // tap index is lane dependent: spell the position offset out (t / 9, (t / 3) % 3, t % 3 of a runtime t)
        const int t = tap < 27 ? tap : 26;  // the empty slot reads a valid address, its weights are zero
        aoff[q] = ((t / 9) * X2_DP * X2_DP + ((t / 3) % 3) * X2_DP + (t % 3)) * 16;
    }
    const float bias = b[m];
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t patch = item >> 3;
        const int px = item & 7;
        const float *src = in + (size_t)patch * 4096 * 8;
        __syncthreads();
        for (int pos = tid; pos < X2_NPOS; pos += 256) {
            const int x = 2 * px - 1 + pos / (X2_DP * X2_DP), y = (pos / X2_DP) % X2_DP - 1, z = pos % X2_DP - 1;
            C5_STAGE3X8(x >= 0 && x < 16 && y >= 0 && y < 16 && z >= 0 && z < 16, src + (((size_t)x * 16 + y) * 16 + z) * 8,
                        lds + 0 * X2_ARR + pos * 16, lds + 1 * X2_ARR + pos * 16, lds + 2 * X2_ARR + pos * 16)
        }
        __syncthreads();
        for (int pi = 0; pi < 2; ++pi) {
            const int py = 2 * wave + pi;
            // tile (xa, yb): output (xa, y = 2 py + yb, z = m); padded corner = position (xa, y, m)
            const unsigned char *base = lds + ((2 * py) * X2_DP + m) * 16;
            f32x4 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (f32x4){bias, bias, bias, bias};
#pragma unroll
            for (int q = 0; q < X2_NQ; ++q) {
                const c5_bf16x8 bh = __builtin_bit_cast(c5_bf16x8, bq[q][0]), bm = __builtin_bit_cast(c5_bf16x8, bq[q][1]),
                                bl = __builtin_bit_cast(c5_bf16x8, bq[q][2]);
                c5_bf16x8 ah[4], am[4], al[4];
                const unsigned char *a = base + aoff[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) {  // j = 2 xa + yb
                    const int o = ((j >> 1) * X2_DP * X2_DP + (j & 1) * X2_DP) * 16;
                    ah[j] = __builtin_bit_cast(c5_bf16x8, *(const uint4 *)(a + o));
                    am[j] = __builtin_bit_cast(c5_bf16x8, *(const uint4 *)(a + o + X2_ARR));
                    al[j] = __builtin_bit_cast(c5_bf16x8, *(const uint4 *)(a + o + 2 * X2_ARR));
                }
                C5_MAC6(4)
            }
            // C rows 4 g + r = z; pooled z = 2 g + zp
            float *dst = out + ((((size_t)patch * 8 + px) * 8 + py) * 8 + 2 * g) * 16 + m;
#pragma unroll
            for (int zp = 0; zp < 2; ++zp) {
                float v = fmaxf(fmaxf(acc[0][2 * zp], acc[0][2 * zp + 1]), fmaxf(acc[1][2 * zp], acc[1][2 * zp + 1]));
                v = fmaxf(v, fmaxf(fmaxf(acc[2][2 * zp], acc[2][2 * zp + 1]), fmaxf(acc[3][2 * zp], acc[3][2 * zp + 1])));
                dst[zp * 16] = enc_tanh(v);
            }
        }
    }
}

// ---- conv1 + pool on the bf16 pipe: the input is binary, so only the weights need the 3-way split ------------------------
// The GEMM view: n = (z parity, channel), m = the 16 even z of a row, k = the 3 x 3 x 4 tap window, with
// the voxels stored as bf16 0 / 1 (exact): a product is A (B_hi + B_mid + B_lo), three MFMAs per k slab.  The window's
// 36 k go into two K = 32 slabs: lane group g carries window rows 2g and 2g + 1 (4 consecutive z each = two dwords of
// the voxel row), the ninth row sits alone in the second slab.  6 x 16 cycles per 32-voxel row instead of 9 x 32.
#define C1X_PITCH 36                       // bf16 per padded z row (34 used)
#define C1X_PLANE (34 * C1X_PITCH)
__global__ void __launch_bounds__(256) k5_conv1pool_x3(const unsigned long long *__restrict__ bits, const float *__restrict__ w1,
                                                       const float *__restrict__ b1, float *__restrict__ p1, int n_items) {
    __shared__ __attribute__((aligned(16))) unsigned short vox[4 * C1X_PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int dz = m >> 3, ch = m & 7;  // as the n index of B and C
    // B: slab 0 = window rows 2g, 2g+1; slab 1 = row 8 in lanes g == 0; element i -> (row + i / 4, kc' = i % 4)
    uint4 bq[2][3];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        C5_SPLIT3X8(bq[sl], ({
            const int r = sl == 0 ? 2 * g + (i >> 2) : (g == 0 && i < 4 ? 8 : -1);
            const int kc = (i & 3) - dz;
            r >= 0 && kc >= 0 && kc < 3 ? w1[(r * 3 + kc) * 8 + ch] : 0.0f;
        }))
    }
    // element offsets (bf16 units) of this lane's two window rows in slab 0; slab 1 reads row 8 everywhere
    const int r0 = 2 * g, r1 = 2 * g + 1;
    const int off0 = (r0 / 3) * C1X_PLANE + (r0 % 3) * C1X_PITCH, off1 = (r1 / 3) * C1X_PLANE + (r1 % 3) * C1X_PITCH;
    const int off8 = 2 * C1X_PLANE + 2 * C1X_PITCH;
    const float bias = b1[ch];
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t patch = item >> 4;
        const int px = item & 15;
        const uint32_t *src = (const uint32_t *)(bits + patch * 512);
        __syncthreads();
        // 4 planes x 34 rows of 36 bf16 = 18 dwords: thread -> (row, third of the row = 6 dwords)
        for (int i = tid; i < 4 * 34 * 3; i += 256) {
            const int row = i / 3, part = i % 3;
            const int x = 2 * px - 1 + row / 34, y = row % 34 - 1;
            const uint32_t word = (x >= 0 && x < 32 && y >= 0 && y < 32) ? src[x * 32 + y] : 0u;
            uint32_t *dst = (uint32_t *)&vox[row * C1X_PITCH + part * 12];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int z0 = part * 12 + 2 * j - 1, z1 = z0 + 1;  // padded indices part*12 + 2j, + 1
                const uint32_t lo16 = (z0 >= 0 && z0 < 32 && ((word >> z0) & 1u)) ? 0x3F80u : 0u;
                const uint32_t hi16 = (z1 >= 0 && z1 < 32 && ((word >> z1) & 1u)) ? 0x3F80u : 0u;
                dst[j] = lo16 | (hi16 << 16);
            }
        }
        __syncthreads();
        for (int pi = 0; pi < 4; ++pi) {
            const int py = 4 * wave + pi;
            // tile (xa, yb): output (xa, y = 2 py + yb, z = 2 m + dz) reads padded (xa + ka, y + kb, 2 m + kc')
            const unsigned short *base = &vox[(2 * py) * C1X_PITCH + 2 * m];
            f32x4 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (f32x4){bias, bias, bias, bias};
            c5_bf16x8 a0[4], a1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // j = 2 xa + yb
                const unsigned short *t = base + (j >> 1) * C1X_PLANE + (j & 1) * C1X_PITCH;
                // 4-byte aligned pairs of dwords (the row offset 2 m is only even): ds_read2_b32, not ds_read_b64
                const uint32_t *q0 = (const uint32_t *)(t + off0), *q1 = (const uint32_t *)(t + off1), *q8 = (const uint32_t *)(t + off8);
                a0[j] = __builtin_bit_cast(c5_bf16x8, make_uint4(q0[0], q0[1], q1[0], q1[1]));
                a1[j] = __builtin_bit_cast(c5_bf16x8, make_uint4(q8[0], q8[1], 0u, 0u));
            }
#pragma unroll
            for (int sp = 2; sp >= 0; --sp) {  // smallest terms first
                const c5_bf16x8 b0 = __builtin_bit_cast(c5_bf16x8, bq[0][sp]), b1v = __builtin_bit_cast(c5_bf16x8, bq[1][sp]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[j], b0, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[j], b1v, acc[j], 0, 0, 0);
            }
            // C row 4 g + r = pooled z; column = (dz, c)
            float *dst = p1 + ((((size_t)patch * 16 + px) * 16 + py) * 16 + 4 * g) * 8 + ch;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = fmaxf(fmaxf(acc[0][r], acc[1][r]), fmaxf(acc[2][r], acc[3][r]));
                v = fmaxf(v, __shfl_xor(v, 8));
                if (dz == (r >> 1)) dst[r * 8] = enc_tanh(v);
            }
        }
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------
CAELO_API int caelo_patches32(caelo_ctx *c, const caelo_voxmap *m, const float *pts, int pts_ld, int64_t k_max,
                              const int32_t *n_key, uint64_t *bits, void *stream) {
    CAELO_REQUIRE(c && m && pts && bits, "null argument");
    CAELO_REQUIRE(c->enc_hidden == CAELO_ACT_TANH && c->enc_code == CAELO_ACT_TANH, "the 32^3 path implements the tanh / tanh encoder only");
    CAELO_REQUIRE(k_max > 0 && pts_ld >= 3 && k_max * 3 < (1ll << 31), "bad shape");
    k5_patches<<<(unsigned)(k_max * 3), 256, 0, caelo_stream(stream)>>>(pts, pts_ld, k_max, n_key, m->brick[0], m->brick[1],
                                                                       m->brick[2], (unsigned long long *)bits);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

CAELO_API int caelo_set_encoder32_dense(caelo_ctx *c, const float *wd1, const float *bd1) {
    CAELO_REQUIRE(c && wd1 && bd1, "null argument");
    return enc_upload_dense1(wd1, bd1, 16384, &c->enc32_wd1x, &c->enc32_bd1);
}

static inline int64_t c5_pad(int64_t n) { return enc_dense_pad(n); }  // whole dense-1 row tiles

// ws = P1 [n][16^3][8] | P2 [n][8^3][16] | F3 [np][16384] | dense-1 split-K partial sums (sized by encoder.hip)
CAELO_API int64_t caelo_encode32_ws_bytes(int64_t n_patches) {
    if (n_patches <= 0) return 0;
    const int64_t np = c5_pad(n_patches);
    return (n_patches * (32768 + 8192) + np * 16384) * (int64_t)sizeof(float) + enc_dense32_part_bytes(np);
}

// test aid: where encode32_impl below puts what its kernels leave behind
CAELO_API int caelo_encode32_ws_layout(int64_t n_patches, int64_t out[7]) {
    CAELO_REQUIRE(out && n_patches > 0, "caelo_encode32_ws_layout: bad argument");
    const int64_t np = c5_pad(n_patches);
    out[0] = 0;
    out[1] = out[0] + n_patches * 32768 * (int64_t)sizeof(float);
    out[2] = out[1] + n_patches * 8192 * (int64_t)sizeof(float);
    out[3] = out[2] + np * 16384 * (int64_t)sizeof(float);
    out[4] = np;
    enc_dense32_slices(&out[5], &out[6]);
    return CAELO_OK;
}

static int encode32_impl(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                         void *ws, void *stream, hipEvent_t *ev /* 5 events or null */) {
    CAELO_REQUIRE(c && bits && out && ws, "null argument");
    CAELO_REQUIRE(c->has_enc, "encoder weights not set (caelo_set_encoder_weights)");
    CAELO_REQUIRE(c->enc_hidden == CAELO_ACT_TANH && c->enc_code == CAELO_ACT_TANH, "the 32^3 path implements the tanh / tanh encoder only");
    CAELO_REQUIRE(c->enc32_wd1x, "32^3 dense_1 not set (caelo_set_encoder32_dense)");
    CAELO_REQUIRE(n_patches > 0 && n_patches < (1ll << 27) && group >= 1 && out_stride >= group * 20, "bad shape");
    hipStream_t s = caelo_stream(stream);
    const int64_t np = c5_pad(n_patches);
    float *p1 = (float *)ws;
    float *p2 = p1 + n_patches * 32768;
    float *f3 = p2 + n_patches * 8192;
    float *part = f3 + np * 16384;
    if (np > n_patches) CAELO_HIP(hipMemsetAsync(f3 + n_patches * 16384, 0, (size_t)(np - n_patches) * 16384 * sizeof(float), s));
    const int items1 = (int)(n_patches * 16);
    if (ev) CAELO_HIP(hipEventRecord(ev[0], s));
    k5_conv1pool_x3<<<items1 < 1024 ? items1 : 1024, 256, 0, s>>>((const unsigned long long *)bits, c->enc_w1, c->enc_b1, p1, items1);
    CAELO_LAUNCH_CHECK();
    if (ev) CAELO_HIP(hipEventRecord(ev[1], s));
    // persistent grids: the B operand (conv weights) is loaded into registers once per workgroup
    const int items2 = (int)(n_patches * 8), items3 = (int)(n_patches * 2);
    // (per call, i.e. for whichever device is current: this path is not a hot one)
    CAELO_HIP(hipFuncSetAttribute((const void *)k5_conv2_x3, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * X2_ARR));
    k5_conv2_x3<<<items2 < 512 ? items2 : 512, 256, 3 * X2_ARR, s>>>(p1, c->enc_w2, c->enc_b2, p2, items2);
    CAELO_LAUNCH_CHECK();
    if (ev) CAELO_HIP(hipEventRecord(ev[2], s));
    k5_conv3_x3<<<items3 < 512 ? items3 : 512, 256, 6 * X3_ARR, s>>>(p2, c->enc_w3, c->enc_b3, f3, items3);
    CAELO_LAUNCH_CHECK();
    if (ev) CAELO_HIP(hipEventRecord(ev[3], s));
    const int rc = enc_dense32_head_launch(c, f3, n_patches, np, part, group, out, out_stride, s);
    if (ev && rc == CAELO_OK) CAELO_HIP(hipEventRecord(ev[4], s));
    return rc;
}

CAELO_API int caelo_encode32(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                             void *ws, void *stream) {
    return encode32_impl(c, bits, n_patches, group, out, out_stride, ws, stream, nullptr);
}

// caelo_encode32 with a HIP event between its launches; synchronises; ms_host[4] = conv1+pool, conv2+pool, conv3, Dense(200)+head
CAELO_API int caelo_encode32_profile(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                                     void *ws, void *stream, float *ms_host) {
    CAELO_REQUIRE(ms_host != nullptr, "null argument");
    enc_prof_events pe;
    CAELO_HIP(pe.create());
    hipEvent_t *ev = pe.ev;
    int rc = encode32_impl(c, bits, n_patches, group, out, out_stride, ws, stream, ev);
    if (rc == CAELO_OK) {
        CAELO_HIP(hipEventSynchronize(ev[4]));
        for (int i = 0; i < 4; ++i) CAELO_HIP(hipEventElapsedTime(&ms_host[i], ev[i], ev[i + 1]));
    }
    return rc;
}
