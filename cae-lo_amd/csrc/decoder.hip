// decoder.hip -- the decoder half of AutoencoderModel4VoxelPatch.h5 (AE4VoxelPatch.py:199-211; autoencoder.predict, :256):
//   code [20] -> Dense(200) -> Dense(2048) -> Reshape(4,4,4,32) -> Conv3D(16) -> UpSampling3D(2) -> Conv3D(8) -> UpSampling3D(2)
//   -> Conv3D(1, sigmoid) -> 16^3 probabilities, with the reconstruction loss (Keras binary_crossentropy, :213) and the thresholded
//   voxels (Voxel.VoxelModel2PC keeps value > 0.1) taken in the last layer's epilogue.
//
// Arithmetic: f32 operands, f32 accumulation on v_mfma_f32_16x16x4_f32 (an exact fmaf chain over ascending k), fmaf on the VALU for
// the last layer.  Nothing is split into f16, so a relu decoder needs no range guard.  Every sum has ONE order that depends on
// nothing but the patch, so a patch's outputs are the same bits in any launch.
//
//   k_dec_dense  64 patches per workgroup.  h3 = act(code W3 + b3) (20 -> 200) into LDS, then G4 = act(h3 W4 + b4) as a
//                [64,200] x [200,2048] GEMM: a wavefront takes every fourth n-tile and keeps four m-tiles of accumulators per B
//                fragment (W4 is uploaded as ready B fragments, [n-tile][k-step][lane]).  G4 [n][2048] f32 goes to the workspace.
//   k_dec_conv   persistent, 512 threads, one patch at a time; conv4's kernel and the folded conv5 kernel stay in LDS (55 + 48 KB),
//                the patch's activations too (8 KB -> 4 KB -> 31 KB with the halo): 150 KB of the 160.
//                conv4: implicit GEMM, M = 64 cells (an m-tile = one x plane), N = 16, K = 27 x 32; the eight wavefronts are
//                  4 m-tiles x 2 halves of the input channels, the halves meet in LDS.  Taps are unrolled, so a tap is a constant
//                  offset from the lane's own cell; taps whose x plane is padding are skipped (their products are zeros).
//                conv5: UpSampling3D(2) + conv as eight parity classes of 2^3 taps on the 4^3 source (dec_fold.hip).  The two z
//                  parities of a class pair touch three source cells in z between them and share one 16-wide tile (8 channels
//                  each): per (px, py) M = 64 source cells, K = 2 x 2 x 3 x 16 with a third of B zero, N = 16 -- 48 k-steps
//                  where two 8-wide classes in half-empty tiles would take 64.
//                conv6: the same fold, K = 8 x 8, eight outputs per 8^3 source cell, one thread per source cell on the VALU; its
//                  input lies in LDS inside a halo of zeros, so no tap is tested.
//                epilogue: p = 1 / (1 + exp(-z)); voxel set <=> (double)p > threshold; a wavefront holds one x-pair of source cells,
//                  so its eight ballots (one per parity class) interleave into eight words of the packed layout; counts by popcount;
//                  loss = mean softplus(-+z) with z clipped to +-logit(1 - 1e-7): float terms summed in double, thread -> wavefront ->
//                  workgroup in a fixed tree, rounded to float once.
#include "caelo_internal.h"

#include <math.h>
#include <vector>

#define DEC_TILE 64           // patches per workgroup of k_dec_dense
#define DEC_H3_LD 201         // LDS leading dimension of h3 (201 = 9 mod 64 banks)
// the decoder's device image, in floats
#define DEC_O_WD3 0                           // [20][200]
#define DEC_O_BD3 (DEC_O_WD3 + 4000)          // [200]
#define DEC_O_WD4X (DEC_O_BD3 + 200)          // [n-tile 128][k-step 50][lane 64]: W4[k-step * 4 + (lane >> 4)][n-tile * 16 + (lane & 15)]
#define DEC_O_BD4 (DEC_O_WD4X + 409600)       // [2048]
#define DEC_O_W4 (DEC_O_BD4 + 2048)           // [27][32][16], Keras order = [k-step 216][lane 64] B fragments as it stands
#define DEC_O_B4 (DEC_O_W4 + 13824)           // [16]
#define DEC_O_W5F (DEC_O_B4 + 16)             // [px*2+py 4][(ox*2+oy)*3+dz 12][16][n 16]: B fragments [k-step 48][lane 64] per (px, py), see dec_pair_z
#define DEC_O_B5 (DEC_O_W5F + 12288)          // [8]
#define DEC_O_W6F (DEC_O_B5 + 8)              // [class 8][offset 8][8]
#define DEC_O_B6 (DEC_O_W6F + 512)            // [1]
#define DEC_IMAGE_FLOATS (DEC_O_B6 + 8)

// LDS of k_dec_conv, in floats
#define DC_X4_LD 33
#define DC_Y4_LD 17
#define DC_O_W4 0
#define DC_O_W5 (DC_O_W4 + 13824)
#define DC_O_X4 (DC_O_W5 + 12288)             // [64 cells][33]
#define DC_O_Y4 (DC_O_X4 + 64 * DC_X4_LD)     // [64 cells][17]
#define DC_O_Y5 (DC_O_Y4 + 64 * DC_Y4_LD)     // [10][10][10 cells][8]: the 8^3 grid inside a halo of zeros
#define DC_O_PART (DC_O_Y5 + 8000)            // conv4's second input-channel half: [m-tile 4][lane 64][4]
#define DC_O_TGT (DC_O_PART + 1024)           // the target's 64 words (u64)
#define DC_O_RED (DC_O_TGT + 128)             // [8] loss partials (f64), then [8][3] counts
#define DC_LDS_FLOATS (DC_O_RED + 40)
#define DC_LDS_BYTES (DC_LDS_FLOATS * 4)

#define DEC_LOGIT_CLIP 16.11809555f           // logit(1 - 1e-7) = log((1 - 1e-7) / 1e-7)

template <int H>
__device__ __forceinline__ float dec_act(float x) {
    if (H == CAELO_ACT_RELU) return x > 0.0f ? x : 0.0f;
    return tanhf(x);
}

// ------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(256) void k_dec_dense(const float *__restrict__ codes, int64_t n, int group, int ld, const float *__restrict__ W,
                                                   float *__restrict__ g4) {
    __shared__ float s_code[DEC_TILE * 20];
    __shared__ float s_h3[DEC_TILE * DEC_H3_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * DEC_TILE;
    for (int i = tid; i < DEC_TILE * 20; i += 256) {
        const int r = i / 20, j = i - r * 20;
        const int64_t p = row0 + r;
        s_code[i] = p < n ? codes[(p / group) * (int64_t)ld + (p % group) * 20 + j] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < DEC_TILE * 200; i += 256) {
        const int r = i / 200, c = i - r * 200;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 20; ++j) acc = fmaf(s_code[r * 20 + j], W[DEC_O_WD3 + j * 200 + c], acc);
        s_h3[r * DEC_H3_LD + c] = dec_act<H>(acc + W[DEC_O_BD3 + c]);
    }
    __syncthreads();
    const float *a_base = s_h3 + (lane & 15) * DEC_H3_LD + (lane >> 4);
    for (int nt = wave; nt < 128; nt += 4) {
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float *bp = W + DEC_O_WD4X + (size_t)nt * 50 * 64 + lane;
#pragma unroll 25
        for (int ks = 0; ks < 50; ++ks) {
            const float b = bp[ks * 64];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a_base[mt * 16 * DEC_H3_LD + ks * 4], b, acc[mt]);
        }
        const int col = nt * 16 + (lane & 15);
        const float bias = W[DEC_O_BD4 + col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t p = row0 + mt * 16 + 4 * (lane >> 4) + i;
                if (p < n) g4[p * 2048 + col] = dec_act<H>(acc[mt][i] + bias);
            }
    }
}

// ------------------------------------------------------------------------------------------------
struct DecConvArgs {
    const float *g4, *W;
    int64_t n;
    const unsigned long long *target;
    double threshold;
    float *prob;
    unsigned long long *rebuilt;
    float *loss;
    int32_t *counts;
};

// eight bits -> the even bits of sixteen
__device__ __forceinline__ unsigned long long dec_spread8(unsigned long long b) {
    b &= 0xFFull;
    b = (b | (b << 4)) & 0x0F0Full;
    b = (b | (b << 2)) & 0x3333ull;
    b = (b | (b << 1)) & 0x5555ull;
    return b;
}

template <int H>
__global__ __launch_bounds__(512) void k_dec_conv(const DecConvArgs a) {
    extern __shared__ float lds[];
    float *sW4 = lds + DC_O_W4, *sW5 = lds + DC_O_W5, *sX4 = lds + DC_O_X4, *sY4 = lds + DC_O_Y4, *sY5 = lds + DC_O_Y5, *sPart = lds + DC_O_PART;
    unsigned long long *sT = (unsigned long long *)(lds + DC_O_TGT);
    double *sLoss = (double *)(lds + DC_O_RED);
    int *sCnt = (int *)(lds + DC_O_RED + 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *W = a.W;
    for (int i = tid; i < 13824; i += 512) sW4[i] = W[DEC_O_W4 + i];
    for (int i = tid; i < 12288; i += 512) sW5[i] = W[DEC_O_W5F + i];
    for (int i = tid; i < 8000; i += 512) sY5[i] = 0.0f;   // the halo stays zero: only the 8^3 interior is ever written
    const int mt = wave & 3, kq = lane >> 4, r = lane & 15, ry = r >> 2, rz = r & 3;

    for (int64_t pn = blockIdx.x; pn < a.n; pn += gridDim.x) {
        // ---- G4 -> X4 [4][4][4][32] (Reshape: ((x*4+y)*4+z)*32+c), the target's words -------------------------------
        for (int i = tid; i < 2048; i += 512) sX4[(i >> 5) * DC_X4_LD + (i & 31)] = a.g4[pn * 2048 + i];
        if (tid < 64) sT[tid] = a.target ? a.target[pn * 64 + tid] : 0ull;
        __syncthreads();

        // ---- conv4: 4^3 x 32 -> 4^3 x 16; wavefront = (m-tile = x plane, half of the input channels) ---------------------
        {
            const int half = wave >> 2;
            f32x4 acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
            const float *ap = sX4 + (mt * 16 + r) * DC_X4_LD + half * 16 + kq;   // the lane's own cell; taps are compile-time offsets
            const float *bp = sW4 + half * 256 + lane;                            // k-step tap * 8 + half * 4 + cq
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                if (mt + tx - 1 < 0 || mt + tx - 1 > 3) continue;   // (wavefront-uniform) the whole plane is padding: its products are zeros
#pragma unroll
                for (int tyz = 0; tyz < 9; ++tyz) {
                    const int ty = tyz / 3, tz = tyz % 3, tap = tx * 9 + tyz;
                    const bool inb = (unsigned)(ry + ty - 1) < 4u && (unsigned)(rz + tz - 1) < 4u;
                    const int off = ((tx - 1) * 16 + (ty - 1) * 4 + (tz - 1)) * DC_X4_LD;   // (outside the plane: an address inside LDS, not used)
#pragma unroll
                    for (int cq = 0; cq < 4; cq += 2) {
                        const float a0 = inb ? ap[off + cq * 4] : 0.0f, a1 = inb ? ap[off + cq * 4 + 4] : 0.0f;
                        acc0 = MFMA16(a0, bp[(tap * 8 + cq) * 64], acc0);
                        acc1 = MFMA16(a1, bp[(tap * 8 + cq + 1) * 64], acc1);
                    }
                }
            }
            f32x4 acc = acc0 + acc1;
            if (half) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sPart[(mt * 64 + lane) * 4 + i] = acc[i];
            }
            __syncthreads();
            if (!half) {
                const float bias = W[DEC_O_B4 + r];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = acc[i] + sPart[(mt * 64 + lane) * 4 + i];
                    sY4[(mt * 16 + kq * 4 + i) * DC_Y4_LD + r] = dec_act<H>(v + bias);   // row 4*(lane>>4)+i = cell (y = lane>>4, z = i)
                }
            }
            __syncthreads();
        }

        // ---- conv5 behind UpSampling3D(2) on the 4^3 source -> 8^3 x 8; wavefront = (m-tile = source x plane, px), then py; the two
        //      z parities share one 16-wide tile (dec_pair_z): K = 2 x 2 x 3 source cells x 16 channels ---------------------------
        {
            const int px = wave >> 2;
            const float bias = W[DEC_O_B5 + (r & 7)];
            const float *ap = sY4 + (mt * 16 + r + (px - 1) * 16) * DC_Y4_LD + kq;
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                f32x4 acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
                const float *bp = sW5 + (px * 2 + py) * 3072 + lane;
#pragma unroll
                for (int ox = 0; ox < 2; ++ox) {
                    if (mt + ox + px - 1 < 0 || mt + ox + px - 1 > 3) continue;   // (wavefront-uniform)
#pragma unroll
                    for (int oyz = 0; oyz < 6; ++oyz) {
                        const int oy = oyz / 3, dz = oyz % 3, od = ox * 6 + oyz;
                        const bool inb = (unsigned)(ry + oy + py - 1) < 4u && (unsigned)(rz + dz - 1) < 4u;
                        const int off = (ox * 16 + (oy + py - 1) * 4 + (dz - 1)) * DC_Y4_LD;
#pragma unroll
                        for (int cq = 0; cq < 4; cq += 2) {
                            const float a0 = inb ? ap[off + cq * 4] : 0.0f, a1 = inb ? ap[off + cq * 4 + 4] : 0.0f;
                            acc0 = MFMA16(a0, bp[(od * 4 + cq) * 64], acc0);
                            acc1 = MFMA16(a1, bp[(od * 4 + cq + 1) * 64], acc1);
                        }
                    }
                }
                const f32x4 acc = acc0 + acc1;
#pragma unroll
                for (int i = 0; i < 4; ++i) {   // row 4*(lane>>4)+i = source cell (sy = lane>>4, sz = i); column = pz * 8 + channel
                    const int pos = ((2 * mt + px + 1) * 10 + (2 * kq + py + 1)) * 10 + 2 * i + (r >> 3) + 1;
                    sY5[pos * 8 + (r & 7)] = dec_act<H>(acc[i] + bias);
                }
            }
            __syncthreads();
        }

        // ---- conv6 behind UpSampling3D(2) + sigmoid, threshold, counts, loss: thread = source cell (wave, lane>>3, lane&7) ----
        {
            const int sx = wave, sy = lane >> 3, sz = lane & 7;
            const float b6 = W[DEC_O_B6];
            unsigned long long ballots[8];
            double lsum = 0.0;   // 4096 float terms per patch: summed in double, rounded once
#pragma unroll
            for (int pxy = 0; pxy < 4; ++pxy) {
                const int px = pxy >> 1, py = pxy & 1;
                float v[2][2][3][8];
#pragma unroll
                for (int ox = 0; ox < 2; ++ox)
#pragma unroll
                    for (int oy = 0; oy < 2; ++oy)
#pragma unroll
                        for (int dz = 0; dz < 3; ++dz) {   // source cell s + o + p - 1, + 1 for the halo
                            const float4 *cp = (const float4 *)(sY5 + (((sx + ox + px) * 10 + (sy + oy + py)) * 10 + (sz + dz)) * 8);
                            const float4 lo = cp[0], hi = cp[1];
                            v[ox][oy][dz][0] = lo.x; v[ox][oy][dz][1] = lo.y; v[ox][oy][dz][2] = lo.z; v[ox][oy][dz][3] = lo.w;
                            v[ox][oy][dz][4] = hi.x; v[ox][oy][dz][5] = hi.y; v[ox][oy][dz][6] = hi.z; v[ox][oy][dz][7] = hi.w;
                        }
                const int X = 2 * sx + px, Y = 2 * sy + py;
                const unsigned long long tw = sT[X * 4 + (Y >> 2)];
                float pr[2];
#pragma unroll
                for (int pz = 0; pz < 2; ++pz) {
                    const int cls = pxy * 2 + pz;
                    float z = b6;
#pragma unroll
                    for (int o = 0; o < 8; ++o)
#pragma unroll
                        for (int c = 0; c < 8; ++c) z = fmaf(v[o >> 2][(o >> 1) & 1][(o & 1) + pz][c], W[DEC_O_W6F + (cls * 8 + o) * 8 + c], z);
                    const float p = 1.0f / (1.0f + expf(-z));
                    pr[pz] = p;
                    ballots[cls] = __ballot((double)p > a.threshold);
                    if (a.loss) {
                        const int Z = 2 * sz + pz;
                        const bool y = (tw >> ((Y & 3) * 16 + Z)) & 1ull;
                        const float zc = fminf(fmaxf(z, -DEC_LOGIT_CLIP), DEC_LOGIT_CLIP);
                        const float t = y ? -zc : zc;   // -log p^ = softplus(-z), -log(1 - p^) = softplus(z)
                        lsum += (double)(fmaxf(t, 0.0f) + log1pf(expf(-fabsf(t))));
                    }
                }
                if (a.prob) *(float2 *)(a.prob + pn * 4096 + (X * 16 + Y) * 16 + 2 * sz) = float2{pr[0], pr[1]};
            }
            // word (X = 2 sx + px, yq): bit (Y & 3) * 16 + Z, Y = 4 yq + 2 sy1 + py, Z = 2 sz + pz; ballot bit = sy * 8 + sz, sy = 2 yq + sy1
            unsigned long long mine = 0ull;
#pragma unroll
            for (int wi = 0; wi < 8; ++wi) {
                const int px = wi >> 2, yq = wi & 3;
                unsigned long long word = 0ull;
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int pz = 0; pz < 2; ++pz)
#pragma unroll
                        for (int s1 = 0; s1 < 2; ++s1)
                            word |= dec_spread8(ballots[px * 4 + py * 2 + pz] >> ((2 * yq + s1) * 8)) << (pz + 16 * (2 * s1 + py));
                if (lane == wi) mine = word;
            }
            int c_in = 0, c_out = 0, c_both = 0;
            if (lane < 8) {
                const int widx = (2 * sx + (lane >> 2)) * 4 + (lane & 3);
                if (a.rebuilt) a.rebuilt[pn * 64 + widx] = mine;
                const unsigned long long t = sT[widx];
                c_in = __popcll(t); c_out = __popcll(mine); c_both = __popcll(t & mine);
            }
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) { c_in += __shfl_xor(c_in, o); c_out += __shfl_xor(c_out, o); c_both += __shfl_xor(c_both, o); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
            if (lane == 0) { sLoss[wave] = lsum; sCnt[wave * 3] = c_in; sCnt[wave * 3 + 1] = c_out; sCnt[wave * 3 + 2] = c_both; }
            __syncthreads();
            if (tid == 0) {
                double l = 0.0;
                int ci = 0, co = 0, cb = 0;
                for (int w = 0; w < 8; ++w) { l += sLoss[w]; ci += sCnt[w * 3]; co += sCnt[w * 3 + 1]; cb += sCnt[w * 3 + 2]; }
                if (a.loss) a.loss[pn] = (float)(l * (1.0 / 4096.0));
                if (a.counts) { a.counts[pn * 3] = ci; a.counts[pn * 3 + 1] = co; a.counts[pn * 3 + 2] = cb; }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
CAELO_API int caelo_set_decoder_model(caelo_ctx *c, const float *wd3, const float *bd3, const float *wd4, const float *bd4, const float *w4,
                                      const float *b4, const float *w5, const float *b5, const float *w6, const float *b6, int hidden, int out) {
    CAELO_REQUIRE(c && wd3 && bd3 && wd4 && bd4 && w4 && b4 && w5 && b5 && w6 && b6, "null argument");
    CAELO_REQUIRE(hidden == CAELO_ACT_TANH || hidden == CAELO_ACT_RELU, "hidden activation: tanh or relu");
    CAELO_REQUIRE(out == CAELO_ACT_SIGMOID, "output activation: sigmoid");
    std::vector<float> img(DEC_IMAGE_FLOATS, 0.0f);
    memcpy(&img[DEC_O_WD3], wd3, 4000 * sizeof(float));
    memcpy(&img[DEC_O_BD3], bd3, 200 * sizeof(float));
    for (int nt = 0; nt < 128; ++nt)
        for (int ks = 0; ks < 50; ++ks)
            for (int l = 0; l < 64; ++l) img[DEC_O_WD4X + ((size_t)nt * 50 + ks) * 64 + l] = wd4[(size_t)(ks * 4 + (l >> 4)) * 2048 + nt * 16 + (l & 15)];
    memcpy(&img[DEC_O_BD4], bd4, 2048 * sizeof(float));
    memcpy(&img[DEC_O_W4], w4, 13824 * sizeof(float));
    memcpy(&img[DEC_O_B4], b4, 16 * sizeof(float));
    std::vector<float> w5f(8 * 8 * 16 * 8);
    int rc = caelo_host_decoder_fold(w5, 16, 8, w5f.data());
    if (rc == CAELO_OK) rc = caelo_host_decoder_fold(w6, 8, 1, &img[DEC_O_W6F]);
    if (rc != CAELO_OK) return rc;
    // dec_pair_z: the two z parities of conv5 side by side in one 16-wide tile over the three source cells s_z - 1 + dz they touch
    // between them -- column pz * 8 + c takes folded[px, py, pz][ox, oy, oz = dz - pz] where that offset exists, zero elsewhere
    for (int pxy = 0; pxy < 4; ++pxy)
        for (int oxy = 0; oxy < 4; ++oxy)
            for (int dz = 0; dz < 3; ++dz)
                for (int ci = 0; ci < 16; ++ci)
                    for (int n = 0; n < 16; ++n) {
                        const int pz = n >> 3, oz = dz - pz;
                        if (oz < 0 || oz > 1) continue;
                        img[DEC_O_W5F + (((size_t)pxy * 12 + oxy * 3 + dz) * 16 + ci) * 16 + n] =
                            w5f[((((size_t)pxy * 2 + pz) * 8 + oxy * 2 + oz) * 16 + ci) * 8 + (n & 7)];
                    }
    memcpy(&img[DEC_O_B5], b5, 8 * sizeof(float));
    img[DEC_O_B6] = b6[0];
    CAELO_HIP(hipSetDevice(c->device));
    CAELO_HIP(hipDeviceSynchronize());   // work already issued may still read the previous image
    if (!c->dec_w) CAELO_HIP(hipMalloc((void **)&c->dec_w, DEC_IMAGE_FLOATS * sizeof(float)));
    CAELO_HIP(hipMemcpy(c->dec_w, img.data(), DEC_IMAGE_FLOATS * sizeof(float), hipMemcpyHostToDevice));
    c->dec_hidden = hidden;
    c->dec_out = out;
    c->has_dec = true;
    return CAELO_OK;
}

CAELO_API int caelo_get_decoder_activations(caelo_ctx *c, int32_t out[2]) {
    CAELO_REQUIRE(c && out, "null argument");
    CAELO_REQUIRE(c->has_dec, "no decoder model set (caelo_set_decoder_model)");
    out[0] = c->dec_hidden;
    out[1] = c->dec_out;
    return CAELO_OK;
}

CAELO_API int64_t caelo_decode_ws_bytes(int64_t n_patches) { return (n_patches > 0 ? n_patches : 1) * (int64_t)(2048 * sizeof(float)); }

CAELO_API int caelo_decode_ws_layout(int64_t n_patches, int64_t out[2]) {
    CAELO_REQUIRE(out && n_patches >= 0, "null argument or a negative patch count");
    out[0] = 0;           // G4 [n][2048] f32, activated
    out[1] = n_patches;   // its rows
    return CAELO_OK;
}

template <int H>
static int dec_launch(caelo_ctx *c, const float *codes, int64_t n, int group, int ld, const DecConvArgs &ca, float *g4, hipStream_t s) {
    // once per device (under a lock: callers on several threads may race here) -- the attribute belongs to the device that is
    // current when it is set, the CU count to the context's device
    static hipError_t attr_slot[CAELO_MAX_DEVICES];
    static bool attr_have[CAELO_MAX_DEVICES];
    static std::mutex attr_mu;
    CAELO_HIP(per_device_once(c->device, attr_slot, attr_have, attr_mu, [] {
        return hipFuncSetAttribute((const void *)k_dec_conv<H>, hipFuncAttributeMaxDynamicSharedMemorySize, DC_LDS_BYTES);
    }));
    static int cus_slot[CAELO_MAX_DEVICES];
    static bool cus_have[CAELO_MAX_DEVICES];
    static std::mutex cus_mu;
    const int cus = per_device_once(c->device, cus_slot, cus_have, cus_mu, [&] {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || v <= 0) return 256;   // MI355X
        return v;
    });
    k_dec_dense<H><<<(unsigned)((n + DEC_TILE - 1) / DEC_TILE), 256, 0, s>>>(codes, n, group, ld, c->dec_w, g4);
    CAELO_LAUNCH_CHECK();
    k_dec_conv<H><<<(unsigned)(n < cus ? n : cus), 512, DC_LDS_BYTES, s>>>(ca);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

CAELO_API int caelo_decode(caelo_ctx *c, const float *codes, int64_t n_patches, int group, int ld, const uint64_t *target_bits, double threshold,
                           float *prob, uint64_t *rebuilt, float *loss, int32_t *counts, void *ws, void *stream) {
    CAELO_REQUIRE(c != nullptr, "null context");
    CAELO_REQUIRE(c->has_dec, "no decoder model set (caelo_set_decoder_model)");
    CAELO_REQUIRE(n_patches >= 0 && n_patches < ((int64_t)1 << 31) * DEC_TILE, "patch count out of range");
    CAELO_REQUIRE(group >= 1 && ld >= 0 && (int64_t)group * 20 <= (int64_t)ld, "codes: group >= 1 and group * 20 <= ld");
    CAELO_REQUIRE(threshold > 0.0 && threshold < 1.0, "threshold must lie in (0, 1)");   // (false for NaN)
    CAELO_REQUIRE(prob || rebuilt || loss || counts, "no output requested");
    CAELO_REQUIRE(!loss || target_bits, "the loss needs the target patches");
    if (n_patches == 0) return CAELO_OK;
    CAELO_REQUIRE(codes && ws, "null codes or workspace");
    DecConvArgs ca;
    ca.g4 = (const float *)ws;
    ca.W = c->dec_w;
    ca.n = n_patches;
    ca.target = (const unsigned long long *)target_bits;
    ca.threshold = threshold;
    ca.prob = prob;
    ca.rebuilt = (unsigned long long *)rebuilt;
    ca.loss = loss;
    ca.counts = counts;
    hipStream_t s = caelo_stream(stream);
    if (c->dec_hidden == CAELO_ACT_RELU) return dec_launch<CAELO_ACT_RELU>(c, codes, n_patches, group, ld, ca, (float *)ws, s);
    return dec_launch<CAELO_ACT_TANH>(c, codes, n_patches, group, ld, ca, (float *)ws, s);
}
