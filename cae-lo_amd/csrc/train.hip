// train.hip -- loss and gradient of the voxel-patch autoencoder (AE4VoxelPatch.py:186-213) and Keras 2.3's Adadelta step.
//   encoder  Conv3D(1->8) MaxPool(2) Conv3D(8->16) MaxPool(2) Conv3D(16->32) Flatten Dense(200) Dense(20)
//   decoder  Dense(200) Dense(2048) Reshape(4,4,4,32) Conv3D(16) UpSampling3D(2) Conv3D(8) UpSampling3D(2) Conv3D(1, sigmoid)
// on plain Keras-layout f32 weights in ONE flat buffer of 864 741 floats (20 tensors, caelo_train_param_layout); the gradient has the
// same layout.  A layer's kernel [.., Cin, Cout] is followed by its bias [Cout], so kernel and bias together are one row-major
// [rows + 1][Cout] matrix: every weight-gradient GEMM below carries a row of ones behind its A operand and the bias gradient falls out.
//
// Arithmetic: f32 operands, f32 accumulation on v_mfma_f32_16x16x4_f32 (an exact fmaf chain over ascending k, as in decoder.hip), a sum
// over K as four such chains.  No floating-point atomics.  Every output element has one owner (a wavefront's accumulator) and one order
// of summation.  Shared with train_ring.hip and defined once in train_common.h: the chains (CHAINS_*), the B operand's staging
// (tc_stage_b), k_tc_wreduce, tc_wave_sum, tc_block_sum, the workspace and parameter layout helpers, the optimizer launcher.  Here:
//   k_tr_conv    forward convs and data gradients as implicit GEMMs, M = cells x patches (an m-tile = 16 consecutive cells), N = output
//                channels, K = 27 x input channels over ascending (tap, channel).  The data gradient is the same kernel with the Keras
//                kernel flipped and its channel axes swapped while it is staged in LDS.  The input is read in place: plain, through
//                UpSampling3D(2) (cell u reads source cell u >> 1: nothing is materialised going forward), or from the bit-packed patch.
//   k_tr_wgrad   a conv's weight gradient: M = 27 Cin + 1, N = Cout, K = cells x patches split into slices of 256 cells, one
//                (m-tile, slice) per wavefront; k_tc_wreduce adds a chunk's slices in a fixed order in double, then that sum to the gradient.
//   k_tr_gemm    the dense layers, their data gradients and their weight gradients (K = the chunk's patches, added to the gradient).
//   pooling      the gradient of a window goes to its FIRST maximum in ascending (dx, dy, dz) order, dz fastest (k_tr_unpool);
//                UpSampling3D's adjoint is the sum of the eight children in that same order (k_tr_upsum).
//   loss         softplus(-+z) with z clipped to +-logit(1 - 1e-7), float terms summed in double per patch in a fixed tree (k_tr_loss),
//                patches added in ascending order in double, rounded once (k_tr_loss_acc): the loss bits depend on n alone, not on the chunk.
// The batch is walked in chunks of `chunk` patches (the workspace holds one chunk's activations and their gradients, tr_layout); chunk
// partials are added in ascending chunk order, so the gradient bits are fixed by (n, chunk).
#include "train_common.h"

#define TR_LOGIT_CLIP 16.11809555f   // logit(1 - 1e-7), decoder.hip's DEC_LOGIT_CLIP
#define TR_SLICE 256                 // cells per K slice of a conv weight gradient
#define TR_MAX_CHUNK 8192

// the 20 tensors, in floats: netref64.ENCODER_SHAPES then netref64_dec.DECODER_SHAPES
static const int64_t TR_COUNT[20] = {216, 8, 3456, 16, 13824, 32, 409600, 200, 4000, 20, 4000, 200, 409600, 2048, 13824, 16, 3456, 8, 216, 1};
enum {
    P_W1 = 0, P_B1 = 216, P_W2 = 224, P_B2 = 3680, P_W3 = 3696, P_B3 = 17520, P_WD1 = 17552, P_BD1 = 427152, P_WD2 = 427352, P_BD2 = 431352,
    P_WD3 = 431372, P_BD3 = 435372, P_WD4 = 435572, P_BD4 = 845172, P_W4 = 847220, P_B4 = 861044, P_W5 = 861060, P_B5 = 864516,
    P_W6 = 864524, P_B6 = 864740, P_TOTAL = 864741
};

// one chunk's workspace, offsets in floats behind the (1 + chunk) doubles of the loss
struct TrLayout {
    int64_t a1, p1, a2, p2, f3, h1, code, h3, g4, y4, y5, z;                                              // saved activations
    int64_t dz, du5, dy5, du4, dy4, dg4, dh3, dcode, dcodep, dh1, df3, dp2, da2, dp1, da1, part, total;   // their gradients, slice partials
    int64_t base_bytes;   // where the floats begin
};

static TrLayout tr_layout(int64_t c) {
    TrLayout L;
    TcTake take{c, 0};
    L.a1 = take(32768); L.p1 = take(4096); L.a2 = take(8192); L.p2 = take(1024); L.f3 = take(2048); L.h1 = take(200); L.code = take(20);
    L.h3 = take(200); L.g4 = take(2048); L.y4 = take(1024); L.y5 = take(4096); L.z = take(4096);
    L.dz = take(4096); L.du5 = take(32768); L.dy5 = take(4096); L.du4 = take(8192); L.dy4 = take(1024); L.dg4 = take(2048); L.dh3 = take(200);
    L.dcode = take(20); L.dcodep = take(20); L.dh1 = take(200); L.df3 = take(2048); L.dp2 = take(1024); L.da2 = take(8192); L.dp1 = take(4096);
    L.da1 = take(32768);
    // slice partials: conv2 2c x 217 x 16 is the largest per patch, conv3 ceil(c / 4) x 433 x 32 the largest per slice
    L.part = take.o;
    L.total = take.o + 6944 * c + 13856 * (c / 4 + 1);
    L.base_bytes = ((1 + c) * 8 + 255) / 256 * 256;
    return L;
}

__device__ __forceinline__ float tr_act(float x, int act) {
    if (act == CAELO_ACT_RELU) return x > 0.0f ? x : 0.0f;
    if (act == CAELO_ACT_TANH) return tanhf(x);
    return x;
}

// the activation's derivative from its stored OUTPUT: relu' = y > 0 (0 at 0), tanh' = 1 - y^2, linear' = 1
__device__ __forceinline__ float tr_dact(float y, int act) {
    if (act == CAELO_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (act == CAELO_ACT_TANH) return 1.0f - y * y;
    return 1.0f;
}

// INMODE: how a conv reads its input tensor
#define TR_IN_PLAIN 0   // [p][S^3][CIN] f32
#define TR_IN_UP 1      // [p][(S/2)^3][CIN] f32 behind UpSampling3D(2)
#define TR_IN_BITS 2    // [p][64] u64, CIN = 1, S = 16

// input value at cell (x, y, z) of patch p, channel ci; the cell is inside the grid
template <int CIN, int S, int INMODE>
__device__ __forceinline__ float tr_in(const void *in, int p, int x, int y, int z, int ci) {
    if (INMODE == TR_IN_BITS) {
        const int lin = (x * 16 + y) * 16 + z;
        return (float)((((const unsigned long long *)in)[(size_t)p * 64 + (lin >> 6)] >> (lin & 63)) & 1ull);
    }
    if (INMODE == TR_IN_UP) {
        const int H = S / 2;
        return ((const float *)in)[((size_t)((p * H + (x >> 1)) * H + (y >> 1)) * H + (z >> 1)) * CIN + ci];
    }
    return ((const float *)in)[((size_t)((p * S + x) * S + y) * S + z) * CIN + ci];
}

// ------------------------------------------------------------------------------------------------
// out[row][co] = act(sum_{tap, ci} in[cell(row) + tap - 1][ci] B[tap * CIN + ci][co] + bias[co]); rows = S^3 x patches (a multiple of 16).
// B = the Keras kernel W [27][CIN][COUT] as it stands, or (FLIP: the data gradient of a conv whose kernel is W [27][COUT][CIN])
// B[tap * CIN + ci][co] = W[26 - tap][co][ci].
template <int CIN, int COUT, int S, int INMODE, bool FLIP>
__global__ __launch_bounds__(256) void k_tr_conv(const void *__restrict__ in, const float *__restrict__ W, const float *__restrict__ bias,
                                                 float *__restrict__ out, int rows, int act) {
    constexpr int K4 = (27 * CIN + 3) / 4 * 4, NP = (COUT + 15) / 16 * 16, NT = NP / 16;
    extern __shared__ float sB[];   // [K4][NP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    tc_stage_b<27, CIN, COUT, FLIP>(sB, W, tid);
    __syncthreads();
    const int tiles = rows >> 4;
    for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
        const int row = tile * 16 + r;
        const int p = row / (S * S * S), cell = row - p * (S * S * S);
        const int x = cell / (S * S), y = (cell / S) % S, z = cell % S;
        f32x4 acc[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) CHAINS_ZERO(acc[nt]);
        if (CIN >= 4) {
#pragma unroll
            for (int tap = 0; tap < 27; ++tap) {
                const int xx = x + tap / 9 - 1, yy = y + (tap / 3) % 3 - 1, zz = z + tap % 3 - 1;
                const bool inb = (unsigned)xx < (unsigned)S && (unsigned)yy < (unsigned)S && (unsigned)zz < (unsigned)S;
#pragma unroll
                for (int cq = 0; cq < CIN / 4; ++cq) {
                    const float a = inb ? tr_in<CIN, S, INMODE>(in, p, xx, yy, zz, cq * 4 + kq) : 0.0f;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) CHAINS_STEP(acc[nt], tap * (CIN / 4) + cq, a, sB[(tap * CIN + cq * 4 + kq) * NP + nt * 16 + r]);
                }
            }
        } else {   // CIN == 1: a k-step spans four taps
#pragma unroll
            for (int ks = 0; ks < K4 / 4; ++ks) {
                const int tap = ks * 4 + kq;
                const int xx = x + tap / 9 - 1, yy = y + (tap / 3) % 3 - 1, zz = z + tap % 3 - 1;
                const bool inb = tap < 27 && (unsigned)xx < (unsigned)S && (unsigned)yy < (unsigned)S && (unsigned)zz < (unsigned)S;
                const float a = inb ? tr_in<CIN, S, INMODE>(in, p, xx, yy, zz, 0) : 0.0f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) CHAINS_STEP(acc[nt], ks, a, sB[tap * NP + nt * 16 + r]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 16 + r;
            if (col < COUT) {
                const float b = bias ? bias[col] : 0.0f;
                const f32x4 sum = CHAINS_JOIN(acc[nt]);
#pragma unroll
                for (int i = 0; i < 4; ++i) out[(size_t)(tile * 16 + 4 * kq + i) * COUT + col] = tr_act(sum[i] + b, act);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// part[slice][m][co] = sum over the slice's rows of A[m][row] delta[row][co], m = tap * CIN + ci: A = in[cell(row) + tap - 1][ci],
// and A = 1 for m = 27 CIN (the bias).  One (m-tile, slice) per wavefront; rows ascending.
template <int CIN, int COUT, int S, int INMODE>
__global__ __launch_bounds__(256) void k_tr_wgrad(const void *__restrict__ in, const float *__restrict__ delta, float *__restrict__ part, int rows,
                                                  int nsl) {
    constexpr int M = 27 * CIN, M1 = M + 1, MT = (M1 + 15) / 16, NP = (COUT + 15) / 16 * 16, NT = NP / 16;
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int mt = w % MT, sl = w / MT;
    if (sl >= nsl) return;   // (wavefront-uniform)
    const int m = mt * 16 + r, tap = m / CIN, ci = m - tap * CIN;
    const int tx = tap / 9 - 1, ty = (tap / 3) % 3 - 1, tz = tap % 3 - 1;
    f32x4 acc[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) CHAINS_ZERO(acc[nt]);
#pragma unroll 4
    for (int ks = 0; ks < TR_SLICE / 4; ++ks) {
        const int row = sl * TR_SLICE + ks * 4 + kq;
        const bool live = row < rows;
        float a = 0.0f;
        if (live) {
            if (m == M) {
                a = 1.0f;
            } else if (m < M) {
                const int p = row / (S * S * S), cell = row - p * (S * S * S);
                const int xx = cell / (S * S) + tx, yy = (cell / S) % S + ty, zz = cell % S + tz;
                if ((unsigned)xx < (unsigned)S && (unsigned)yy < (unsigned)S && (unsigned)zz < (unsigned)S) a = tr_in<CIN, S, INMODE>(in, p, xx, yy, zz, ci);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 16 + r;
            const float b = live && col < COUT ? delta[(size_t)row * COUT + col] : 0.0f;
            CHAINS_STEP(acc[nt], ks, a, b);
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = nt * 16 + r;
        const f32x4 sum = CHAINS_JOIN(acc[nt]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mrow = mt * 16 + 4 * kq + i;
            if (mrow < M1 && col < COUT) part[((size_t)sl * M1 + mrow) * COUT + col] = sum[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// MaxPooling3D(2): A [p][(2S)^3][C] -> P [p][S^3][C]
template <int C, int S>
__global__ __launch_bounds__(256) void k_tr_pool(const float *__restrict__ A, float *__restrict__ P, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = i % C, cell = (i / C) % (S * S * S), p = i / (C * S * S * S);
    const int x = cell / (S * S), y = (cell / S) % S, z = cell % S;
    float best = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const float v = A[((size_t)((p * 2 * S + 2 * x + (o >> 2)) * 2 * S + 2 * y + ((o >> 1) & 1)) * 2 * S + 2 * z + (o & 1)) * C + ch];
        if (o == 0 || v > best) best = v;
    }
    P[i] = best;
}

// its gradient: dA = act'(A) dP at the window's first maximum in ascending (dx, dy, dz) order, 0 at the other seven cells
template <int C, int S>
__global__ __launch_bounds__(256) void k_tr_unpool(const float *__restrict__ A, const float *__restrict__ dP, float *__restrict__ dA, int total, int act) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = i % C, cell = (i / C) % (S * S * S), p = i / (C * S * S * S);
    const int x = cell / (S * S), y = (cell / S) % S, z = cell % S;
    float best = 0.0f;
    int arg = 0;
    size_t at[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        at[o] = ((size_t)((p * 2 * S + 2 * x + (o >> 2)) * 2 * S + 2 * y + ((o >> 1) & 1)) * 2 * S + 2 * z + (o & 1)) * C + ch;
        const float v = A[at[o]];
        if (o == 0 || v > best) { best = v; arg = o; }
    }
    const float g = dP[i] * tr_dact(best, act);
#pragma unroll
    for (int o = 0; o < 8; ++o) dA[at[o]] = o == arg ? g : 0.0f;
}

// UpSampling3D(2)'s adjoint with the source layer's activation: dY [p][S^3][C] = act'(Y) x the sum of dU over the eight children
template <int C, int S>
__global__ __launch_bounds__(256) void k_tr_upsum(const float *__restrict__ dU, const float *__restrict__ Y, float *__restrict__ dY, int total, int act) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = i % C, cell = (i / C) % (S * S * S), p = i / (C * S * S * S);
    const int x = cell / (S * S), y = (cell / S) % S, z = cell % S;
    float s = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; ++o)
        s += dU[((size_t)((p * 2 * S + 2 * x + (o >> 2)) * 2 * S + 2 * y + ((o >> 1) & 1)) * 2 * S + 2 * z + (o & 1)) * C + ch];
    dY[i] = s * tr_dact(Y[i], act);
}

__global__ __launch_bounds__(256) void k_tr_actgrad(float *__restrict__ out, const float *__restrict__ d, const float *__restrict__ y, int count, int act) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = d[i] * tr_dact(y[i], act);
}

// ------------------------------------------------------------------------------------------------
// C [M][N] (ldc) = A [M][K] x B [K][N], A(m, k) = A[m sam + k sak] (ones: A(M - 1, k) = 1), B(k, n) = B[k sbk + n sbn]; one 16 x 16 tile per
// wavefront, k ascending.  mode 0: C = act(acc + bias[n]); 1: C = acc; 2: C += acc
struct TrGemm {
    const float *A, *B, *bias;
    float *C;
    int64_t sam, sak, sbk, sbn, ldc;
    int M, N, K, act, mode, ones;
};

__global__ __launch_bounds__(256) void k_tr_gemm(const TrGemm g) {
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
    const int tn = (g.N + 15) / 16, tm = (g.M + 15) / 16;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= tn * tm) return;   // (wavefront-uniform)
    const int m = (tile / tn) * 16 + r, n = (tile % tn) * 16 + r;
    const bool one = g.ones && m == g.M - 1, am = m < g.M, bn = n < g.N;
    const float *ap = g.A + (int64_t)m * g.sam, *bp = g.B + (int64_t)n * g.sbn;
    f32x4 acc4[4];
    CHAINS_ZERO(acc4);
    for (int k0 = 0; k0 < g.K; k0 += 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * j + kq;
            const bool kin = k < g.K;
            const float a = kin && am ? (one ? 1.0f : ap[(int64_t)k * g.sak]) : 0.0f;
            const float b = kin && bn ? bp[(int64_t)k * g.sbk] : 0.0f;
            CHAINS_STEP(acc4, j, a, b);
        }
    }
    const f32x4 acc = CHAINS_JOIN(acc4);
    if (!bn) return;
    const float bias = g.mode == 0 && g.bias ? g.bias[n] : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int mrow = (tile / tn) * 16 + 4 * kq + i;
        if (mrow >= g.M) continue;
        float *cp = g.C + (int64_t)mrow * g.ldc + n;
        if (g.mode == 0) *cp = tr_act(acc[i] + bias, g.act);
        else if (g.mode == 1) *cp = acc[i];
        else *cp += acc[i];
    }
}

// ------------------------------------------------------------------------------------------------
// one workgroup per patch: its 4096 loss terms summed in double (thread, then tc_block_sum: a fixed tree), and
// dz = (sigmoid(z) - y) scale where |z| <= the clip, 0 beyond it
__global__ __launch_bounds__(256) void k_tr_loss(const float *__restrict__ z, const unsigned long long *__restrict__ bits, float *__restrict__ dz,
                                                 double *__restrict__ patch_loss, float scale) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const unsigned long long word = bits[(size_t)p * 64 + (tid >> 2)];
    double lsum = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int lin = tid * 16 + j;
        const bool y = (word >> (lin & 63)) & 1ull;
        const float v = z[(size_t)p * 4096 + lin];
        const float zc = fminf(fmaxf(v, -TR_LOGIT_CLIP), TR_LOGIT_CLIP);
        const float t = y ? -zc : zc;
        lsum += (double)(fmaxf(t, 0.0f) + log1pf(expf(-fabsf(t))));
        if (dz) {
            const float s = 1.0f / (1.0f + expf(-v));
            dz[(size_t)p * 4096 + lin] = fabsf(v) <= TR_LOGIT_CLIP ? (s - (y ? 1.0f : 0.0f)) * scale : 0.0f;
        }
    }
    tc_block_sum(lsum, patch_loss + p);
}

// the chunk's patches onto the running sum, ascending; the last chunk rounds the mean once (k_rt_loss_acc's order at one sum per image, minus its butterflies)
__global__ void k_tr_loss_acc(const double *__restrict__ patch_loss, int c, double *__restrict__ acc, int first, int last, double count,
                              float *__restrict__ loss) {
    if (threadIdx.x || blockIdx.x) return;
    double a = first ? 0.0 : *acc;
    for (int i = 0; i < c; ++i) a += patch_loss[i];
    *acc = a;
    if (last) *loss = (float)(a / count);
}

// ------------------------------------------------------------------------------------------------
// Keras 2.3 Adadelta, every operation rounded on its own in f32 (the file is built with -ffp-contract=off).  The square root and the
// quotient go through f64, whose 53 bits >= 2 x 24 + 2 make the value rounded back to f32 the correctly rounded f32 result whatever
// the compiler's f32 sqrt / division expansion is.
__device__ __forceinline__ float tr_sqrt_rn(float x) { return (float)sqrt((double)x); }

__global__ __launch_bounds__(256) void k_tr_adadelta(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ acc_g,
                                                     float *__restrict__ acc_d, int64_t count, float lr, float rho, float eps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float one_rho = 1.0f - rho;
    const float gi = g[i], d = acc_d[i];
    const float g2 = gi * gi;
    const float a = rho * acc_g[i] + one_rho * g2;
    const float num = gi * tr_sqrt_rn(d + eps);
    const float u = (float)((double)num / (double)tr_sqrt_rn(a + eps));
    const float u2 = u * u;
    acc_g[i] = a;
    p[i] = p[i] - lr * u;
    acc_d[i] = rho * d + one_rho * u2;
}

// ================================================================================================
CAELO_API int caelo_train_param_layout(int64_t out[20][2]) {
    CAELO_REQUIRE(out != nullptr, "null argument");
    tc_param_layout(TR_COUNT, 20, out);
    return CAELO_OK;
}

CAELO_API int64_t caelo_train_ws_bytes(int64_t chunk) {
    if (chunk < 1 || chunk > TR_MAX_CHUNK) return 0;
    const TrLayout L = tr_layout(chunk);
    return L.base_bytes + L.total * (int64_t)sizeof(float);
}

CAELO_API int caelo_train_ws_layout(int64_t chunk, int64_t out[3]) {
    CAELO_REQUIRE(out && chunk >= 1 && chunk <= TR_MAX_CHUNK, "null argument, or chunk outside [1, 8192]");
    const TrLayout L = tr_layout(chunk);
    out[0] = L.base_bytes + L.dz * 4;      // dL/dz [chunk][4096]
    out[1] = L.base_bytes + L.dcode * 4;   // dL/dcode [chunk][20]
    out[2] = L.base_bytes + L.dp1 * 4;     // dL/dP1 [chunk][8^3 x 8]
    return CAELO_OK;
}

template <int CIN, int COUT, int S, int INMODE, bool FLIP>
static void tr_conv(const void *in, const float *W, const float *bias, float *out, int rows, int act, hipStream_t s) {
    constexpr int K4 = (27 * CIN + 3) / 4 * 4, NP = (COUT + 15) / 16 * 16;
    const int tiles = rows / 16;
    int blocks = (tiles + 15) / 16;   // four tiles per wavefront amortise the kernel's trip through LDS
    if (blocks > 2048) blocks = 2048;
    k_tr_conv<CIN, COUT, S, INMODE, FLIP><<<blocks, 256, K4 * NP * sizeof(float), s>>>(in, W, bias, out, rows, act);
}

template <int CIN, int COUT, int S, int INMODE>
static void tr_wgrad(const void *in, const float *delta, float *part, float *dst, int rows, hipStream_t s) {
    constexpr int M1 = 27 * CIN + 1, MT = (M1 + 15) / 16;
    const int nsl = (rows + TR_SLICE - 1) / TR_SLICE, count = M1 * COUT;
    k_tr_wgrad<CIN, COUT, S, INMODE><<<(MT * nsl + 3) / 4, 256, 0, s>>>(in, delta, part, rows, nsl);
    tc_wreduce(part, nsl, count, dst, s);
}

static void tr_gemm(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, float *C, int64_t ldc, int M, int N, int K,
                    const float *bias, int act, int mode, int ones, hipStream_t s) {
    TrGemm g;
    g.A = A; g.B = B; g.bias = bias; g.C = C;
    g.sam = sam; g.sak = sak; g.sbk = sbk; g.sbn = sbn; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.act = act; g.mode = mode; g.ones = ones;
    const int tiles = ((M + 15) / 16) * ((N + 15) / 16);
    k_tr_gemm<<<(tiles + 3) / 4, 256, 0, s>>>(g);
}

static inline unsigned tr_blocks(int64_t total) { return (unsigned)((total + 255) / 256); }

CAELO_API int caelo_autoencoder_grad(caelo_ctx *c, const float *params, int enc_hidden, int enc_code, int dec_hidden, const uint64_t *bits, int64_t n,
                                     int64_t chunk, float *grads, float *loss, void *ws, void *stream) {
    CAELO_REQUIRE(c != nullptr, "null context");
    CAELO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "patch count out of range");
    CAELO_REQUIRE(chunk >= 1 && chunk <= TR_MAX_CHUNK, "chunk outside [1, 8192]");
    CAELO_REQUIRE(params && loss && ws && (bits || n == 0), "null params, loss, workspace or patches");
    CAELO_REQUIRE(enc_hidden == CAELO_ACT_TANH || enc_hidden == CAELO_ACT_RELU, "encoder hidden activation: tanh or relu");
    CAELO_REQUIRE(enc_code == CAELO_ACT_TANH || enc_code == CAELO_ACT_LINEAR, "code activation: tanh or linear");
    CAELO_REQUIRE(dec_hidden == CAELO_ACT_TANH || dec_hidden == CAELO_ACT_RELU, "decoder hidden activation: tanh or relu");
    hipStream_t s = caelo_stream(stream);
    if (grads) CAELO_HIP(hipMemsetAsync(grads, 0, P_TOTAL * sizeof(float), s));
    if (n == 0) {
        CAELO_HIP(hipMemsetAsync(loss, 0, sizeof(float), s));
        return CAELO_OK;
    }
    const TrLayout L = tr_layout(chunk);
    double *lacc = (double *)ws, *ploss = lacc + 1;
    float *f = (float *)((char *)ws + L.base_bytes);
    const float *P = params;
    float *G = grads;
    const float scale = (float)(1.0 / (4096.0 * (double)n));
    const int eh = enc_hidden, ec = enc_code, dh = dec_hidden, lin = CAELO_ACT_LINEAR;

    for (int64_t start = 0; start < n; start += chunk) {
        const int cc = (int)(n - start < chunk ? n - start : chunk);
        const unsigned long long *b = (const unsigned long long *)bits + start * 64;
        // ---- forward ------------------------------------------------------------------------------------------------------------
        tr_conv<1, 8, 16, TR_IN_BITS, false>(b, P + P_W1, P + P_B1, f + L.a1, 4096 * cc, eh, s);
        k_tr_pool<8, 8><<<tr_blocks(4096 * cc), 256, 0, s>>>(f + L.a1, f + L.p1, 4096 * cc);
        tr_conv<8, 16, 8, TR_IN_PLAIN, false>(f + L.p1, P + P_W2, P + P_B2, f + L.a2, 512 * cc, eh, s);
        k_tr_pool<16, 4><<<tr_blocks(1024 * cc), 256, 0, s>>>(f + L.a2, f + L.p2, 1024 * cc);
        tr_conv<16, 32, 4, TR_IN_PLAIN, false>(f + L.p2, P + P_W3, P + P_B3, f + L.f3, 64 * cc, eh, s);
        tr_gemm(f + L.f3, 2048, 1, P + P_WD1, 200, 1, f + L.h1, 200, cc, 200, 2048, P + P_BD1, eh, 0, 0, s);
        tr_gemm(f + L.h1, 200, 1, P + P_WD2, 20, 1, f + L.code, 20, cc, 20, 200, P + P_BD2, ec, 0, 0, s);
        tr_gemm(f + L.code, 20, 1, P + P_WD3, 200, 1, f + L.h3, 200, cc, 200, 20, P + P_BD3, dh, 0, 0, s);
        tr_gemm(f + L.h3, 200, 1, P + P_WD4, 2048, 1, f + L.g4, 2048, cc, 2048, 200, P + P_BD4, dh, 0, 0, s);
        tr_conv<32, 16, 4, TR_IN_PLAIN, false>(f + L.g4, P + P_W4, P + P_B4, f + L.y4, 64 * cc, dh, s);
        tr_conv<16, 8, 8, TR_IN_UP, false>(f + L.y4, P + P_W5, P + P_B5, f + L.y5, 512 * cc, dh, s);
        tr_conv<8, 1, 16, TR_IN_UP, false>(f + L.y5, P + P_W6, P + P_B6, f + L.z, 4096 * cc, lin, s);
        k_tr_loss<<<cc, 256, 0, s>>>(f + L.z, b, G ? f + L.dz : nullptr, ploss, scale);
        k_tr_loss_acc<<<1, 64, 0, s>>>(ploss, cc, lacc, start == 0, start + chunk >= n, 4096.0 * (double)n, loss);
        CAELO_LAUNCH_CHECK();
        if (!G) continue;
        // ---- backward: the decoder ---------------------------------------------------------------------------------------------------
        tr_wgrad<8, 1, 16, TR_IN_UP>(f + L.y5, f + L.dz, f + L.part, G + P_W6, 4096 * cc, s);
        tr_conv<1, 8, 16, TR_IN_PLAIN, true>(f + L.dz, P + P_W6, nullptr, f + L.du5, 4096 * cc, lin, s);
        k_tr_upsum<8, 8><<<tr_blocks(4096 * cc), 256, 0, s>>>(f + L.du5, f + L.y5, f + L.dy5, 4096 * cc, dh);
        tr_wgrad<16, 8, 8, TR_IN_UP>(f + L.y4, f + L.dy5, f + L.part, G + P_W5, 512 * cc, s);
        tr_conv<8, 16, 8, TR_IN_PLAIN, true>(f + L.dy5, P + P_W5, nullptr, f + L.du4, 512 * cc, lin, s);
        k_tr_upsum<16, 4><<<tr_blocks(1024 * cc), 256, 0, s>>>(f + L.du4, f + L.y4, f + L.dy4, 1024 * cc, dh);
        tr_wgrad<32, 16, 4, TR_IN_PLAIN>(f + L.g4, f + L.dy4, f + L.part, G + P_W4, 64 * cc, s);
        tr_conv<16, 32, 4, TR_IN_PLAIN, true>(f + L.dy4, P + P_W4, nullptr, f + L.dg4, 64 * cc, lin, s);
        k_tr_actgrad<<<tr_blocks(2048 * cc), 256, 0, s>>>(f + L.dg4, f + L.dg4, f + L.g4, 2048 * cc, dh);
        tr_gemm(f + L.h3, 1, 200, f + L.dg4, 2048, 1, G + P_WD4, 2048, 201, 2048, cc, nullptr, lin, 2, 1, s);
        tr_gemm(f + L.dg4, 2048, 1, P + P_WD4, 1, 2048, f + L.dh3, 200, cc, 200, 2048, nullptr, lin, 1, 0, s);
        k_tr_actgrad<<<tr_blocks(200 * cc), 256, 0, s>>>(f + L.dh3, f + L.dh3, f + L.h3, 200 * cc, dh);
        tr_gemm(f + L.code, 1, 20, f + L.dh3, 200, 1, G + P_WD3, 200, 21, 200, cc, nullptr, lin, 2, 1, s);
        tr_gemm(f + L.dh3, 200, 1, P + P_WD3, 1, 200, f + L.dcode, 20, cc, 20, 200, nullptr, lin, 1, 0, s);
        // ---- the encoder ------------------------------------------------------------------------------------------------------------
        k_tr_actgrad<<<tr_blocks(20 * cc), 256, 0, s>>>(f + L.dcodep, f + L.dcode, f + L.code, 20 * cc, ec);
        tr_gemm(f + L.h1, 1, 200, f + L.dcodep, 20, 1, G + P_WD2, 20, 201, 20, cc, nullptr, lin, 2, 1, s);
        tr_gemm(f + L.dcodep, 20, 1, P + P_WD2, 1, 20, f + L.dh1, 200, cc, 200, 20, nullptr, lin, 1, 0, s);
        k_tr_actgrad<<<tr_blocks(200 * cc), 256, 0, s>>>(f + L.dh1, f + L.dh1, f + L.h1, 200 * cc, eh);
        tr_gemm(f + L.f3, 1, 2048, f + L.dh1, 200, 1, G + P_WD1, 200, 2049, 200, cc, nullptr, lin, 2, 1, s);
        tr_gemm(f + L.dh1, 200, 1, P + P_WD1, 1, 200, f + L.df3, 2048, cc, 2048, 200, nullptr, lin, 1, 0, s);
        k_tr_actgrad<<<tr_blocks(2048 * cc), 256, 0, s>>>(f + L.df3, f + L.df3, f + L.f3, 2048 * cc, eh);
        tr_wgrad<16, 32, 4, TR_IN_PLAIN>(f + L.p2, f + L.df3, f + L.part, G + P_W3, 64 * cc, s);
        tr_conv<32, 16, 4, TR_IN_PLAIN, true>(f + L.df3, P + P_W3, nullptr, f + L.dp2, 64 * cc, lin, s);
        k_tr_unpool<16, 4><<<tr_blocks(1024 * cc), 256, 0, s>>>(f + L.a2, f + L.dp2, f + L.da2, 1024 * cc, eh);
        tr_wgrad<8, 16, 8, TR_IN_PLAIN>(f + L.p1, f + L.da2, f + L.part, G + P_W2, 512 * cc, s);
        tr_conv<16, 8, 8, TR_IN_PLAIN, true>(f + L.da2, P + P_W2, nullptr, f + L.dp1, 512 * cc, lin, s);
        k_tr_unpool<8, 8><<<tr_blocks(4096 * cc), 256, 0, s>>>(f + L.a1, f + L.dp1, f + L.da1, 4096 * cc, eh);
        tr_wgrad<1, 8, 16, TR_IN_BITS>(b, f + L.da1, f + L.part, G + P_W1, 4096 * cc, s);
        CAELO_LAUNCH_CHECK();
    }
    return CAELO_OK;
}

CAELO_API int caelo_adadelta_step(caelo_ctx *c, float *params, const float *grads, float *acc_g, float *acc_d, int64_t count, float lr, float rho,
                                  float eps, void *stream) {
    return tc_optimizer_step(__func__, c, count, params && grads && acc_g && acc_d, stream, [&](unsigned blocks, hipStream_t s) {
        k_tr_adadelta<<<blocks, 256, 0, s>>>(params, grads, acc_g, acc_d, count, lr, rho, eps);
    });
}
