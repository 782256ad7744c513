// train_ring.hip -- loss and gradient of the spherical-ring autoencoder (AE4SphericalRingPC.py:129-144) and Keras 2.2.4's Adam step.
//   Input [n][h][w][3]  conv2d_1 3x3 3->32 relu  conv2d_2 1x1 32->8 relu (the response layer)  MaxPooling2D(2)  conv2d_3 3x3 8->16 relu
//   MaxPooling2D(2)  conv2d_4 3x3 16->16 relu  UpSampling2D(2)  conv2d_5 3x3 16->8 relu  UpSampling2D(2)  conv2d_6 1x1 8->3 linear
// trained against its own input with mean_squared_error, on plain Keras-layout f32 weights in ONE flat buffer of 5 835 floats (12
// tensors, caelo_ring_train_param_layout); the gradient and Adam's m and v have the same layout.  A layer's kernel [kh][kw][Cin][Cout]
// is followed by its bias [Cout], so the two are one row-major [taps Cin + 1][Cout] matrix: every weight-gradient GEMM carries a row
// of ones behind its A operand and the bias gradient is its last row (train.hip's arrangement).
//
// Arithmetic as in train.hip: four MFMA chains per sum over K, no floating-point atomics, one owner and one order of summation per output
// element.  CHAINS_*, tc_stage_b, k_tc_wreduce, tc_wave_sum, tc_block_sum, the layout helpers and the optimizer launcher: train_common.h.
//   k_rt_conv    forward convs and data gradients as implicit GEMMs.  A workgroup owns a tile of 4 rows x 64 columns of one image and
//                stages the (4 + 2) x (64 + 2) x Cin input tile with its halo (zeros outside the image) and the layer's B operand in LDS
//                once; a wavefront takes one row: four m-tiles of 16 consecutive pixels (columns >= w are computed on zeros and not
//                stored), N = Cout padded to 16, K = taps x Cin over ascending (tap, channel), 27 padded to 28.  The data gradient is
//                the same kernel with the taps flipped and the channel axes swapped while B is staged.  The input is read through
//                strides (the caller's images in place) and optionally through UpSampling2D(2) (pixel u reads source pixel u >> 1).
//   k_rt_wgrad   a layer's weight gradient: M = taps Cin + 1, N = Cout, K = pixels.  A workgroup stages the same input tile and the
//                tile's 256 delta rows in LDS, walks up to eight tiles with its sums in registers and writes one slice of partial sums
//                per K part; k_tc_wreduce adds a chunk's slices in a fixed order in double (one wavefront per element) and then adds
//                that to the gradient.
//   pooling      the gradient of a window goes to its FIRST maximum in ascending (dy, dx) order, dx fastest (k_rt_unpool);
//                UpSampling2D's adjoint sums the four children in that order, times the source layer's relu' (k_rt_upsum).
//   loss         (r - x)^2 in double: 4096 elements per workgroup in a fixed tree (k_rt_loss), an image's workgroups in a fixed butterfly,
//                images in ascending order, rounded once (k_rt_loss_acc) -- the loss bits depend on (n, h, w) alone, not on the chunk.
// A1 (32 channels at full resolution) is STORED by the forward pass, not recomputed: recomputing it is the network's largest layer
// again (46 % of a forward pass) while storing it costs one write and two reads of 128 bytes per pixel.
#include "train_common.h"

#define RT_TR 4            // rows of a workgroup's tile: one per wavefront
#define RT_TC 64           // its columns: four m-tiles
#define RT_LOSS_ELEMS 4096 // elements of one image a loss workgroup sums
#define RT_MAX_CHUNK 4096
#define RT_MAX_PIXELS ((int64_t)1 << 24)

// the 12 tensors, in floats: conv2d_1 .. conv2d_6, kernel then bias
static const int64_t RT_COUNT[12] = {864, 32, 256, 8, 1152, 16, 2304, 16, 1152, 8, 24, 3};
enum {
    Q_W1 = 0, Q_B1 = 864, Q_W2 = 896, Q_B2 = 1152, Q_W3 = 1160, Q_B3 = 2312, Q_W4 = 2328, Q_B4 = 4632, Q_W5 = 4648, Q_B5 = 5800, Q_W6 = 5808,
    Q_B6 = 5832, Q_TOTAL = 5835
};

// a [n][rows][cols][channels] f32 tensor read through strides (in floats): element (i, y, x, c) is p[i is + y rs + x ps + c]
struct RtIn {
    const float *p;
    int64_t is, rs, ps;
};

static RtIn rt_plain(const float *p, int h, int w, int c) { return RtIn{p, (int64_t)h * w * c, (int64_t)w * c, (int64_t)c}; }

// one chunk's workspace, offsets in floats behind the doubles of the loss
struct RtLayout {
    int64_t a1, a2, p1, a3, p2, y4, y5, r;                         // saved activations
    int64_t dr, du5, dy5, du4, dy4, dp2, da3, dp1, da2, da1, part; // their gradients, slice partials
    int64_t total, base_bytes, loss_blocks;                        // loss_blocks: workgroups of k_rt_loss per image
};

static inline int64_t rt_tiles(int h, int w) { return (int64_t)((h + RT_TR - 1) / RT_TR) * ((w + RT_TC - 1) / RT_TC); }

static RtLayout rt_layout(int h, int w, int64_t c) {
    RtLayout L;
    const int64_t px = (int64_t)h * w, px2 = px / 4, px4 = px / 16;
    TcTake take{c, 0};
    L.a1 = take(32 * px); L.a2 = take(8 * px); L.p1 = take(8 * px2); L.a3 = take(16 * px2); L.p2 = take(16 * px4); L.y4 = take(16 * px4);
    L.y5 = take(8 * px2); L.r = take(3 * px);
    L.dr = take(3 * px); L.du5 = take(8 * px); L.dy5 = take(8 * px2); L.du4 = take(16 * px2); L.dy4 = take(16 * px4); L.dp2 = take(16 * px4);
    L.da3 = take(16 * px2); L.dp1 = take(8 * px2); L.da2 = take(8 * px); L.da1 = take(32 * px);
    // slice partials, the largest of the six weight gradients: conv2d_1 writes two K parts of 28 x 32 floats per full-resolution tile,
    // conv2d_3 73 x 16 per half-resolution tile, conv2d_4 145 x 16 per quarter-resolution tile (rt_wgrad)
    int64_t part = 2 * 896 * rt_tiles(h, w);
    if (1168 * rt_tiles(h / 2, w / 2) > part) part = 1168 * rt_tiles(h / 2, w / 2);
    if (2320 * rt_tiles(h / 4, w / 4) > part) part = 2320 * rt_tiles(h / 4, w / 4);
    L.part = take.o;
    L.total = take.o + part * c;
    L.loss_blocks = (3 * px + RT_LOSS_ELEMS - 1) / RT_LOSS_ELEMS;
    L.base_bytes = ((1 + L.loss_blocks * c) * 8 + 255) / 256 * 256;
    return L;
}

__device__ __forceinline__ float rt_act(float x, int act) { return act == CAELO_ACT_RELU ? (x > 0.0f ? x : 0.0f) : x; }

// ------------------------------------------------------------------------------------------------
// The input tile of a workgroup with its halo, zeros outside the image: sA[(py AW + px) PS + c], PS = CIN | 1 (an odd pixel stride keeps
// the 16 pixels x 4 channels of an A fetch on distinct LDS banks for CIN = 16 and 32).
template <int CIN, int KS, int UP>
__device__ __forceinline__ void rt_stage_tile(float *sA, const RtIn in, int img, int y0, int x0, int H, int Wd, int tid) {
    constexpr int HL = KS / 2, PS = CIN | 1, AW = RT_TC + 2 * HL, AH = RT_TR + 2 * HL;
    for (int i = tid; i < AH * AW * CIN; i += 256) {
        const int c = i % CIN, px = (i / CIN) % AW, py = i / (CIN * AW);
        const int y = y0 + py - HL, x = x0 + px - HL;
        float v = 0.0f;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)Wd) v = in.p[(int64_t)img * in.is + (int64_t)(y >> UP) * in.rs + (int64_t)(x >> UP) * in.ps + c];
        sA[(py * AW + px) * PS + c] = v;
    }
}

// out[img][y][x][co] = act(sum_{tap, ci} in[img][y + dy - HL][x + dx - HL][ci] B[tap CIN + ci][co] + bias[co]), H x Wd pixels per image.
// B = the Keras kernel W [taps][CIN][COUT] as it stands, or (FLIP: the data gradient of a conv whose kernel is W [taps][COUT][CIN])
// B[tap CIN + ci][co] = W[taps - 1 - tap][co][ci].  gate (optional, out's shape): the result is kept where gate > 0 and 0 elsewhere
// (the relu' of the layer whose output gate is).  One workgroup per (image, tile).
template <int CIN, int COUT, int KS, int UP, bool FLIP>
__global__ __launch_bounds__(256) void k_rt_conv(const RtIn in, const float *__restrict__ W, const float *__restrict__ bias, float *__restrict__ out,
                                                 const float *__restrict__ gate, int H, int Wd, int tiles_x, int tiles_y, int act) {
    constexpr int K = KS * KS * CIN, K4 = (K + 3) / 4 * 4, NP = (COUT + 15) / 16 * 16, NT = NP / 16;
    constexpr int HL = KS / 2, PS = CIN | 1, AW = RT_TC + 2 * HL;
    extern __shared__ float smem[];
    float *sB = smem, *sA = smem + K4 * NP;   // [K4][NP], the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, img = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = tx * RT_TC, y0 = ty * RT_TR;
    tc_stage_b<KS * KS, CIN, COUT, FLIP>(sB, W, tid);
    rt_stage_tile<CIN, KS, UP>(sA, in, img, y0, x0, H, Wd, tid);
    __syncthreads();
    const int y = y0 + wave;
    if (y >= H) return;   // (wavefront-uniform, behind the only barrier)
    for (int mt = 0; mt < RT_TC / 16; ++mt) {
        const int xb = x0 + mt * 16;
        if (xb >= Wd) break;
        f32x4 acc[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) CHAINS_ZERO(acc[nt]);
#pragma unroll
        for (int ks = 0; ks < K4 / 4; ++ks) {
            const int k = ks * 4 + kq, tap = k / CIN, ci = k - tap * CIN;
            const int dy = tap / KS, dx = tap - dy * KS;
            const float a = (K4 == K || k < K) ? sA[((wave + dy) * AW + mt * 16 + r + dx) * PS + ci] : 0.0f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) CHAINS_STEP(acc[nt], ks, a, sB[k * NP + nt * 16 + r]);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 16 + r;
            if (col < COUT) {
                const float b = bias ? bias[col] : 0.0f;
                const f32x4 sum = CHAINS_JOIN(acc[nt]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = xb + 4 * kq + i;
                    if (x < Wd) {
                        const int64_t at = (((int64_t)img * H + y) * Wd + x) * COUT + col;
                        float v = rt_act(sum[i] + b, act);
                        if (gate) v = gate[at] > 0.0f ? v : 0.0f;
                        out[at] = v;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// part[slice][m][co] = sum over the slice's pixels of A[m][pixel] delta[pixel][co], m = tap CIN + ci: A = in[pixel + tap - HL][ci], and
// A = 1 for m = taps CIN (the bias).  A workgroup walks `group` consecutive tiles (256 pixels each in (row, column) order, pixels outside
// the image carry a zero delta), staging one at a time, and keeps its sums in registers across them; its wavefronts share the (m-tile,
// K part) jobs, KSPLIT K parts of 256 / KSPLIT pixels per tile where there are fewer than four m-tiles; slice = workgroup x KSPLIT + K part.
template <int CIN, int COUT, int KS, int UP>
__global__ __launch_bounds__(256) void k_rt_wgrad(const RtIn in, const float *__restrict__ delta, float *__restrict__ part, int H, int Wd, int tiles_x,
                                                  int tiles_y, int tiles, int group) {
    constexpr int T = KS * KS, M = T * CIN, M1 = M + 1, MT = (M1 + 15) / 16, NP = (COUT + 15) / 16 * 16, NT = NP / 16;
    constexpr int HL = KS / 2, PS = CIN | 1, AW = RT_TC + 2 * HL, AH = RT_TR + 2 * HL, KSPLIT = MT >= 4 ? 1 : 4 / MT;
    constexpr int STEPS = RT_TR * RT_TC / 4 / KSPLIT, JOBS = (MT * KSPLIT + 3) / 4;
    extern __shared__ float smem[];
    float *sA = smem, *sD = smem + AH * AW * PS;   // the tile, [256][NP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    f32x4 acc[JOBS][NT][4];
#pragma unroll
    for (int j = 0; j < JOBS; ++j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) CHAINS_ZERO(acc[j][nt]);
    for (int g = 0; g < group; ++g) {
        const int t = blockIdx.x * group + g;
        if (t >= tiles) break;   // (workgroup-uniform)
        const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, img = t / (tiles_x * tiles_y);
        const int x0 = tx * RT_TC, y0 = ty * RT_TR;
        rt_stage_tile<CIN, KS, UP>(sA, in, img, y0, x0, H, Wd, tid);
        for (int i = tid; i < RT_TR * RT_TC * NP; i += 256) {
            const int col = i % NP, pix = i / NP;
            const int y = y0 + pix / RT_TC, x = x0 + pix % RT_TC;
            sD[i] = (y < H && x < Wd && col < COUT) ? delta[(((int64_t)img * H + y) * Wd + x) * COUT + col] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < JOBS; ++j) {
            const int job = wave + 4 * j;
            if (job < MT * KSPLIT) {   // (wavefront-uniform)
                const int mt = job % MT, kp = job / MT;
                const int m = mt * 16 + r, tap = m / CIN, ci = m - tap * CIN;
                const int dy = tap / KS, dx = tap - dy * KS;
                const int base = m < M ? (dy * AW + dx) * PS + ci : 0;
#pragma unroll 8
                for (int ks = 0; ks < STEPS; ++ks) {
                    const int pix = (kp * STEPS + ks) * 4 + kq;
                    const float v = sA[base + ((pix / RT_TC) * AW + pix % RT_TC) * PS];
                    const float a = m < M ? v : (m == M ? 1.0f : 0.0f);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) CHAINS_STEP(acc[j][nt], ks, a, sD[pix * NP + nt * 16 + r]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < JOBS; ++j) {
        const int job = wave + 4 * j;
        if (job >= MT * KSPLIT) continue;
        const int mt = job % MT, kp = job / MT;
        const int64_t slice = (int64_t)blockIdx.x * KSPLIT + kp;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 16 + r;
            const f32x4 sum = CHAINS_JOIN(acc[j][nt]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mrow = mt * 16 + 4 * kq + i;
                if (mrow < M1 && col < COUT) part[(slice * M1 + mrow) * COUT + col] = sum[i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// MaxPooling2D(2): A [p][2 HS][2 WS][C] -> P [p][HS][WS][C]; `total` = the elements of P
#define RT_CELL(i)                                                                                           \
    const int ch = (int)((i) % C);                                                                           \
    const int x = (int)(((i) / C) % WS), y = (int)(((i) / ((int64_t)C * WS)) % HS);                          \
    const int64_t p = (i) / ((int64_t)C * WS * HS);                                                          \
    int64_t at[4];                                                                                           \
    _Pragma("unroll") for (int o = 0; o < 4; ++o) at[o] = (((p * 2 * HS + 2 * y + (o >> 1)) * 2 * WS) + 2 * x + (o & 1)) * C + ch;

template <int C>
__global__ __launch_bounds__(256) void k_rt_pool(const float *__restrict__ A, float *__restrict__ P, int HS, int WS, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    RT_CELL(i)
    float best = A[at[0]];
#pragma unroll
    for (int o = 1; o < 4; ++o) {
        const float v = A[at[o]];
        if (v > best) best = v;
    }
    P[i] = best;
}

// its gradient behind relu: dA = (A > 0) dP at the window's first maximum in ascending (dy, dx) order, 0 at the other three cells
template <int C>
__global__ __launch_bounds__(256) void k_rt_unpool(const float *__restrict__ A, const float *__restrict__ dP, float *__restrict__ dA, int HS, int WS,
                                                   int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    RT_CELL(i)
    float best = A[at[0]];
    int arg = 0;
#pragma unroll
    for (int o = 1; o < 4; ++o) {
        const float v = A[at[o]];
        if (v > best) { best = v; arg = o; }
    }
    const float g = best > 0.0f ? dP[i] : 0.0f;
#pragma unroll
    for (int o = 0; o < 4; ++o) dA[at[o]] = o == arg ? g : 0.0f;
}

// UpSampling2D(2)'s adjoint behind relu: dY [p][HS][WS][C] = (Y > 0) x the sum of dU over the four children in ascending (dy, dx) order
template <int C>
__global__ __launch_bounds__(256) void k_rt_upsum(const float *__restrict__ dU, const float *__restrict__ Y, float *__restrict__ dY, int HS, int WS,
                                                  int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    RT_CELL(i)
    float s = dU[at[0]];
#pragma unroll
    for (int o = 1; o < 4; ++o) s += dU[at[o]];
    dY[i] = Y[i] > 0.0f ? s : 0.0f;
}

// ------------------------------------------------------------------------------------------------
// workgroup b of image i: elements e = b 4096 + j 256 + tid (e = pixel x 3 + channel) of (r - x)^2, d = r - x rounded in f32, squared and
// summed in double (thread: ascending j, then tc_block_sum); dr = d scale
__global__ __launch_bounds__(256) void k_rt_loss(const float *__restrict__ rec, const RtIn in, float *__restrict__ dr, double *__restrict__ block_sums, int Wd,
                                                 int64_t per_img, int loss_blocks, float scale) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x % loss_blocks, img = blockIdx.x / loss_blocks;
    double lsum = 0.0;
#pragma unroll 4
    for (int j = 0; j < RT_LOSS_ELEMS / 256; ++j) {
        const int64_t e = (int64_t)b * RT_LOSS_ELEMS + j * 256 + tid;
        if (e < per_img) {
            const int64_t pix = e / 3;
            const int c = (int)(e - pix * 3), y = (int)(pix / Wd), x = (int)(pix - (int64_t)y * Wd);
            const float d = rec[(int64_t)img * per_img + e] - in.p[(int64_t)img * in.is + (int64_t)y * in.rs + (int64_t)x * in.ps + c];
            lsum += (double)d * (double)d;
            if (dr) dr[(int64_t)img * per_img + e] = d * scale;
        }
    }
    tc_block_sum(lsum, block_sums + blockIdx.x);
}

// one wavefront: each image's workgroup sums meet in a fixed order (lane l takes l, l + 64, ..., then the butterfly), the images are added
// to the running sum in ascending order; the last chunk rounds the mean once
__global__ __launch_bounds__(64) void k_rt_loss_acc(const double *__restrict__ block_sums, int c, int loss_blocks, double *__restrict__ acc, int first, int last,
                                                    double count, float *__restrict__ loss) {
    const int lane = threadIdx.x;
    double a = first ? 0.0 : *acc;
    for (int i = 0; i < c; ++i) {
        double s = 0.0;
        for (int b = lane; b < loss_blocks; b += 64) s += block_sums[(int64_t)i * loss_blocks + b];
        a += tc_wave_sum(s);
    }
    if (lane == 0) {
        *acc = a;
        if (last) *loss = (float)(a / count);
    }
}

// ------------------------------------------------------------------------------------------------
// Keras 2.2.4 Adam (optimizers.py: m_t = beta_1 m + (1. - beta_1) g; v_t = beta_2 v + (1. - beta_2) K.square(g);
// p_t = p - lr_t * m_t / (K.sqrt(v_t) + epsilon)), every operation rounded on its own in f32 (the file is built with -ffp-contract=off),
// in Python's order: (lr_t m_t) / (sqrt(v_t) + eps).  The square root and the quotient go through f64, whose 53 bits >= 2 x 24 + 2 make
// the value rounded back to f32 the correctly rounded f32 result (k_tr_adadelta's argument).
__global__ __launch_bounds__(256) void k_rt_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int64_t count,
                                                 float lr_t, float beta1, float beta2, float eps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float one_b1 = 1.0f - beta1, one_b2 = 1.0f - beta2;
    const float gi = g[i];
    const float g2 = gi * gi;
    const float mg = one_b1 * gi, vg = one_b2 * g2;
    const float bm = beta1 * m[i], bv = beta2 * v[i];
    const float mt = bm + mg, vt = bv + vg;
    const float num = lr_t * mt;
    const float den = (float)sqrt((double)vt) + eps;
    const float u = (float)((double)num / (double)den);
    m[i] = mt;
    v[i] = vt;
    p[i] = p[i] - u;
}

// ================================================================================================
CAELO_API int caelo_ring_train_param_layout(int64_t out[12][2]) {
    CAELO_REQUIRE(out != nullptr, "null argument");
    tc_param_layout(RT_COUNT, 12, out);
    return CAELO_OK;
}

static bool rt_shape_ok(int h, int w, int64_t chunk) {
    return h > 0 && w > 0 && h % 4 == 0 && w % 4 == 0 && (int64_t)h * w <= RT_MAX_PIXELS && chunk >= 1 && chunk <= RT_MAX_CHUNK;
}

CAELO_API int64_t caelo_ring_train_ws_bytes(int h, int w, int64_t chunk) {
    if (!rt_shape_ok(h, w, chunk)) return 0;
    const RtLayout L = rt_layout(h, w, chunk);
    return L.base_bytes + L.total * (int64_t)sizeof(float);
}

CAELO_API int caelo_ring_train_ws_layout(int h, int w, int64_t chunk, int64_t out[4]) {
    CAELO_REQUIRE(out && rt_shape_ok(h, w, chunk), "null argument, h or w not a positive multiple of 4, or chunk outside [1, 4096]");
    const RtLayout L = rt_layout(h, w, chunk);
    out[0] = L.base_bytes + L.a2 * 4;    // A2 [chunk][h][w][8]
    out[1] = L.base_bytes + L.r * 4;     // r [chunk][h][w][3]
    out[2] = L.base_bytes + L.dp1 * 4;   // dL/dP1 [chunk][h/2][w/2][8]
    out[3] = L.base_bytes + L.dr * 4;    // dL/dr [chunk][h][w][3]
    return CAELO_OK;
}

template <int CIN, int COUT, int KS, int UP, bool FLIP>
static void rt_conv(const RtIn in, const float *W, const float *bias, float *out, const float *gate, int imgs, int h, int w, int act, hipStream_t s) {
    constexpr int K4 = (KS * KS * CIN + 3) / 4 * 4, NP = (COUT + 15) / 16 * 16, HL = KS / 2;
    constexpr size_t lds = (K4 * NP + (RT_TR + 2 * HL) * (RT_TC + 2 * HL) * (CIN | 1)) * sizeof(float);
    static_assert(lds <= 65536, "the tile and the B operand must fit the default LDS allotment");
    const int tx = (w + RT_TC - 1) / RT_TC, ty = (h + RT_TR - 1) / RT_TR;
    k_rt_conv<CIN, COUT, KS, UP, FLIP><<<(unsigned)((int64_t)imgs * tx * ty), 256, lds, s>>>(in, W, bias, out, gate, h, w, tx, ty, act);
}

template <int CIN, int COUT, int KS, int UP>
static void rt_wgrad(const RtIn in, const float *delta, float *part, float *dst, int imgs, int h, int w, hipStream_t s) {
    constexpr int M1 = KS * KS * CIN + 1, MT = (M1 + 15) / 16, NP = (COUT + 15) / 16 * 16, HL = KS / 2, KSPLIT = MT >= 4 ? 1 : 4 / MT;
    constexpr size_t lds = ((RT_TR + 2 * HL) * (RT_TC + 2 * HL) * (CIN | 1) + RT_TR * RT_TC * NP) * sizeof(float);
    static_assert(lds <= 65536, "the tile and its delta rows must fit the default LDS allotment");
    const int tx = (w + RT_TC - 1) / RT_TC, ty = (h + RT_TR - 1) / RT_TR, count = M1 * COUT;
    const int tiles = (int)((int64_t)imgs * tx * ty);
    // tiles per workgroup: fewer, longer slices where there are tiles to spare -- a function of (images, h, w) alone, like the order of
    // summation it fixes
    const int group = tiles / 1024 < 1 ? 1 : (tiles / 1024 > 8 ? 8 : tiles / 1024);
    const int wgs = (tiles + group - 1) / group;
    k_rt_wgrad<CIN, COUT, KS, UP><<<(unsigned)wgs, 256, lds, s>>>(in, delta, part, h, w, tx, ty, tiles, group);
    tc_wreduce(part, (int64_t)wgs * KSPLIT, count, dst, s);
}

static inline unsigned rt_blocks(int64_t total) { return (unsigned)((total + 255) / 256); }

CAELO_API int caelo_ring_autoencoder_grad(caelo_ctx *c, const float *params, const float *images, int64_t n, int h, int w, int64_t img_stride,
                                          int64_t row_stride, int64_t pix_stride, int64_t chunk, float *grads, float *loss, float *recon, void *ws,
                                          void *stream) {
    CAELO_REQUIRE(c != nullptr, "null context");
    CAELO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "image count out of range");
    CAELO_REQUIRE(h > 0 && w > 0 && h % 4 == 0 && w % 4 == 0,
                  "h and w must be positive multiples of 4: Keras pads the 'same' poolings of other sizes, and that path is not built");
    CAELO_REQUIRE((int64_t)h * w <= RT_MAX_PIXELS, "images of more than 2^24 pixels");
    CAELO_REQUIRE(pix_stride >= 3 && row_stride >= (int64_t)w * pix_stride && img_stride >= (int64_t)h * row_stride,
                  "strides that make pixels overlap (pix_stride < 3, row_stride < w pix_stride or img_stride < h row_stride)");
    CAELO_REQUIRE(chunk >= 1 && chunk <= RT_MAX_CHUNK, "chunk outside [1, 4096]");
    CAELO_REQUIRE(params && loss && ws && (images || n == 0), "null params, loss, workspace or images");
    hipStream_t s = caelo_stream(stream);
    if (grads) CAELO_HIP(hipMemsetAsync(grads, 0, Q_TOTAL * sizeof(float), s));
    if (n == 0) {
        CAELO_HIP(hipMemsetAsync(loss, 0, sizeof(float), s));
        return CAELO_OK;
    }
    const RtLayout L = rt_layout(h, w, chunk);
    double *lacc = (double *)ws, *bsum = lacc + 1;
    float *f = (float *)((char *)ws + L.base_bytes);
    const float *P = params;
    float *G = grads;
    const int h2 = h / 2, w2 = w / 2, h4 = h / 4, w4 = w / 4;
    const int64_t px = (int64_t)h * w, px2 = px / 4, px4 = px / 16;
    const double count = 3.0 * (double)px * (double)n;
    const float scale = (float)(2.0 / count);
    const int relu = CAELO_ACT_RELU, lin = CAELO_ACT_LINEAR;

    for (int64_t start = 0; start < n; start += chunk) {
        const int cc = (int)(n - start < chunk ? n - start : chunk);
        const RtIn X = RtIn{images + start * img_stride, img_stride, row_stride, pix_stride};
        // ---- forward ------------------------------------------------------------------------------------------------------------
        rt_conv<3, 32, 3, 0, false>(X, P + Q_W1, P + Q_B1, f + L.a1, nullptr, cc, h, w, relu, s);
        rt_conv<32, 8, 1, 0, false>(rt_plain(f + L.a1, h, w, 32), P + Q_W2, P + Q_B2, f + L.a2, nullptr, cc, h, w, relu, s);
        k_rt_pool<8><<<rt_blocks(8 * px2 * cc), 256, 0, s>>>(f + L.a2, f + L.p1, h2, w2, 8 * px2 * cc);
        rt_conv<8, 16, 3, 0, false>(rt_plain(f + L.p1, h2, w2, 8), P + Q_W3, P + Q_B3, f + L.a3, nullptr, cc, h2, w2, relu, s);
        k_rt_pool<16><<<rt_blocks(16 * px4 * cc), 256, 0, s>>>(f + L.a3, f + L.p2, h4, w4, 16 * px4 * cc);
        rt_conv<16, 16, 3, 0, false>(rt_plain(f + L.p2, h4, w4, 16), P + Q_W4, P + Q_B4, f + L.y4, nullptr, cc, h4, w4, relu, s);
        rt_conv<16, 8, 3, 1, false>(rt_plain(f + L.y4, h4, w4, 16), P + Q_W5, P + Q_B5, f + L.y5, nullptr, cc, h2, w2, relu, s);
        rt_conv<8, 3, 1, 1, false>(rt_plain(f + L.y5, h2, w2, 8), P + Q_W6, P + Q_B6, f + L.r, nullptr, cc, h, w, lin, s);
        k_rt_loss<<<(unsigned)(L.loss_blocks * cc), 256, 0, s>>>(f + L.r, X, G ? f + L.dr : nullptr, bsum, w, 3 * px, (int)L.loss_blocks, scale);
        k_rt_loss_acc<<<1, 64, 0, s>>>(bsum, cc, (int)L.loss_blocks, lacc, start == 0, start + chunk >= n, count, loss);
        CAELO_LAUNCH_CHECK();
        if (recon) CAELO_HIP(hipMemcpyAsync(recon + start * 3 * px, f + L.r, (size_t)cc * 3 * px * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (!G) continue;
        // ---- backward -----------------------------------------------------------------------------------------------------------
        rt_wgrad<8, 3, 1, 1>(rt_plain(f + L.y5, h2, w2, 8), f + L.dr, f + L.part, G + Q_W6, cc, h, w, s);
        rt_conv<3, 8, 1, 0, true>(rt_plain(f + L.dr, h, w, 3), P + Q_W6, nullptr, f + L.du5, nullptr, cc, h, w, lin, s);
        k_rt_upsum<8><<<rt_blocks(8 * px2 * cc), 256, 0, s>>>(f + L.du5, f + L.y5, f + L.dy5, h2, w2, 8 * px2 * cc);
        rt_wgrad<16, 8, 3, 1>(rt_plain(f + L.y4, h4, w4, 16), f + L.dy5, f + L.part, G + Q_W5, cc, h2, w2, s);
        rt_conv<8, 16, 3, 0, true>(rt_plain(f + L.dy5, h2, w2, 8), P + Q_W5, nullptr, f + L.du4, nullptr, cc, h2, w2, lin, s);
        k_rt_upsum<16><<<rt_blocks(16 * px4 * cc), 256, 0, s>>>(f + L.du4, f + L.y4, f + L.dy4, h4, w4, 16 * px4 * cc);
        rt_wgrad<16, 16, 3, 0>(rt_plain(f + L.p2, h4, w4, 16), f + L.dy4, f + L.part, G + Q_W4, cc, h4, w4, s);
        rt_conv<16, 16, 3, 0, true>(rt_plain(f + L.dy4, h4, w4, 16), P + Q_W4, nullptr, f + L.dp2, nullptr, cc, h4, w4, lin, s);
        k_rt_unpool<16><<<rt_blocks(16 * px4 * cc), 256, 0, s>>>(f + L.a3, f + L.dp2, f + L.da3, h4, w4, 16 * px4 * cc);
        rt_wgrad<8, 16, 3, 0>(rt_plain(f + L.p1, h2, w2, 8), f + L.da3, f + L.part, G + Q_W3, cc, h2, w2, s);
        rt_conv<16, 8, 3, 0, true>(rt_plain(f + L.da3, h2, w2, 16), P + Q_W3, nullptr, f + L.dp1, nullptr, cc, h2, w2, lin, s);
        k_rt_unpool<8><<<rt_blocks(8 * px2 * cc), 256, 0, s>>>(f + L.a2, f + L.dp1, f + L.da2, h2, w2, 8 * px2 * cc);
        rt_wgrad<32, 8, 1, 0>(rt_plain(f + L.a1, h, w, 32), f + L.da2, f + L.part, G + Q_W2, cc, h, w, s);
        rt_conv<8, 32, 1, 0, true>(rt_plain(f + L.da2, h, w, 8), P + Q_W2, nullptr, f + L.da1, f + L.a1, cc, h, w, lin, s);
        rt_wgrad<3, 32, 3, 0>(X, f + L.da1, f + L.part, G + Q_W1, cc, h, w, s);
        CAELO_LAUNCH_CHECK();
    }
    return CAELO_OK;
}

CAELO_API int caelo_adam_step(caelo_ctx *c, float *params, const float *grads, float *m, float *v, int64_t count, float lr_t, float beta1, float beta2,
                              float eps, void *stream) {
    return tc_optimizer_step(__func__, c, count, params && grads && m && v, stream, [&](unsigned blocks, hipStream_t s) {
        k_rt_adam<<<blocks, 256, 0, s>>>(params, grads, m, v, count, lr_t, beta1, beta2, eps);
    });
}
