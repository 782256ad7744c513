// train_common.h -- what train.hip and train_ring.hip share, each piece ONCE: both trainers promise that the same (n, chunk) gives the
// same bits, and that promise is the order of summation written down here.  Internal linkage throughout (static kernels: a host stub per file).
#pragma once
#include "caelo_internal.h"

#include <math.h>

// ---- a sum over K on the matrix pipe ---------------------------------------------------------------------------------------------
// Four exact fmaf chains over ascending k on v_mfma_f32_16x16x4_f32: k-step s goes to chain s & 3, the chains are joined as
// (0 + 1) + (2 + 3).  Shorter chains lose fewer bits, and the four are independent instructions for the matrix pipe.  An accumulator
// is a plain f32x4 c[4] in registers.  Macros, not functions: handing the array to a function or wrapping it in a struct moved the
// kernels' register allocation (k_rt_conv lost a wavefront of occupancy in one form), these leave every main loop as it was.
// CHAINS_ZERO is one unbraced for statement with its own index j_, CHAINS_STEP evaluates s twice: callers pass plain expressions.
#define CHAINS_ZERO(c) _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) (c)[j_] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}
#define CHAINS_STEP(c, s, a, b) ((c)[(s) & 3] = MFMA16((a), (b), (c)[(s) & 3]))
#define CHAINS_JOIN(c) (((c)[0] + (c)[1]) + ((c)[2] + (c)[3]))

// A conv's B operand into LDS, sB[K4][NP] (K = TAPS x CIN padded to 4, N = COUT padded to 16, zeros in the padding): the Keras kernel
// W [TAPS][CIN][COUT] as it stands, or (FLIP: the data gradient of a conv whose kernel is W [TAPS][COUT][CIN]) the taps flipped and
// the channel axes swapped, B[tap CIN + ci][co] = W[TAPS - 1 - tap][co][ci].  All 256 threads; the caller's barrier follows.
template <int TAPS, int CIN, int COUT, bool FLIP>
__device__ __forceinline__ void tc_stage_b(float *sB, const float *W, int tid) {
    constexpr int K = TAPS * CIN, K4 = (K + 3) / 4 * 4, NP = (COUT + 15) / 16 * 16;
    for (int i = tid; i < K4 * NP; i += 256) {
        const int k = i / NP, n = i - k * NP;
        float v = 0.0f;
        if (k < K && n < COUT) {
            const int tap = k / CIN, ci = k - tap * CIN;
            v = FLIP ? W[((TAPS - 1 - tap) * COUT + n) * CIN + ci] : W[k * COUT + n];
        }
        sB[i] = v;
    }
}

// ---- sums in double ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double tc_wave_sum(double s) {   // the 64 lanes' values in a fixed butterfly; every lane gets the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// *dst = the sum of the 256 threads' values: each wavefront's butterfly, then the four partials through LDS as ((0 + 1) + 2) + 3 (every thread calls it, once per kernel)
__device__ __forceinline__ void tc_block_sum(double v, double *dst) {
    __shared__ double s_part[4];
    v = tc_wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *dst = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// dst[i] += the sum over the slices of part[slice][i], in double, rounded once: one wavefront per element, lane l takes slices l, l + 64,
// ... in ascending order, the 64 lane sums meet in the butterfly -- an order fixed by nsl alone
static __global__ __launch_bounds__(256) void k_tc_wreduce(const float *__restrict__ part, int64_t nsl, int count, float *__restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count) return;   // (wavefront-uniform)
    double s = 0.0;
    for (int64_t sl = lane; sl < nsl; sl += 64) s += (double)part[sl * count + i];
    s = tc_wave_sum(s);
    if (lane == 0) dst[i] += (float)s;
}

static inline void tc_wreduce(const float *part, int64_t nsl, int count, float *dst, hipStream_t s) { k_tc_wreduce<<<(count + 3) / 4, 256, 0, s>>>(part, nsl, count, dst); }

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// a chunk's workspace handed out in floats: take(per) = the offset of the next per x c floats, each region rounded up to 64 floats
struct TcTake {
    int64_t c, o;
    int64_t operator()(int64_t per) { const int64_t at = o; o += (per * c + 63) / 64 * 64; return at; }
};

// (offset, count) of n tensors that follow each other in one flat buffer
static inline void tc_param_layout(const int64_t *counts, int n, int64_t (*out)[2]) {
    int64_t o = 0;
    for (int t = 0; t < n; ++t) {
        out[t][0] = o; out[t][1] = counts[t];
        o += counts[t];
    }
}

// An elementwise optimizer step over `count` floats: the checks of an entry point `who` (ptrs: none of its buffers is null), then
// launch(blocks of 256 threads, stream) with the update kernel, whose arithmetic is the entry point's own.
template <typename Launch>
static int tc_optimizer_step(const char *who, const caelo_ctx *c, int64_t count, bool ptrs, void *stream, Launch launch) {
    auto refuse = [who](const char *msg) -> int { caelo_set_error("%s: %s", who, msg); return CAELO_ERR_ARG; };   // CAELO_REQUIRE under the entry point's name
    if (!c) return refuse("null context");
    if (count < 0 || count >= ((int64_t)1 << 39)) return refuse("count out of range");
    if (count == 0) return CAELO_OK;
    if (!ptrs) return refuse("null argument");
    launch((unsigned)((count + 255) / 256), caelo_stream(stream));
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
