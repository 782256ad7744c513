// evaluate.hip -- key point repeatability of the reference's evaluation (EvaluationOnKeypts.py), device resident.
//
// Reference behaviour restated here (never its code):
//   GetPairDistances              EvaluationOnKeypts.py:68-81   NearestNeighbors(n_neighbors=1).fit(frame i).kneighbors(frame i+1)
//   ComputeDispersionOfKeypoints  EvaluationOnKeypts.py:83-94   the same with the fit set as its own query set (every distance is 0)
//   the histogram                 EvaluationOnKeypts.py:128-140 C_t = #(dist / D_t < 1), counts[t] = C_t - C_{t-1},
//                                                               counts[T] = #(dist / D_{T-1} >= 1)
// scikit-learn 0.24.2 answers these queries with its kd-tree (the fit sets hold more than 3 points: the host refuses smaller ones).
// The tree prunes with lower bounds that never exceed a point's own reduced distance, so the distance it returns is the minimum over
// all fit points of euclidean_rdist (d = 0; d += (x - y)^2 over x, y, z, every operation rounded on its own), then a correctly
// rounded sqrt.  That is what one thread computes here, in the same order, for one query point.
//
// Layout: one workgroup per (pair, tile of EV_TILE query points); the fit set goes through LDS in chunks of EV_CHUNK points (any
// K up to CAELO_KP_NN_MAX_K); each thread keeps its running minimum; the bins are counted with wave ballots, one atomic per wave
// and bin.
#include "caelo_internal.h"

#pragma clang fp contract(off)

#define EV_TILE 256
#define EV_CHUNK 1024

struct EvParams {
    double thr[CAELO_KP_NN_MAX_THRESHOLDS];
    int n_thr;
    int ld;
    int64_t n_frames;
};

__global__ void __launch_bounds__(EV_TILE) k_kp_nn_pairs(const double *__restrict__ pts, const int32_t *__restrict__ n_key,
                                                         const int32_t *__restrict__ pairs, double *__restrict__ dist_out,
                                                         unsigned long long *__restrict__ counts, EvParams prm) {
    __shared__ double sx[EV_CHUNK], sy[EV_CHUNK], sz[EV_CHUNK];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t f0 = pairs[2 * p], f1 = pairs[2 * p + 1];   // (fit frame, query frame)
    if (f0 < 0 || f1 < 0 || f0 >= prm.n_frames || f1 >= prm.n_frames) return;   // the host refuses these: never read out of bounds
    const int k0 = min(max(n_key[f0], 0), prm.ld), k1 = min(max(n_key[f1], 0), prm.ld);
    const int j = blockIdx.y * EV_TILE + tid;
    if (blockIdx.y * EV_TILE >= k1) return;   // (uniform over the workgroup)
    const double *fit = pts + (size_t)f0 * prm.ld * 3;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (j < k1) {
        const double *q = pts + ((size_t)f1 * prm.ld + j) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    double best = __builtin_inf();
    for (int base = 0; base < k0; base += EV_CHUNK) {
        const int m = min(EV_CHUNK, k0 - base);
        __syncthreads();
        for (int i = tid; i < m; i += EV_TILE) {
            const double *s = fit + (size_t)(base + i) * 3;
            sx[i] = s[0]; sy[i] = s[1]; sz[i] = s[2];
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < m; ++i) {   // all lanes read the same address: LDS broadcast
            const double dx = __dsub_rn(qx, sx[i]), dy = __dsub_rn(qy, sy[i]), dz = __dsub_rn(qz, sz[i]);
            const double d = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));   // (0 + dx^2 is dx^2)
            best = d < best ? d : best;
        }
    }
    const bool valid = j < k1;
    const double dist = __dsqrt_rn(best);
    if (valid && dist_out) dist_out[(size_t)p * prm.ld + j] = dist;
    // bins: per wave, C_t by ballot; lane 0 adds C_t - C_{t-1} (and the overflow bin) to the pair's row
    const int lane = tid & 63;
    unsigned long long *row = counts + (size_t)p * (prm.n_thr + 1);
    long long prev = 0;
    for (int t = 0; t < prm.n_thr; ++t) {
        const long long c = __popcll(__ballot(valid && __ddiv_rn(dist, prm.thr[t]) < 1.0));
        if (lane == 0 && c != prev) atomicAdd(row + t, (unsigned long long)(c - prev));   // (two's complement: a negative bin adds up too)
        prev = c;
    }
    const long long rest = __popcll(__ballot(valid)) - prev;   // dist / D_{T-1} >= 1: the complement (the distances are never NaN)
    if (lane == 0 && rest != 0) atomicAdd(row + prm.n_thr, (unsigned long long)rest);
}

CAELO_API int caelo_kp_nn_pairs(caelo_ctx *c, const double *pts, int64_t n_frames, int ld, const int32_t *n_key, const int32_t *pairs,
                                int64_t n_pairs, const double *thresholds, int n_thresholds, double *dist, int64_t *counts, void *stream) {
    CAELO_REQUIRE(c && n_key && pairs && thresholds && counts && (pts || n_frames == 0), "null argument");
    CAELO_REQUIRE(n_frames >= 0 && n_frames < (1LL << 31) && n_pairs >= 0 && n_pairs < (1LL << 31), "bad shape");
    CAELO_REQUIRE(ld >= 1 && ld <= CAELO_KP_NN_MAX_K, "ld must lie in [1, CAELO_KP_NN_MAX_K]");
    CAELO_REQUIRE(n_thresholds >= 1 && n_thresholds <= CAELO_KP_NN_MAX_THRESHOLDS, "1 to CAELO_KP_NN_MAX_THRESHOLDS thresholds");
    EvParams prm;
    for (int t = 0; t < CAELO_KP_NN_MAX_THRESHOLDS; ++t) prm.thr[t] = 1.0;
    for (int t = 0; t < n_thresholds; ++t) {
        CAELO_REQUIRE(thresholds[t] > 0.0 && thresholds[t] <= 1.7976931348623157e308, "thresholds must be finite and positive");
        prm.thr[t] = thresholds[t];
    }
    prm.n_thr = n_thresholds;
    prm.ld = ld;
    prm.n_frames = n_frames;
    hipStream_t s = caelo_stream(stream);
    CAELO_HIP(hipMemsetAsync(counts, 0, (size_t)n_pairs * (n_thresholds + 1) * sizeof(int64_t), s));
    if (n_pairs == 0) return CAELO_OK;
    const dim3 grid((unsigned)n_pairs, (unsigned)((ld + EV_TILE - 1) / EV_TILE));
    k_kp_nn_pairs<<<grid, EV_TILE, 0, s>>>(pts, n_key, pairs, dist, (unsigned long long *)counts, prm);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
