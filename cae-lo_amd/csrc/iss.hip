// iss.hip -- ISS (intrinsic shape signatures) key points on the device: the hand-crafted detector of the reference's key point
// comparison (PclKeyPts.py:41-46, :92-103: PCLKeypoint.keypointIss, a PCL binding the reference does not ship).
//
// The model is PCL 1.8's ISSKeypoint3D with border estimation off; the definition itself is DESIGN.md 9h and is restated here:
//   neighbours      j is a neighbour of i at radius r  <=>  d2 < r * r (strict; r * r one rounded product; i is its own neighbour),
//                   d = double(P[j]) - double(P[i]),  d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded on its own
//   scatter matrix  fewer than min_neighbors neighbours at salient_radius: saliency -1, eigenvalues 0.  Otherwise
//                   C_ab = sum_j d_a * d_b over the neighbours in ascending j (acc = acc + (d_a * d_b)), not divided by the count
//   eigenvalues     e1 >= e2 >= e3 of C by cyclic Jacobi in float64 (iss_eigenvalues: a pure function of the six entries)
//   candidate       saliency = e3 if e3 >= 0, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (IEEE divisions, NaN compares false), else -1
//   key point       saliency > 0, at least min_neighbors neighbours at non_max_radius, and no neighbour j there with
//                   saliency[i] < saliency[j] (equal saliencies both survive); key points are listed in ascending index
//
// Layout: the pattern of k_kp_nn_pairs (evaluate.hip), as the all-pairs walk of iss_common.h has it: AP_WALK_SUMS for the scatter
// matrices, ap_walk_flags for the suppression.  All sums run in ascending point index inside one thread, nothing is accumulated across
// threads and there are no atomics: a result is the same bits on every run.  n_pts is clamped to [0, ld]; rows past it are never staged,
// so they never reach a decision; a NaN coordinate only makes comparisons false, and every loop has a fixed bound.
#pragma clang fp contract(off)

#include "iss_common.h"   // the sizes, the all-pairs walk, the Jacobi and the host helpers: shared with harris.hip

struct IssParams {
    double rs2, rn2;   // salient_radius^2, non_max_radius^2: one rounded product each
    double g21, g32;
    int min_nb;
    int ld;
};

// Eigenvalues e[0] >= e[1] >= e[2] of the symmetric matrix (a00 a01 a02; a01 a11 a12; a02 a12 a22): the diagonal iss_jacobi leaves, sorted.
__device__ __forceinline__ void iss_eigenvalues(double a00, double a01, double a02, double a11, double a12, double a22, double e[3]) {
    iss_jacobi<false>(a00, a01, a02, a11, a12, a22, nullptr);
    double t;
    if (a00 < a11) { t = a00; a00 = a11; a11 = t; }
    if (a11 < a22) { t = a11; a11 = a22; a22 = t; }
    if (a00 < a11) { t = a00; a00 = a11; a11 = t; }
    e[0] = a00; e[1] = a11; e[2] = a22;
}

// the scatter matrix: every neighbour counts, with d d^T
struct IssScatterPass : ApSums {
    __device__ __forceinline__ void stage(int, int, int) {}
    __device__ __forceinline__ bool counts(int) const { return true; }
    __device__ __forceinline__ void add(int, double dx, double dy, double dz) { ApSums::add(dx, dy, dz); }
};

__global__ void __launch_bounds__(ISS_TILE) k_iss_scatter(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                          double *__restrict__ saliency, double *__restrict__ eig,
                                                          int32_t *__restrict__ n_neigh, IssParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, prm.ld);
    IssScatterPass c;
    AP_WALK_SUMS(q, prm.rs2, sx, sy, sz, c);
    if (q.i >= prm.ld) return;
    double sal = -1.0, e[3] = {0.0, 0.0, 0.0};
    if (q.valid && c.cnt >= prm.min_nb) {
        iss_eigenvalues(c.cxx, c.cxy, c.cxz, c.cyy, c.cyz, c.czz, e);
        if (e[2] >= 0.0 && __ddiv_rn(e[1], e[0]) < prm.g21 && __ddiv_rn(e[2], e[1]) < prm.g32) sal = e[2];
    } else if (!q.valid) {
        c.cnt = 0;
    }
    const size_t o = q.f * (size_t)prm.ld + q.i;
    saliency[o] = sal;
    if (eig) { eig[o * 3] = e[0]; eig[o * 3 + 1] = e[1]; eig[o * 3 + 2] = e[2]; }
    if (n_neigh) n_neigh[o] = c.cnt;
}

__global__ void __launch_bounds__(ISS_TILE) k_iss_nms(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                      const double *__restrict__ saliency, uint8_t *__restrict__ is_key, IssParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK], ss[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, prm.ld);
    ApSuppress c(q, saliency, prm.ld, ss);
    ap_walk_flags(q, prm.rn2, sx, sy, sz, c);
    if (q.i >= prm.ld) return;
    is_key[q.f * (size_t)prm.ld + q.i] = (q.valid && c.qs > 0.0 && c.cnt >= prm.min_nb && !c.beaten) ? 1 : 0;
}

// One workgroup per frame: the flagged indices in ascending order (wave ballots, the waves' counts through LDS, a running base),
// -1 behind them up to ld, and their number.
__global__ void __launch_bounds__(ISS_SCAN) k_iss_compact(const uint8_t *__restrict__ is_key, const int32_t *__restrict__ n_pts,
                                                          int32_t *__restrict__ key_idx, int32_t *__restrict__ n_key, int ld) {
    __shared__ int wcount[ISS_SCAN / 64];
    const size_t f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = min(max(n_pts[f], 0), ld);
    const uint8_t *flag = is_key + f * (size_t)ld;
    int32_t *out = key_idx + f * (size_t)ld;
    int total = 0;
    for (int base = 0; base < n; base += ISS_SCAN) {
        const int i = base + tid;
        const bool key = i < n && flag[i] != 0;
        const unsigned long long mask = __ballot(key);
        if (lane == 0) wcount[w] = __popcll(mask);
        __syncthreads();
        int before = total;
        for (int v = 0; v < ISS_SCAN / 64; ++v) {
            const int c = wcount[v];
            before += v < w ? c : 0;
            total += c;
        }
        if (key) out[before + __popcll(mask & ((1ull << lane) - 1ull))] = i;   // (before + rank < total <= n <= ld)
        __syncthreads();
    }
    for (int i = total + tid; i < ld; i += ISS_SCAN) out[i] = -1;
    if (tid == 0) n_key[f] = total;
}

int iss_launch_compact(const uint8_t *is_key, const int32_t *n_pts, int32_t *key_idx, int32_t *n_key, int ld, int64_t n_frames, hipStream_t s) {
    k_iss_compact<<<dim3((unsigned)n_frames), ISS_SCAN, 0, s>>>(is_key, n_pts, key_idx, n_key, ld);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

static bool iss_finite_positive(double v) { return iss_finite(v) && v > 0.0; }

CAELO_API int64_t caelo_iss_ws_bytes(int64_t n_frames, int ld) {
    if (n_frames < 0 || ld < 1) return 0;
    return iss_round256((n_frames > 0 ? n_frames : 1) * (int64_t)ld);   // one byte per point: k_iss_nms -> k_iss_compact
}

CAELO_API int caelo_iss_keypoints(caelo_ctx *c, const float *pts, int64_t n_frames, int ld, const int32_t *n_pts, const caelo_iss_params *prm,
                                  double *saliency, double *eig, int32_t *n_neigh, int32_t *key_idx, int32_t *n_key, void *ws,
                                  int64_t ws_bytes, void *stream) {
    ISS_REQUIRE_FRAMES(c, prm, n_frames, ld);
    CAELO_REQUIRE(iss_finite_positive(prm->salient_radius) && iss_finite_positive(prm->non_max_radius), "the radii must be finite and positive");
    CAELO_REQUIRE(iss_finite_positive(prm->gamma_21) && iss_finite_positive(prm->gamma_32), "the gammas must be finite and positive");
    CAELO_REQUIRE(prm->min_neighbors >= 1, "min_neighbors must be at least 1");
    CAELO_REQUIRE(n_frames == 0 || (pts && n_pts && saliency && key_idx && n_key && ws), "null argument");
    CAELO_REQUIRE(ws_bytes >= caelo_iss_ws_bytes(n_frames, ld), "workspace too small (caelo_iss_ws_bytes)");
    if (n_frames == 0) return CAELO_OK;
    IssParams p;
    p.rs2 = prm->salient_radius * prm->salient_radius;
    p.rn2 = prm->non_max_radius * prm->non_max_radius;
    p.g21 = prm->gamma_21;
    p.g32 = prm->gamma_32;
    p.min_nb = prm->min_neighbors;
    p.ld = ld;
    hipStream_t s = caelo_stream(stream);
    uint8_t *is_key = (uint8_t *)ws;
    return iss_run_frames(n_frames, ld, is_key, n_pts, key_idx, n_key, s, [&](dim3 grid, int64_t f0, size_t o) -> int {
        k_iss_scatter<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, saliency + o, eig ? eig + o * 3 : nullptr,
                                                n_neigh ? n_neigh + o : nullptr, p);
        CAELO_LAUNCH_CHECK();
        k_iss_nms<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, saliency + o, is_key + o, p);
        CAELO_LAUNCH_CHECK();
        return CAELO_OK;
    });
}
