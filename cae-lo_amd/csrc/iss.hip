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
// Layout: the pattern of k_kp_nn_pairs (evaluate.hip).  A workgroup is (tile of ISS_TILE query points, frame); the frame's points go
// through LDS as float64 in chunks of ISS_CHUNK and every lane reads the same LDS address (a broadcast).  All sums run in ascending
// point index inside one thread, nothing is accumulated across threads and there are no atomics: a result is the same bits on
// every run.  n_pts is clamped to [0, ld]; rows past it are never staged, so they never reach a decision; a NaN coordinate only
// makes comparisons false, and every loop has a fixed bound.
#pragma clang fp contract(off)

#include "iss_common.h"   // the sizes, iss_rotate, iss_stage, iss_d2: shared with harris.hip

struct IssParams {
    double rs2, rn2;   // salient_radius^2, non_max_radius^2: one rounded product each
    double g21, g32;
    int min_nb;
    int ld;
};

// Eigenvalues e[0] >= e[1] >= e[2] of the symmetric matrix (a00 a01 a02; a01 a11 a12; a02 a12 a22): cyclic Jacobi, rotations in
// the order (0,1), (0,2), (1,2), until the off-diagonal is exactly zero or ISS_SWEEPS sweeps are done.
__device__ __forceinline__ void iss_eigenvalues(double a00, double a01, double a02, double a11, double a12, double a22, double e[3]) {
    for (int sweep = 0; sweep < ISS_SWEEPS; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        iss_rotate(a00, a11, a01, a02, a12);
        iss_rotate(a00, a22, a02, a01, a12);
        iss_rotate(a11, a22, a12, a01, a02);
    }
    double t;
    if (a00 < a11) { t = a00; a00 = a11; a11 = t; }
    if (a11 < a22) { t = a11; a11 = a22; a22 = t; }
    if (a00 < a11) { t = a00; a00 = a11; a11 = t; }
    e[0] = a00; e[1] = a11; e[2] = a22;
}

// acc = acc + (d_a * d_b), six sums
__device__ __forceinline__ void iss_accumulate(double dx, double dy, double dz, double &cxx, double &cxy, double &cxz, double &cyy,
                                               double &cyz, double &czz) {
    cxx = __dadd_rn(cxx, __dmul_rn(dx, dx)); cxy = __dadd_rn(cxy, __dmul_rn(dx, dy)); cxz = __dadd_rn(cxz, __dmul_rn(dx, dz));
    cyy = __dadd_rn(cyy, __dmul_rn(dy, dy)); cyz = __dadd_rn(cyz, __dmul_rn(dy, dz)); czz = __dadd_rn(czz, __dmul_rn(dz, dz));
}

__global__ void __launch_bounds__(ISS_TILE) k_iss_scatter(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                          double *__restrict__ saliency, double *__restrict__ eig,
                                                          int32_t *__restrict__ n_neigh, IssParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK];
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const int n = min(max(n_pts[f], 0), prm.ld);
    const int i = blockIdx.x * ISS_TILE + tid;
    const float *P = pts + f * (size_t)prm.ld * 3;
    const bool valid = i < n;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (valid) {
        const float *q = P + (size_t)i * 3;
        qx = (double)q[0]; qy = (double)q[1]; qz = (double)q[2];
    }
    int cnt = 0;
    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    const int n_loop = (int)blockIdx.x * ISS_TILE < n ? n : 0;   // (uniform over the workgroup: a tile past the frame only writes defaults)
    for (int base = 0; base < n_loop; base += ISS_CHUNK) {
        const int m = min(ISS_CHUNK, n_loop - base);
        __syncthreads();
        iss_stage(P, base, m, tid, sx, sy, sz);
        __syncthreads();
        // all lanes read the same address: LDS broadcast.  Four points at a time: the distances are branch-free, and the sums are
        // visited (in the same ascending order) only when one of the four is a neighbour of some lane -- one point in a hundred is
        int k = 0;
        for (; k + ISS_GROUP <= m; k += ISS_GROUP) {
            double dx[ISS_GROUP], dy[ISS_GROUP], dz[ISS_GROUP];
            bool in[ISS_GROUP], any = false;
#pragma unroll
            for (int u = 0; u < ISS_GROUP; ++u) {
                dx[u] = __dsub_rn(sx[k + u], qx); dy[u] = __dsub_rn(sy[k + u], qy); dz[u] = __dsub_rn(sz[k + u], qz);
                in[u] = iss_d2(dx[u], dy[u], dz[u]) < prm.rs2;
                any |= in[u];
            }
            if (any) {
#pragma unroll
                for (int u = 0; u < ISS_GROUP; ++u)
                    if (in[u]) { ++cnt; iss_accumulate(dx[u], dy[u], dz[u], cxx, cxy, cxz, cyy, cyz, czz); }
            }
        }
        for (; k < m; ++k) {
            const double dx = __dsub_rn(sx[k], qx), dy = __dsub_rn(sy[k], qy), dz = __dsub_rn(sz[k], qz);
            if (iss_d2(dx, dy, dz) < prm.rs2) { ++cnt; iss_accumulate(dx, dy, dz, cxx, cxy, cxz, cyy, cyz, czz); }
        }
    }
    if (i >= prm.ld) return;
    double sal = -1.0, e[3] = {0.0, 0.0, 0.0};
    if (valid && cnt >= prm.min_nb) {
        iss_eigenvalues(cxx, cxy, cxz, cyy, cyz, czz, e);
        if (e[2] >= 0.0 && __ddiv_rn(e[1], e[0]) < prm.g21 && __ddiv_rn(e[2], e[1]) < prm.g32) sal = e[2];
    } else if (!valid) {
        cnt = 0;
    }
    const size_t o = f * (size_t)prm.ld + i;
    saliency[o] = sal;
    if (eig) { eig[o * 3] = e[0]; eig[o * 3 + 1] = e[1]; eig[o * 3 + 2] = e[2]; }
    if (n_neigh) n_neigh[o] = cnt;
}

__global__ void __launch_bounds__(ISS_TILE) k_iss_nms(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                      const double *__restrict__ saliency, uint8_t *__restrict__ is_key, IssParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK], ss[ISS_CHUNK];
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const int n = min(max(n_pts[f], 0), prm.ld);
    const int i = blockIdx.x * ISS_TILE + tid;
    const float *P = pts + f * (size_t)prm.ld * 3;
    const double *S = saliency + f * (size_t)prm.ld;
    const bool valid = i < n;
    double qx = 0.0, qy = 0.0, qz = 0.0, qs = -1.0;
    if (valid) {
        const float *q = P + (size_t)i * 3;
        qx = (double)q[0]; qy = (double)q[1]; qz = (double)q[2];
        qs = S[i];
    }
    int cnt = 0;
    bool beaten = false;
    const int n_loop = (int)blockIdx.x * ISS_TILE < n ? n : 0;
    for (int base = 0; base < n_loop; base += ISS_CHUNK) {
        const int m = min(ISS_CHUNK, n_loop - base);
        __syncthreads();
        iss_stage(P, base, m, tid, sx, sy, sz);
        for (int k = tid; k < m; k += ISS_TILE) ss[k] = S[base + k];
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < m; ++k) {
            const double dx = __dsub_rn(sx[k], qx), dy = __dsub_rn(sy[k], qy), dz = __dsub_rn(sz[k], qz);
            const bool in = iss_d2(dx, dy, dz) < prm.rn2;   // (branch-free: a compare, an add and two mask operations per pair)
            cnt += in ? 1 : 0;
            beaten |= in & (qs < ss[k]);
        }
    }
    if (i >= prm.ld) return;
    is_key[f * (size_t)prm.ld + i] = (valid && qs > 0.0 && cnt >= prm.min_nb && !beaten) ? 1 : 0;
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

static bool iss_finite_positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

CAELO_API int64_t caelo_iss_ws_bytes(int64_t n_frames, int ld) {
    if (n_frames < 0 || ld < 1) return 0;
    const int64_t flags = (n_frames > 0 ? n_frames : 1) * (int64_t)ld;   // one byte per point: k_iss_nms -> k_iss_compact
    return (flags + 255) / 256 * 256;
}

CAELO_API int caelo_iss_keypoints(caelo_ctx *c, const float *pts, int64_t n_frames, int ld, const int32_t *n_pts, const caelo_iss_params *prm,
                                  double *saliency, double *eig, int32_t *n_neigh, int32_t *key_idx, int32_t *n_key, void *ws,
                                  int64_t ws_bytes, void *stream) {
    CAELO_REQUIRE(c && prm, "null argument");
    CAELO_REQUIRE(n_frames >= 0 && n_frames < (1LL << 31), "bad shape");
    CAELO_REQUIRE(ld >= 1 && ld <= CAELO_ISS_MAX_POINTS, "ld must lie in [1, CAELO_ISS_MAX_POINTS]");
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
    const unsigned tiles = (unsigned)((ld + ISS_TILE - 1) / ISS_TILE);
    for (int64_t f0 = 0; f0 < n_frames; f0 += ISS_MAX_GRID_Y) {   // the frame is blockIdx.y: slices of what a grid's y takes
        const int64_t nf = n_frames - f0 < ISS_MAX_GRID_Y ? n_frames - f0 : ISS_MAX_GRID_Y;
        const size_t o = (size_t)f0 * ld;
        const dim3 grid(tiles, (unsigned)nf);
        k_iss_scatter<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, saliency + o, eig ? eig + o * 3 : nullptr,
                                                n_neigh ? n_neigh + o : nullptr, p);
        CAELO_LAUNCH_CHECK();
        k_iss_nms<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, saliency + o, is_key + o, p);
        CAELO_LAUNCH_CHECK();
    }
    return iss_launch_compact(is_key, n_pts, key_idx, n_key, ld, n_frames, s);
}
