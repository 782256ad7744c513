// sift.hip -- SIFT3D key points on the device: the third hand-crafted detector of the reference's key point comparison
// (PclKeyPts.py:55-58, :63: PCLKeypoint.keypointSift, a PCL binding the reference does not ship).
//
// The model is PCL 1.8's SIFTKeypoint on PointXYZ with the point's z coordinate as the filtered field; the definition itself is
// DESIGN.md 9j and is restated here, for one octave (the pyramid over the octaves is the host's: Engine.sift_keypoints):
//   scale space  value_j = double(P[j].z); d2 as in ISS: d = double(P[j]) - double(P[i]), d2 = (dx*dx + dy*dy) + dz*dz.  For every scale
//                s of the S ascending scales: j counts  <=>  d2 <= 9.0 * (sigma[s]*sigma[s]) (not strict; two rounded products; i counts
//                itself), w = exp((-0.5 * d2) / (sigma[s]*sigma[s])), num_s = sum value_j * w and den_s = sum w over the counting j in
//                ascending j, resp_s = num_s / den_s, dog[i][s] = resp_{s+1} - resp_s for s = 0 .. D-1, D = S - 1.  exp is the
//                device's float64 exp, the one operation here that is not correctly rounded.
//   neighbours   the CAELO_SIFT_K = 25 points with the smallest (d2, j) in lexicographic order, the point itself among them; a frame
//                of fewer than 25 points has no key points (its dog is still written)
//   key point    for s = 1 .. D-2, v = dog[i][s], mn[t] / mx[t] the minimum / maximum of dog[j][t] over the 25 neighbours: (i, s) is
//                a key point  <=>  |v| >= min_contrast and (v == mn[s] && v < mn[s-1] && v < mn[s+1]  ||
//                v == mx[s] && v > mx[s-1] && v > mx[s+1]); equal values at the same level both survive
//   output       key_mask[i] has bit s set for every key (i, s); the points with a non-zero mask are listed in ascending index
//
// Layout: the all-pairs walk of iss_common.h twice (AP_WALK_SUMS for the scale space, a walk of its own for the selection), one thread
// per point for the rule, k_iss_compact for the list.  All sums run in ascending point index inside one thread, nothing is accumulated
// across threads and there are no atomics: a result is the same bits on every run.  n_pts is clamped to [0, ld]; rows past it are
// never staged, so they never reach a decision; a NaN coordinate only makes comparisons false, and every loop has a fixed bound.
#pragma clang fp contract(off)

#include "iss_common.h"
#include <cmath>

#define SIFT_K CAELO_SIFT_K
#define SIFT_MAXS CAELO_SIFT_MAX_SCALES
#define SIFT_CELLS 256   // threads of k_sift_centroids

// A kernel argument, uniform over the grid: every entry is read as a scalar.
struct SiftParams {
    double thr[SIFT_MAXS];    // 9.0 * (sigma*sigma); -1 behind the last scale, which no d2 is at or under
    double sig2[SIFT_MAXS];   // sigma*sigma; 1 behind the last scale
    double r2;                // the next double above thr[S-1]: d2 < r2  <=>  d2 <= thr[S-1], the walk's strict test
    double min_contrast;
    int n_scales, ld;
};

// The scale space: 2 * MAXS running sums per lane, all indexed by unrolled constants (they stay in registers).  The scales ascend, so
// a pair inside 9 sigma_s^2 is inside every larger one: the tests below are true from the first such s on.
template <int MAXS>
struct SiftDogPass {
    const SiftParams &prm;
    const double *sz;
    double num[MAXS], den[MAXS];
    __device__ __forceinline__ SiftDogPass(const SiftParams &p, const double *sz_) : prm(p), sz(sz_) {
#pragma unroll
        for (int s = 0; s < MAXS; ++s) num[s] = den[s] = 0.0;
    }
    __device__ __forceinline__ void stage(int, int, int) {}
    __device__ __forceinline__ bool counts(int) const { return true; }
    __device__ __forceinline__ void add(int k, double dx, double dy, double dz) {
        const double d2 = iss_d2(dx, dy, dz), h = __dmul_rn(-0.5, d2), z = sz[k];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            if (d2 <= prm.thr[s]) {
                const double w = exp(__ddiv_rn(h, prm.sig2[s]));
                num[s] = __dadd_rn(num[s], __dmul_rn(z, w));
                den[s] = __dadd_rn(den[s], w);
            }
        }
    }
};

template <int MAXS>
__global__ void __launch_bounds__(ISS_TILE) k_sift_dog(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                       double *__restrict__ dog, SiftParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, prm.ld);
    SiftDogPass<MAXS> c(prm, sz);
    AP_WALK_SUMS(q, prm.r2, sx, sy, sz, c);
    if (q.i >= prm.ld) return;
    const int D = prm.n_scales - 1;
    double *out = dog + (q.f * (size_t)prm.ld + q.i) * D;
    double resp[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) resp[s] = __ddiv_rn(c.num[s], c.den[s]);   // (behind the last scale 0 / 0, never written)
#pragma unroll
    for (int s = 0; s + 1 < MAXS; ++s)
        if (s < D) out[s] = q.valid ? __dsub_rn(resp[s + 1], resp[s]) : 0.0;
}

struct SiftNoStage {
    __device__ __forceinline__ void stage(int, int, int) {}
};

// (d, j) into the ascending list bd, bj: it is carried through the slots and exchanged with every entry it precedes in (d2, j) order;
// what falls off the end is dropped.  Constant indices only.
__device__ __forceinline__ void sift_insert(double (&bd)[SIFT_K], int (&bj)[SIFT_K], double d, int j) {
#pragma unroll
    for (int t = 0; t < SIFT_K; ++t) {
        const bool first = d < bd[t] || (d == bd[t] && j < bj[t]);
        const double od = bd[t];
        const int oj = bj[t];
        bd[t] = first ? d : od;
        bj[t] = first ? j : oj;
        d = first ? od : d;
        j = first ? oj : j;
    }
}

// The 25 nearest points of every point in (d2, j) order.  (d2, j) is a total order, so the selection does not depend on the order
// the points are met in: the walk starts at the chunk the tile itself lies in, whose points are the likeliest to be near, and wraps
// round; the list has then settled before most of the frame goes by, and a pair costs the one compare against the list's last.
__global__ void __launch_bounds__(ISS_TILE) k_sift_knn(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                       int32_t *__restrict__ knn, int ld) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, ld);
    double bd[SIFT_K];
    int bj[SIFT_K];
#pragma unroll
    for (int t = 0; t < SIFT_K; ++t) {
        bd[t] = __builtin_huge_val();
        bj[t] = -1;
    }
    SiftNoStage none;
    const int n_chunks = (q.n_loop + ISS_CHUNK - 1) / ISS_CHUNK, own = (int)blockIdx.x * ISS_TILE / ISS_CHUNK;   // (own < n_chunks when n_loop > 0)
    for (int c = 0; c < n_chunks; ++c) {
        const int base = (own + c < n_chunks ? own + c : own + c - n_chunks) * ISS_CHUNK;
        const int m = min(ISS_CHUNK, q.n_loop - base);
        ap_stage(q, base, m, sx, sy, sz, none);
        int k = 0;
        for (; k + ISS_GROUP <= m; k += ISS_GROUP) {
            double d2[ISS_GROUP];
            bool any = false;
#pragma unroll
            for (int u = 0; u < ISS_GROUP; ++u) {
                d2[u] = iss_d2(__dsub_rn(sx[k + u], q.qx), __dsub_rn(sy[k + u], q.qy), __dsub_rn(sz[k + u], q.qz));
                any |= d2[u] <= bd[SIFT_K - 1];
            }
            if (any) {
#pragma unroll
                for (int u = 0; u < ISS_GROUP; ++u)
                    if (d2[u] <= bd[SIFT_K - 1]) sift_insert(bd, bj, d2[u], base + k + u);
            }
        }
        for (; k < m; ++k) {
            const double d2 = iss_d2(__dsub_rn(sx[k], q.qx), __dsub_rn(sy[k], q.qy), __dsub_rn(sz[k], q.qz));
            if (d2 <= bd[SIFT_K - 1]) sift_insert(bd, bj, d2, base + k);
        }
    }
    if (q.i >= ld) return;
    int32_t *out = knn + (q.f * (size_t)ld + q.i) * SIFT_K;
#pragma unroll
    for (int t = 0; t < SIFT_K; ++t) out[t] = q.valid ? bj[t] : -1;
}

// The rule, one thread per point: level after level the minimum and maximum of dog over the 25 neighbours, the two levels before
// kept, and the rule applied to the middle one.
__global__ void __launch_bounds__(ISS_TILE) k_sift_extrema(const int32_t *__restrict__ n_pts, const double *__restrict__ dog,
                                                           const int32_t *__restrict__ knn, uint32_t *__restrict__ key_mask,
                                                           uint8_t *__restrict__ is_key, double min_contrast, int D, int ld) {
    const size_t f = blockIdx.y;
    const int i = blockIdx.x * ISS_TILE + threadIdx.x;
    if (i >= ld) return;
    const int n = min(max(n_pts[f], 0), ld);
    const size_t o = f * (size_t)ld + i;
    uint32_t mask = 0;
    if (i < n && n >= SIFT_K) {
        const int32_t *nb = knn + o * SIFT_K;
        const double *G = dog + f * (size_t)ld * D;
        double mn0 = 0.0, mx0 = 0.0, mn1 = 0.0, mx1 = 0.0, v1 = 0.0;
        for (int t = 0; t < D; ++t) {
            double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
#pragma unroll 5
            for (int u = 0; u < SIFT_K; ++u) {
                const int j = nb[u];
                if ((unsigned)j < (unsigned)n) {
                    const double g = G[(size_t)j * D + t];
                    mn = g < mn ? g : mn;
                    mx = g > mx ? g : mx;
                }
            }
            if (t >= 2) {   // the level s = t - 1 between s - 1 (mn0, mx0) and s + 1 (mn, mx)
                const double v = v1;
                const bool low = v == mn1 && v < mn0 && v < mn, high = v == mx1 && v > mx0 && v > mx;
                if (fabs(v) >= min_contrast && (low || high)) mask |= 1u << (t - 1);
            }
            mn0 = mn1; mx0 = mx1;
            mn1 = mn; mx1 = mx;
            v1 = G[(size_t)i * D + t];
        }
    }
    key_mask[o] = mask;
    is_key[o] = mask != 0 ? 1 : 0;
}

// One thread per cell: the float64 sums of its run of the stably sorted row order, one row after the other (ascending input row), each
// divided by the count and rounded to float32.
__global__ void __launch_bounds__(SIFT_CELLS) k_sift_centroids(const float *__restrict__ pts, const int32_t *__restrict__ order,
                                                               const int32_t *__restrict__ starts, int n, int n_cells,
                                                               float *__restrict__ out) {
    const int c = blockIdx.x * SIFT_CELLS + threadIdx.x;
    if (c >= n_cells) return;
    const int a = min(max(starts[c], 0), n), b = min(max(starts[c + 1], a), n);
    double x = 0.0, y = 0.0, z = 0.0;
    int cnt = 0;
    for (int r = a; r < b; ++r) {
        const int row = order[r];
        if ((unsigned)row >= (unsigned)n) continue;
        const float *p = pts + (size_t)row * 3;
        // (a sum starts from its first term, not from 0.0: a cell of one point at -0.0 keeps the sign)
        x = cnt ? __dadd_rn(x, (double)p[0]) : (double)p[0];
        y = cnt ? __dadd_rn(y, (double)p[1]) : (double)p[1];
        z = cnt ? __dadd_rn(z, (double)p[2]) : (double)p[2];
        ++cnt;
    }
    const double k = (double)(cnt > 0 ? cnt : 1);
    float *o = out + (size_t)c * 3;
    o[0] = (float)__ddiv_rn(x, k); o[1] = (float)__ddiv_rn(y, k); o[2] = (float)__ddiv_rn(z, k);
}

CAELO_API int caelo_voxel_centroids(caelo_ctx *c, const float *pts, int64_t n_pts, const int32_t *order, const int32_t *starts,
                                    int64_t n_cells, float *centroids, void *stream) {
    CAELO_REQUIRE(c, "null argument");
    CAELO_REQUIRE(n_pts >= 0 && n_pts < (1LL << 31) && n_cells >= 0 && n_cells <= n_pts, "bad shape");
    if (n_cells == 0) return CAELO_OK;
    CAELO_REQUIRE(pts && order && starts && centroids, "null argument");
    hipStream_t s = caelo_stream(stream);
    k_sift_centroids<<<dim3((unsigned)((n_cells + SIFT_CELLS - 1) / SIFT_CELLS)), SIFT_CELLS, 0, s>>>(pts, order, starts, (int)n_pts,
                                                                                                      (int)n_cells, centroids);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

// workspace: knn [n_frames][ld][25] i32 (used when the caller passes none) | is_key [n_frames][ld] u8
CAELO_API int64_t caelo_sift_ws_bytes(int64_t n_frames, int ld) {
    if (n_frames < 0 || ld < 1) return 0;
    const int64_t pts = (n_frames > 0 ? n_frames : 1) * (int64_t)ld;
    return iss_round256(pts * SIFT_K * 4) + iss_round256(pts);
}

CAELO_API int caelo_sift_octave(caelo_ctx *c, const float *pts, int64_t n_frames, int ld, const int32_t *n_pts, const caelo_sift_params *prm,
                                double *dog, int32_t *knn, uint32_t *key_mask, int32_t *key_idx, int32_t *n_key, void *ws,
                                int64_t ws_bytes, void *stream) {
    ISS_REQUIRE_FRAMES(c, prm, n_frames, ld);
    CAELO_REQUIRE(prm->n_scales >= 3 && prm->n_scales <= SIFT_MAXS, "n_scales must lie in [3, CAELO_SIFT_MAX_SCALES]");
    for (int s = 0; s < prm->n_scales; ++s)
        CAELO_REQUIRE(iss_finite(prm->sigma[s]) && prm->sigma[s] > 0.0 && (s == 0 || prm->sigma[s] > prm->sigma[s - 1]),
                      "the scales must be finite, positive and increasing");
    CAELO_REQUIRE(iss_finite(prm->min_contrast) && prm->min_contrast >= 0.0, "min_contrast must be finite and not negative");
    CAELO_REQUIRE(n_frames == 0 || (pts && n_pts && dog && key_mask && key_idx && n_key && ws), "null argument");
    CAELO_REQUIRE(ws_bytes >= caelo_sift_ws_bytes(n_frames, ld), "workspace too small (caelo_sift_ws_bytes)");
    if (n_frames == 0) return CAELO_OK;
    SiftParams p;
    const int S = prm->n_scales, D = S - 1;
    for (int s = 0; s < SIFT_MAXS; ++s) {
        p.sig2[s] = s < S ? prm->sigma[s] * prm->sigma[s] : 1.0;
        p.thr[s] = s < S ? 9.0 * p.sig2[s] : -1.0;
    }
    p.r2 = std::nextafter(p.thr[S - 1], (double)INFINITY);
    p.min_contrast = prm->min_contrast;
    p.n_scales = S;
    p.ld = ld;
    hipStream_t s = caelo_stream(stream);
    const int64_t all = n_frames * (int64_t)ld;
    int32_t *nn = knn ? knn : (int32_t *)ws;
    uint8_t *is_key = (uint8_t *)ws + iss_round256(all * SIFT_K * 4);
    return iss_run_frames(n_frames, ld, is_key, n_pts, key_idx, n_key, s, [&](dim3 grid, int64_t f0, size_t o) -> int {
        if (S <= 11)
            k_sift_dog<11><<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, dog + o * D, p);
        else
            k_sift_dog<SIFT_MAXS><<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, dog + o * D, p);
        CAELO_LAUNCH_CHECK();
        k_sift_knn<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, nn + o * SIFT_K, ld);
        CAELO_LAUNCH_CHECK();
        k_sift_extrema<<<grid, ISS_TILE, 0, s>>>(n_pts + f0, dog + o * D, nn + o * SIFT_K, key_mask + o, is_key + o, p.min_contrast, D, ld);
        CAELO_LAUNCH_CHECK();
        return CAELO_OK;
    });
}
