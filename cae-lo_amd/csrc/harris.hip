// harris.hip -- Harris3D key points on the device: the second hand-crafted detector of the reference's key point comparison
// (PclKeyPts.py:50-51, :63: PCLKeypoint.keypointHarris, a PCL binding the reference does not ship).
//
// The model is PCL 1.8's HarrisKeypoint3D, method HARRIS, non-maximum suppression on, refinement off, normals from NormalEstimation
// at the same radius; the definition itself is DESIGN.md 9i and is restated here:
//   neighbours   j is a neighbour of i  <=>  d2 < radius * radius (strict; one rounded product; i is its own neighbour),
//                d = double(P[j]) - double(P[i]),  d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded on its own
//   normal       k neighbours; k < 3: invalid.  Otherwise S_a = sum d_a, S_ab = sum d_a * d_b over the neighbours in ascending j,
//                C_ab = S_ab - (S_a * S_b) / double(k); cyclic Jacobi as iss_eigenvalues does it, the rotations accumulated into V
//                from the identity; the normal is the column of the smallest diagonal entry (lowest index on a tie) divided by
//                sqrt((x*x + y*y) + z*z), negated if (n_x*p_x + n_y*p_y) + n_z*p_z > 0 (it faces the sensor at the origin)
//   response     invalid normal: -1.  Otherwise c = neighbours with a valid normal (>= 1), N_ab = (sum n_a * n_b) / double(c) over them in
//                ascending j, tr = (N_xx + N_yy) + N_zz, det = (((N_xx*N_yy)*N_zz + (2*N_xy)*N_xz*N_yz) - (N_xz*N_xz)*N_yy
//                - (N_xy*N_xy)*N_zz) - (N_yz*N_yz)*N_xx left to right, response = (0.04 + det) - (0.04*tr)*tr if tr != 0, else 0
//   key point    valid normal, response >= threshold, and no neighbour j with a valid normal has response[i] < response[j] (equal
//                responses both survive); key points are listed in ascending index
//
// Layout: that of iss.hip, the all-pairs walk of iss_common.h: AP_WALK_SUMS for the normals and the response, ap_walk_flags for the
// suppression; in the second pass the frame's normals and valid bytes, in the third its responses go through LDS beside its points.
// All sums run in ascending point index inside one thread, nothing is accumulated across threads and there are no atomics: a result is
// the same bits on every run.  n_pts is clamped to [0, ld]; rows past it are never staged, so they never reach a decision; a NaN
// coordinate only makes comparisons false, and every loop has a fixed bound.
#pragma clang fp contract(off)

#include "iss_common.h"

struct HarrisParams {
    double r2;          // radius^2: one rounded product
    double threshold;
    int ld;
};

// Unit eigenvector nv[3] of the smallest eigenvalue of the symmetric matrix (a00 a01 a02; a01 a11 a12; a02 a12 a22): iss_jacobi with V
// carried from the identity, then the column of the smallest diagonal entry (lowest index on a tie), normalised.
__device__ __forceinline__ void harris_smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double nv[3]) {
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    iss_jacobi<true>(a00, a01, a02, a11, a12, a22, v);
    const bool c1 = a11 < a00, c2 = a22 < (c1 ? a11 : a00);   // (all nine entries are read: a load under a condition would keep v in memory)
    const double ex = c2 ? v[0][2] : c1 ? v[0][1] : v[0][0];
    const double ey = c2 ? v[1][2] : c1 ? v[1][1] : v[1][0];
    const double ez = c2 ? v[2][2] : c1 ? v[2][1] : v[2][0];
    const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez)));
    nv[0] = __ddiv_rn(ex, nrm); nv[1] = __ddiv_rn(ey, nrm); nv[2] = __ddiv_rn(ez, nrm);
}

// C_ab = S_ab - (S_a * S_b) / k
__device__ __forceinline__ double harris_cov(double sab, double sa, double sb, double k) {
    return __dsub_rn(sab, __ddiv_rn(__dmul_rn(sa, sb), k));
}

// the normals: every neighbour counts, with acc = acc + d_a in front of d d^T
struct HarrisNormalsPass : ApSums {
    double mx = 0.0, my = 0.0, mz = 0.0;
    __device__ __forceinline__ void stage(int, int, int) {}
    __device__ __forceinline__ bool counts(int) const { return true; }
    __device__ __forceinline__ void add(int, double dx, double dy, double dz) {
        mx = __dadd_rn(mx, dx); my = __dadd_rn(my, dy); mz = __dadd_rn(mz, dz);
        ApSums::add(dx, dy, dz);
    }
};

__global__ void __launch_bounds__(ISS_TILE) k_harris_normals(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                             double *__restrict__ normals, uint8_t *__restrict__ has_normal,
                                                             int32_t *__restrict__ n_neigh, HarrisParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, prm.ld);
    HarrisNormalsPass c;
    AP_WALK_SUMS(q, prm.r2, sx, sy, sz, c);
    if (q.i >= prm.ld) return;
    double nv[3] = {0.0, 0.0, 0.0};
    const bool ok = q.valid && c.cnt >= 3;
    if (ok) {
        const double kd = (double)c.cnt;
        harris_smallest_eigenvector(harris_cov(c.cxx, c.mx, c.mx, kd), harris_cov(c.cxy, c.mx, c.my, kd), harris_cov(c.cxz, c.mx, c.mz, kd),
                                    harris_cov(c.cyy, c.my, c.my, kd), harris_cov(c.cyz, c.my, c.mz, kd), harris_cov(c.czz, c.mz, c.mz, kd), nv);
        if (__dadd_rn(__dadd_rn(__dmul_rn(nv[0], q.qx), __dmul_rn(nv[1], q.qy)), __dmul_rn(nv[2], q.qz)) > 0.0) {
            nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2];
        }
    } else if (!q.valid) {
        c.cnt = 0;
    }
    const size_t o = q.f * (size_t)prm.ld + q.i;
    normals[o * 3] = nv[0]; normals[o * 3 + 1] = nv[1]; normals[o * 3 + 2] = nv[2];
    has_normal[o] = ok ? 1 : 0;
    if (n_neigh) n_neigh[o] = c.cnt;
}

// the response: the neighbours with a valid normal count, with n n^T; the frame's normals and valid bytes are staged beside its points
struct HarrisResponsePass : ApSums {
    const double *NV;
    const uint8_t *HV;
    double *snx, *sny, *snz;
    uint8_t *sv;
    __device__ __forceinline__ void stage(int base, int m, int tid) {
        for (int k = tid; k < m; k += ISS_TILE) {
            const double *s = NV + (size_t)(base + k) * 3;
            snx[k] = s[0]; sny[k] = s[1]; snz[k] = s[2];
            sv[k] = HV[base + k];
        }
    }
    __device__ __forceinline__ bool counts(int k) const { return sv[k] != 0; }
    __device__ __forceinline__ void add(int k, double, double, double) { ApSums::add(snx[k], sny[k], snz[k]); }
};

__global__ void __launch_bounds__(ISS_TILE) k_harris_response(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                              const double *__restrict__ normals, const uint8_t *__restrict__ has_normal,
                                                              double *__restrict__ response, HarrisParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK], snx[ISS_CHUNK], sny[ISS_CHUNK], snz[ISS_CHUNK];
    __shared__ uint8_t sv[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, prm.ld);
    HarrisResponsePass c;
    c.NV = normals + q.f * (size_t)prm.ld * 3;
    c.HV = has_normal + q.f * (size_t)prm.ld;
    c.snx = snx; c.sny = sny; c.snz = snz; c.sv = sv;
    const bool ok = q.valid && c.HV[q.i] != 0;
    AP_WALK_SUMS(q, prm.r2, sx, sy, sz, c);
    if (q.i >= prm.ld) return;
    double r = -1.0;
    if (ok) {   // (cnt >= 1: the point is its own neighbour and its normal is valid)
        const double k = (double)c.cnt;
        const double nxx = __ddiv_rn(c.cxx, k), nxy = __ddiv_rn(c.cxy, k), nxz = __ddiv_rn(c.cxz, k);
        const double nyy = __ddiv_rn(c.cyy, k), nyz = __ddiv_rn(c.cyz, k), nzz = __ddiv_rn(c.czz, k);
        const double tr = __dadd_rn(__dadd_rn(nxx, nyy), nzz);
        r = 0.0;
        if (tr != 0.0) {
            double det = __dadd_rn(__dmul_rn(__dmul_rn(nxx, nyy), nzz), __dmul_rn(__dmul_rn(__dmul_rn(2.0, nxy), nxz), nyz));
            det = __dsub_rn(det, __dmul_rn(__dmul_rn(nxz, nxz), nyy));
            det = __dsub_rn(det, __dmul_rn(__dmul_rn(nxy, nxy), nzz));
            det = __dsub_rn(det, __dmul_rn(__dmul_rn(nyz, nyz), nxx));
            r = __dsub_rn(__dadd_rn(0.04, det), __dmul_rn(__dmul_rn(0.04, tr), tr));
        }
    }
    response[q.f * (size_t)prm.ld + q.i] = r;
}

// The third all-pairs pass: a point is flagged when its response is at or above the threshold (which an invalid normal's -1 never is)
// and no neighbour has a larger response (an invalid normal's -1 never is larger: no valid bytes are needed here).  ISS's suppression
// pass; the count it keeps is not read here.
__global__ void __launch_bounds__(ISS_TILE) k_harris_nms(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                         const double *__restrict__ response, uint8_t *__restrict__ is_key, HarrisParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK], ss[ISS_CHUNK];
    const ApQuery q = ap_query(pts, n_pts, prm.ld);
    ApSuppress c(q, response, prm.ld, ss);
    ap_walk_flags(q, prm.r2, sx, sy, sz, c);
    if (q.i >= prm.ld) return;
    is_key[q.f * (size_t)prm.ld + q.i] = (q.valid && c.qs >= prm.threshold && !c.beaten) ? 1 : 0;
}

// workspace: normals [n_frames][ld][3] f64 (used when the caller passes none) | has_normal [n_frames][ld] u8 | is_key [n_frames][ld] u8
CAELO_API int64_t caelo_harris_ws_bytes(int64_t n_frames, int ld) {
    if (n_frames < 0 || ld < 1) return 0;
    const int64_t pts = (n_frames > 0 ? n_frames : 1) * (int64_t)ld;
    return iss_round256(pts * 24) + 2 * iss_round256(pts);
}

CAELO_API int caelo_harris_keypoints(caelo_ctx *c, const float *pts, int64_t n_frames, int ld, const int32_t *n_pts, const caelo_harris_params *prm,
                                     double *response, double *normals, int32_t *n_neigh, int32_t *key_idx, int32_t *n_key, void *ws,
                                     int64_t ws_bytes, void *stream) {
    ISS_REQUIRE_FRAMES(c, prm, n_frames, ld);
    CAELO_REQUIRE(iss_finite(prm->radius) && prm->radius > 0.0, "the radius must be finite and positive");
    CAELO_REQUIRE(iss_finite(prm->threshold) && prm->threshold >= 0.0, "the threshold must be finite and not negative");
    CAELO_REQUIRE(n_frames == 0 || (pts && n_pts && response && key_idx && n_key && ws), "null argument");
    CAELO_REQUIRE(ws_bytes >= caelo_harris_ws_bytes(n_frames, ld), "workspace too small (caelo_harris_ws_bytes)");
    if (n_frames == 0) return CAELO_OK;
    HarrisParams p;
    p.r2 = prm->radius * prm->radius;
    p.threshold = prm->threshold;
    p.ld = ld;
    hipStream_t s = caelo_stream(stream);
    const int64_t all = n_frames * (int64_t)ld;
    double *nv = normals ? normals : (double *)ws;
    uint8_t *has_normal = (uint8_t *)ws + iss_round256(all * 24);
    uint8_t *is_key = has_normal + iss_round256(all);
    return iss_run_frames(n_frames, ld, is_key, n_pts, key_idx, n_key, s, [&](dim3 grid, int64_t f0, size_t o) -> int {
        k_harris_normals<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, nv + o * 3, has_normal + o, n_neigh ? n_neigh + o : nullptr, p);
        CAELO_LAUNCH_CHECK();
        k_harris_response<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, nv + o * 3, has_normal + o, response + o, p);
        CAELO_LAUNCH_CHECK();
        k_harris_nms<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, response + o, is_key + o, p);
        CAELO_LAUNCH_CHECK();
        return CAELO_OK;
    });
}
