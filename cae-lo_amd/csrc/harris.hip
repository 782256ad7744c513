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
// Layout: that of iss.hip.  A workgroup is (tile of ISS_TILE query points, frame); the frame's points -- and in the second pass their
// normals and valid bytes, in the third their responses -- go through LDS as float64 in chunks of ISS_CHUNK, every lane reading the
// same address (a broadcast).  All sums run in ascending point index inside one thread, nothing is accumulated across threads and
// there are no atomics: a result is the same bits on every run.  n_pts is clamped to [0, ld]; rows past it are never staged, so they
// never reach a decision; a NaN coordinate only makes comparisons false, and every loop has a fixed bound.
#pragma clang fp contract(off)

#include "iss_common.h"

struct HarrisParams {
    double r2;          // radius^2: one rounded product
    double threshold;
    int ld;
};

// Unit eigenvector nv[3] of the smallest eigenvalue of the symmetric matrix (a00 a01 a02; a01 a11 a12; a02 a12 a22): the cyclic Jacobi
// of iss_eigenvalues (same rotation order, formulas, skip rule and sweep bound), every rotation applied to V as well, V = I at the start.
// A pure function of the six entries; a row and column that are exactly zero keep their unit vector exactly.
__device__ __forceinline__ void harris_smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double nv[3]) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v_rc: row r, column c
    double c, s, x, y;
    for (int sweep = 0; sweep < ISS_SWEEPS; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        if (iss_rotate_cs(a00, a11, a01, a02, a12, c, s)) {   // columns 0 and 1
            x = v00; y = v01; v00 = c * x - s * y; v01 = s * x + c * y;
            x = v10; y = v11; v10 = c * x - s * y; v11 = s * x + c * y;
            x = v20; y = v21; v20 = c * x - s * y; v21 = s * x + c * y;
        }
        if (iss_rotate_cs(a00, a22, a02, a01, a12, c, s)) {   // columns 0 and 2
            x = v00; y = v02; v00 = c * x - s * y; v02 = s * x + c * y;
            x = v10; y = v12; v10 = c * x - s * y; v12 = s * x + c * y;
            x = v20; y = v22; v20 = c * x - s * y; v22 = s * x + c * y;
        }
        if (iss_rotate_cs(a11, a22, a12, a01, a02, c, s)) {   // columns 1 and 2
            x = v01; y = v02; v01 = c * x - s * y; v02 = s * x + c * y;
            x = v11; y = v12; v11 = c * x - s * y; v12 = s * x + c * y;
            x = v21; y = v22; v21 = c * x - s * y; v22 = s * x + c * y;
        }
    }
    double ex = v00, ey = v10, ez = v20, e = a00;
    if (a11 < e) { ex = v01; ey = v11; ez = v21; e = a11; }
    if (a22 < e) { ex = v02; ey = v12; ez = v22; }
    const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez)));
    nv[0] = __ddiv_rn(ex, nrm); nv[1] = __ddiv_rn(ey, nrm); nv[2] = __ddiv_rn(ez, nrm);
}

// acc = acc + d_a and acc = acc + (d_a * d_b): nine sums
__device__ __forceinline__ void harris_accumulate(double dx, double dy, double dz, double &sx, double &sy, double &sz, double &cxx, double &cxy,
                                                  double &cxz, double &cyy, double &cyz, double &czz) {
    sx = __dadd_rn(sx, dx); sy = __dadd_rn(sy, dy); sz = __dadd_rn(sz, dz);
    cxx = __dadd_rn(cxx, __dmul_rn(dx, dx)); cxy = __dadd_rn(cxy, __dmul_rn(dx, dy)); cxz = __dadd_rn(cxz, __dmul_rn(dx, dz));
    cyy = __dadd_rn(cyy, __dmul_rn(dy, dy)); cyz = __dadd_rn(cyz, __dmul_rn(dy, dz)); czz = __dadd_rn(czz, __dmul_rn(dz, dz));
}

// C_ab = S_ab - (S_a * S_b) / k
__device__ __forceinline__ double harris_cov(double sab, double sa, double sb, double k) {
    return __dsub_rn(sab, __ddiv_rn(__dmul_rn(sa, sb), k));
}

__global__ void __launch_bounds__(ISS_TILE) k_harris_normals(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                             double *__restrict__ normals, uint8_t *__restrict__ has_normal,
                                                             int32_t *__restrict__ n_neigh, HarrisParams prm) {
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
    double mx = 0.0, my = 0.0, mz = 0.0, cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    const int n_loop = (int)blockIdx.x * ISS_TILE < n ? n : 0;   // (uniform over the workgroup: a tile past the frame only writes defaults)
    for (int base = 0; base < n_loop; base += ISS_CHUNK) {
        const int m = min(ISS_CHUNK, n_loop - base);
        __syncthreads();
        iss_stage(P, base, m, tid, sx, sy, sz);
        __syncthreads();
        // as k_iss_scatter: four branch-free distances, and the sums visited in ascending order only when some lane has a neighbour
        int k = 0;
        for (; k + ISS_GROUP <= m; k += ISS_GROUP) {
            double dx[ISS_GROUP], dy[ISS_GROUP], dz[ISS_GROUP];
            bool in[ISS_GROUP], any = false;
#pragma unroll
            for (int u = 0; u < ISS_GROUP; ++u) {
                dx[u] = __dsub_rn(sx[k + u], qx); dy[u] = __dsub_rn(sy[k + u], qy); dz[u] = __dsub_rn(sz[k + u], qz);
                in[u] = iss_d2(dx[u], dy[u], dz[u]) < prm.r2;
                any |= in[u];
            }
            if (any) {
#pragma unroll
                for (int u = 0; u < ISS_GROUP; ++u)
                    if (in[u]) { ++cnt; harris_accumulate(dx[u], dy[u], dz[u], mx, my, mz, cxx, cxy, cxz, cyy, cyz, czz); }
            }
        }
        for (; k < m; ++k) {
            const double dx = __dsub_rn(sx[k], qx), dy = __dsub_rn(sy[k], qy), dz = __dsub_rn(sz[k], qz);
            if (iss_d2(dx, dy, dz) < prm.r2) { ++cnt; harris_accumulate(dx, dy, dz, mx, my, mz, cxx, cxy, cxz, cyy, cyz, czz); }
        }
    }
    if (i >= prm.ld) return;
    double nv[3] = {0.0, 0.0, 0.0};
    const bool ok = valid && cnt >= 3;
    if (ok) {
        const double kd = (double)cnt;
        harris_smallest_eigenvector(harris_cov(cxx, mx, mx, kd), harris_cov(cxy, mx, my, kd), harris_cov(cxz, mx, mz, kd),
                                    harris_cov(cyy, my, my, kd), harris_cov(cyz, my, mz, kd), harris_cov(czz, mz, mz, kd), nv);
        if (__dadd_rn(__dadd_rn(__dmul_rn(nv[0], qx), __dmul_rn(nv[1], qy)), __dmul_rn(nv[2], qz)) > 0.0) {
            nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2];
        }
    } else if (!valid) {
        cnt = 0;
    }
    const size_t o = f * (size_t)prm.ld + i;
    normals[o * 3] = nv[0]; normals[o * 3 + 1] = nv[1]; normals[o * 3 + 2] = nv[2];
    has_normal[o] = ok ? 1 : 0;
    if (n_neigh) n_neigh[o] = cnt;
}

// acc = acc + (n_a * n_b), six sums
__device__ __forceinline__ void harris_accumulate_normal(double nx, double ny, double nz, double &cxx, double &cxy, double &cxz, double &cyy,
                                                         double &cyz, double &czz) {
    cxx = __dadd_rn(cxx, __dmul_rn(nx, nx)); cxy = __dadd_rn(cxy, __dmul_rn(nx, ny)); cxz = __dadd_rn(cxz, __dmul_rn(nx, nz));
    cyy = __dadd_rn(cyy, __dmul_rn(ny, ny)); cyz = __dadd_rn(cyz, __dmul_rn(ny, nz)); czz = __dadd_rn(czz, __dmul_rn(nz, nz));
}

__global__ void __launch_bounds__(ISS_TILE) k_harris_response(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                              const double *__restrict__ normals, const uint8_t *__restrict__ has_normal,
                                                              double *__restrict__ response, HarrisParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK], snx[ISS_CHUNK], sny[ISS_CHUNK], snz[ISS_CHUNK];
    __shared__ uint8_t sv[ISS_CHUNK];
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const int n = min(max(n_pts[f], 0), prm.ld);
    const int i = blockIdx.x * ISS_TILE + tid;
    const float *P = pts + f * (size_t)prm.ld * 3;
    const double *NV = normals + f * (size_t)prm.ld * 3;
    const uint8_t *HV = has_normal + f * (size_t)prm.ld;
    const bool valid = i < n;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    bool ok = false;
    if (valid) {
        const float *q = P + (size_t)i * 3;
        qx = (double)q[0]; qy = (double)q[1]; qz = (double)q[2];
        ok = HV[i] != 0;
    }
    int cnt = 0;
    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    const int n_loop = (int)blockIdx.x * ISS_TILE < n ? n : 0;
    for (int base = 0; base < n_loop; base += ISS_CHUNK) {
        const int m = min(ISS_CHUNK, n_loop - base);
        __syncthreads();
        iss_stage(P, base, m, tid, sx, sy, sz);
        for (int k = tid; k < m; k += ISS_TILE) {
            const double *s = NV + (size_t)(base + k) * 3;
            snx[k] = s[0]; sny[k] = s[1]; snz[k] = s[2];
            sv[k] = HV[base + k];
        }
        __syncthreads();
        int k = 0;
        for (; k + ISS_GROUP <= m; k += ISS_GROUP) {
            bool in[ISS_GROUP], any = false;
#pragma unroll
            for (int u = 0; u < ISS_GROUP; ++u) {
                const double dx = __dsub_rn(sx[k + u], qx), dy = __dsub_rn(sy[k + u], qy), dz = __dsub_rn(sz[k + u], qz);
                in[u] = (iss_d2(dx, dy, dz) < prm.r2) & (sv[k + u] != 0);
                any |= in[u];
            }
            if (any) {
#pragma unroll
                for (int u = 0; u < ISS_GROUP; ++u)
                    if (in[u]) { ++cnt; harris_accumulate_normal(snx[k + u], sny[k + u], snz[k + u], cxx, cxy, cxz, cyy, cyz, czz); }
            }
        }
        for (; k < m; ++k) {
            const double dx = __dsub_rn(sx[k], qx), dy = __dsub_rn(sy[k], qy), dz = __dsub_rn(sz[k], qz);
            if ((iss_d2(dx, dy, dz) < prm.r2) & (sv[k] != 0)) { ++cnt; harris_accumulate_normal(snx[k], sny[k], snz[k], cxx, cxy, cxz, cyy, cyz, czz); }
        }
    }
    if (i >= prm.ld) return;
    double r = -1.0;
    if (ok) {   // (cnt >= 1: the point is its own neighbour and its normal is valid)
        const double c = (double)cnt;
        const double nxx = __ddiv_rn(cxx, c), nxy = __ddiv_rn(cxy, c), nxz = __ddiv_rn(cxz, c);
        const double nyy = __ddiv_rn(cyy, c), nyz = __ddiv_rn(cyz, c), nzz = __ddiv_rn(czz, c);
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
    response[f * (size_t)prm.ld + i] = r;
}

// The third all-pairs pass: a point is flagged when its response is at or above the threshold (which an invalid normal's -1 never is)
// and no neighbour has a larger response (an invalid normal's -1 never is larger: no valid bytes are needed here).
__global__ void __launch_bounds__(ISS_TILE) k_harris_nms(const float *__restrict__ pts, const int32_t *__restrict__ n_pts,
                                                         const double *__restrict__ response, uint8_t *__restrict__ is_key, HarrisParams prm) {
    __shared__ double sx[ISS_CHUNK], sy[ISS_CHUNK], sz[ISS_CHUNK], ss[ISS_CHUNK];
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const int n = min(max(n_pts[f], 0), prm.ld);
    const int i = blockIdx.x * ISS_TILE + tid;
    const float *P = pts + f * (size_t)prm.ld * 3;
    const double *S = response + f * (size_t)prm.ld;
    const bool valid = i < n;
    double qx = 0.0, qy = 0.0, qz = 0.0, qs = -1.0;
    if (valid) {
        const float *q = P + (size_t)i * 3;
        qx = (double)q[0]; qy = (double)q[1]; qz = (double)q[2];
        qs = S[i];
    }
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
            beaten |= (iss_d2(dx, dy, dz) < prm.r2) & (qs < ss[k]);   // (branch-free)
        }
    }
    if (i >= prm.ld) return;
    is_key[f * (size_t)prm.ld + i] = (valid && qs >= prm.threshold && !beaten) ? 1 : 0;
}

static bool harris_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

static int64_t harris_round256(int64_t v) { return (v + 255) / 256 * 256; }

// workspace: normals [n_frames][ld][3] f64 (used when the caller passes none) | has_normal [n_frames][ld] u8 | is_key [n_frames][ld] u8
CAELO_API int64_t caelo_harris_ws_bytes(int64_t n_frames, int ld) {
    if (n_frames < 0 || ld < 1) return 0;
    const int64_t pts = (n_frames > 0 ? n_frames : 1) * (int64_t)ld;
    return harris_round256(pts * 24) + 2 * harris_round256(pts);
}

CAELO_API int caelo_harris_keypoints(caelo_ctx *c, const float *pts, int64_t n_frames, int ld, const int32_t *n_pts, const caelo_harris_params *prm,
                                     double *response, double *normals, int32_t *n_neigh, int32_t *key_idx, int32_t *n_key, void *ws,
                                     int64_t ws_bytes, void *stream) {
    CAELO_REQUIRE(c && prm, "null argument");
    CAELO_REQUIRE(n_frames >= 0 && n_frames < (1LL << 31), "bad shape");
    CAELO_REQUIRE(ld >= 1 && ld <= CAELO_ISS_MAX_POINTS, "ld must lie in [1, CAELO_ISS_MAX_POINTS]");
    CAELO_REQUIRE(harris_finite(prm->radius) && prm->radius > 0.0, "the radius must be finite and positive");
    CAELO_REQUIRE(harris_finite(prm->threshold) && prm->threshold >= 0.0, "the threshold must be finite and not negative");
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
    uint8_t *has_normal = (uint8_t *)ws + harris_round256(all * 24);
    uint8_t *is_key = has_normal + harris_round256(all);
    const unsigned tiles = (unsigned)((ld + ISS_TILE - 1) / ISS_TILE);
    for (int64_t f0 = 0; f0 < n_frames; f0 += ISS_MAX_GRID_Y) {   // the frame is blockIdx.y: slices of what a grid's y takes
        const int64_t nf = n_frames - f0 < ISS_MAX_GRID_Y ? n_frames - f0 : ISS_MAX_GRID_Y;
        const size_t o = (size_t)f0 * ld;
        const dim3 grid(tiles, (unsigned)nf);
        k_harris_normals<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, nv + o * 3, has_normal + o, n_neigh ? n_neigh + o : nullptr, p);
        CAELO_LAUNCH_CHECK();
        k_harris_response<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, nv + o * 3, has_normal + o, response + o, p);
        CAELO_LAUNCH_CHECK();
        k_harris_nms<<<grid, ISS_TILE, 0, s>>>(pts + o * 3, n_pts + f0, response + o, is_key + o, p);
        CAELO_LAUNCH_CHECK();
    }
    return iss_launch_compact(is_key, n_pts, key_idx, n_key, ld, n_frames, s);
}
