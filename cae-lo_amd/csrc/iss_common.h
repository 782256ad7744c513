// iss_common.h -- what the all-pairs float64 key point detectors share (iss.hip, harris.hip): the tile and chunk sizes, the staging
// of a chunk of points through LDS, the rounded squared distance, one Jacobi rotation, and the ordered compaction of a flag
// array.  Every function here is a pure function of its arguments with every operation rounded on its own; a translation unit that
// includes this header sets `#pragma clang fp contract(off)` before it does.
#pragma once
#include "caelo_internal.h"

#define ISS_TILE 256
#define ISS_CHUNK 1024
#define ISS_GROUP 4        // points per step of the inner loop of the passes that sum (k_iss_scatter, k_harris_normals, k_harris_response)
#define ISS_SCAN 1024      // threads of k_iss_compact
#define ISS_SWEEPS 12      // a 3 x 3 matrix is through after 5 or 6; the bound is what ends a matrix of NaNs
#define ISS_MAX_GRID_Y 65535

// One Jacobi rotation that annihilates a_pq; a_rp and a_rq are the other two off-diagonal entries (r the third index).
// An entry that changes neither diagonal neighbour when added to it is set to zero without a rotation.  A zero a_pq is left alone,
// and a row and column of zeros stay zeros: c * 0 - s * 0 and s * 0 + c * 0 are 0, and the diagonal entry is never touched.
// -> true when a rotation was applied; c and s are then its cosine and sine (the caller may apply them to eigenvectors:
// v_p' = c * v_p - s * v_q, v_q' = s * v_p + c * v_q), else they are left alone.
__device__ __forceinline__ bool iss_rotate_cs(double &app, double &aqq, double &apq, double &arp, double &arq, double &c, double &s) {
    if (apq == 0.0) return false;
    const double g = fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        apq = 0.0;
        return false;
    }
    const double theta = __ddiv_rn(aqq - app, 2.0 * apq);
    const double t = __ddiv_rn(copysign(1.0, theta), fabs(theta) + __dsqrt_rn(theta * theta + 1.0));   // (theta^2 = inf: t = 0)
    c = __ddiv_rn(1.0, __dsqrt_rn(t * t + 1.0));
    s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    return true;
}

__device__ __forceinline__ void iss_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
    double c, s;
    iss_rotate_cs(app, aqq, apq, arp, arq, c, s);
}

// stage points base .. base + m - 1 of the frame as float64 (between two barriers of the caller)
__device__ __forceinline__ void iss_stage(const float *__restrict__ P, int base, int m, int tid, double *sx, double *sy, double *sz) {
    for (int k = tid; k < m; k += ISS_TILE) {
        const float *s = P + (size_t)(base + k) * 3;
        sx[k] = (double)s[0]; sy[k] = (double)s[1]; sz[k] = (double)s[2];
    }
}

__device__ __forceinline__ double iss_d2(double dx, double dy, double dz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// k_iss_compact (iss.hip) for n_frames frames on `s`: per frame the flagged indices of is_key [n_frames][ld] in ascending order into
// key_idx [n_frames][ld], -1 behind them, and their number into n_key.  -> CAELO_OK or CAELO_ERR_HIP (the error text is set).
int iss_launch_compact(const uint8_t *is_key, const int32_t *n_pts, int32_t *key_idx, int32_t *n_key, int ld, int64_t n_frames, hipStream_t s);
