// adaptive.hip -- the comparison protocol's registrar (Scripts/GenerateTrajactory.m:203-237 -> External/ransacfitRt.m, ransac.m,
// estimateRigidTransform.m, quat2rot.m): 3-point samples, a quaternion least-squares fit, ONE inlier threshold, an adaptive trial
// count and a refit on the best trial's inliers, float64 throughout.  include/caelo.h states the contract; DESIGN.md 9k the design.
//
// The sample rule, the fit, the inlier test and the walk are __host__ __device__ functions: k_adaptive runs them with a workgroup
// per pair, caelo_host_ransac_adaptive runs them on host arrays one trial after the other (the CPU tests pin every branch there, and
// a stand-alone host program can call it under a sanitizer).  A trial's model is the same operations in the same order on both
// sides; only the refit's sums are a tree on the device and a loop on the host.
//
// The kernel scores AD_C trials AHEAD of the walk: AD_C threads fit one trial each into LDS, every thread scores its own point pair
// against the AD_C models (broadcast LDS reads, a ballot and a popcount per wavefront and model, added into LDS counters -- integer
// adds: any order gives the same sum), then ONE thread walks the chunk's counts exactly like ransac.m:140-229 walks its trials.  A trial
// at or past the index where that loop stops is never looked at, whatever it would have scored, and among equal counts the later trial
// wins (`>=`): the result is the sequential loop's.  Nothing crosses workgroups, nothing is written to global memory before the end.
#include "caelo_internal.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

#define AD_HD __host__ __device__ inline
#define AD_THREADS 1024    // one point pair per thread (n <= CAELO_MAX_KEYPTS)
#define AD_WAVES (AD_THREADS / 64)
#define AD_C 128           // trials per chunk: the 100 trials every pair runs at least are one chunk
#define AD_SWEEPS 30       // a 4 x 4 matrix is through after 6 to 8; the bound is what ends a matrix of NaNs
#define AD_TERMS 15
static_assert(CAELO_MAX_KEYPTS == AD_THREADS, "one thread per key point");
static_assert(AD_C == 128, "k_adaptive keeps a wavefront's counts of a chunk in two registers per lane");

// ---- the sample rule (this project's: three distinct indices from three uniform doubles) -----------------------------------------
AD_HD int ad_pick(double u, int m) {   // min(floor(u m), m - 1), and 0 for anything below 0 or not a number
    const double f = floor(u * (double)m);
    return f >= 0.0 ? (f < (double)m ? (int)f : m - 1) : 0;
}

AD_HD void ad_sample(const double *u, int n, int &i0, int &i1, int &i2) {   // n >= 3
    i0 = ad_pick(u[0], n);
    const int j1 = ad_pick(u[1], n - 1);
    i1 = j1 + (j1 >= i0 ? 1 : 0);
    const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    i2 = ad_pick(u[2], n - 2);
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
}

// ---- the fit (estimateRigidTransform.m + quat2rot.m): x ~ R y + T ---------------------------------------------------------------
// One centred pair's terms of B = sum A^T A, A = [0, (y - x)^T; x - y, [y + x]x]:  with d = y - x, s = y + x
//   B00 = |d|^2,  B0j = (s x d)_j,  Bij = d_i d_j - s_i s_j + delta_ij |s|^2.   S: d d^T (6) | s s^T (6) | s x d (3)
AD_HD void ad_terms(double *S, double x0, double x1, double x2, double y0, double y1, double y2) {
    const double d0 = y0 - x0, d1 = y1 - x1, d2 = y2 - x2, s0 = y0 + x0, s1 = y1 + x1, s2 = y2 + x2;
    S[0] += d0 * d0; S[1] += d0 * d1; S[2] += d0 * d2; S[3] += d1 * d1; S[4] += d1 * d2; S[5] += d2 * d2;
    S[6] += s0 * s0; S[7] += s0 * s1; S[8] += s0 * s2; S[9] += s1 * s1; S[10] += s1 * s2; S[11] += s2 * s2;
    S[12] += s1 * d2 - s2 * d1; S[13] += s2 * d0 - s0 * d2; S[14] += s0 * d1 - s1 * d0;
}

// (x, y) <- (c x - s y, s x + c y)
AD_HD void ad_turn(double &x, double &y, double c, double s) {
    const double x0 = x, y0 = y;
    x = c * x0 - s * y0;
    y = s * x0 + c * y0;
}

// entry (i, j) of the symmetric matrix kept in its upper triangle (constant indices once the loops are unrolled)
#define AD_A(i, j) a[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]

// The unit eigenvector of the smallest eigenvalue of the symmetric 4 x 4 matrix a (upper triangle read and destroyed): the cyclic
// Jacobi of iss_common.h on four rows -- rotations in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), an entry that changes neither
// diagonal neighbour when added to it set to zero without a rotation, until the off-diagonal is exactly zero.  This is the last right
// singular vector estimateRigidTransform.m takes from svd(B): B is symmetric and positive semi-definite.
AD_HD void ad_smallest_eigvec(double (*a)[4], double *q) {
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < AD_SWEEPS; ++sweep) {
        if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[0][3] == 0.0 && a[1][2] == 0.0 && a[1][3] == 0.0 && a[2][3] == 0.0) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                const double apq = a[p][r];
                if (apq == 0.0) continue;
                const double g = fabs(apq);
                if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[r][r]) + g == fabs(a[r][r])) {
                    a[p][r] = 0.0;
                    continue;
                }
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta^2 = inf: t = 0)
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                const double h = t * apq;
                a[p][p] = a[p][p] - h;
                a[r][r] = a[r][r] + h;
                a[p][r] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k != p && k != r) ad_turn(AD_A(k, p), AD_A(k, r), c, s);
                    ad_turn(v[k][p], v[k][r], c, s);
                }
            }
    }
    int best = 0;
    double lam = a[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (a[k][k] < lam) { lam = a[k][k]; best = k; }
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = best == 0 ? v[k][0] : best == 1 ? v[k][1] : best == 2 ? v[k][2] : v[k][3];
}

// rt = (R row-major | T) from the fifteen sums over the centred pairs and the two centroids
AD_HD void ad_solve(const double *S, const double *xc, const double *yc, double *rt) {
    const double trs = S[6] + S[9] + S[11];
    double a[4][4];
    a[0][0] = S[0] + S[3] + S[5]; a[0][1] = S[12]; a[0][2] = S[13]; a[0][3] = S[14];
    a[1][1] = S[0] - S[6] + trs; a[1][2] = S[1] - S[7]; a[1][3] = S[2] - S[8];
    a[2][2] = S[3] - S[9] + trs; a[2][3] = S[4] - S[10];
    a[3][3] = S[5] - S[11] + trs;
    a[1][0] = a[2][0] = a[2][1] = a[3][0] = a[3][1] = a[3][2] = 0.0;   // (never read)
    double q[4];
    ad_smallest_eigvec(a, q);
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];   // quat2rot.m
    rt[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; rt[1] = 2.0 * (q1 * q2 - q0 * q3); rt[2] = 2.0 * (q1 * q3 + q0 * q2);
    rt[3] = 2.0 * (q1 * q2 + q0 * q3); rt[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3; rt[5] = 2.0 * (q2 * q3 - q0 * q1);
    rt[6] = 2.0 * (q1 * q3 - q0 * q2); rt[7] = 2.0 * (q2 * q3 + q0 * q1); rt[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
    rt[9] = xc[0] - (rt[0] * yc[0] + rt[1] * yc[1] + rt[2] * yc[2]);   // T3 T2 T1: x = R (y - yc) + xc
    rt[10] = xc[1] - (rt[3] * yc[0] + rt[4] * yc[1] + rt[5] * yc[2]);
    rt[11] = xc[2] - (rt[6] * yc[0] + rt[7] * yc[1] + rt[8] * yc[2]);
}

// Where the points of a pair are read from: p0 / p1 [axis][AD_THREADS] (the kernel's LDS image, the host twin's copy)
struct AdPoints {
    const double *x, *y;
    AD_HD double X(int axis, int i) const { return x[axis * AD_THREADS + i]; }
    AD_HD double Y(int axis, int i) const { return y[axis * AD_THREADS + i]; }
};

// the fit to the three pairs i0, i1, i2, added in this order
AD_HD void ad_fit3(const AdPoints &P, int i0, int i1, int i2, double *rt) {
    double xc[3], yc[3], S[AD_TERMS];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xc[k] = (P.X(k, i0) + P.X(k, i1) + P.X(k, i2)) / 3.0;
        yc[k] = (P.Y(k, i0) + P.Y(k, i1) + P.Y(k, i2)) / 3.0;
    }
#pragma unroll
    for (int k = 0; k < AD_TERMS; ++k) S[k] = 0.0;
    ad_terms(S, P.X(0, i0) - xc[0], P.X(1, i0) - xc[1], P.X(2, i0) - xc[2], P.Y(0, i0) - yc[0], P.Y(1, i0) - yc[1], P.Y(2, i0) - yc[2]);
    ad_terms(S, P.X(0, i1) - xc[0], P.X(1, i1) - xc[1], P.X(2, i1) - xc[2], P.Y(0, i1) - yc[0], P.Y(1, i1) - yc[1], P.Y(2, i1) - yc[2]);
    ad_terms(S, P.X(0, i2) - xc[0], P.X(1, i2) - xc[1], P.X(2, i2) - xc[2], P.Y(0, i2) - yc[0], P.Y(1, i2) - yc[1], P.Y(2, i2) - yc[2]);
    ad_solve(S, xc, yc, rt);
}

// ---- the inlier test: d = sqrt(sum (x - (R y + T))^2) < t ---------------------------------------------------------------------
// The square root is only taken where the sum lies within 2^-50 of t^2: outside that band the correctly rounded root is on the same
// side of t as the sum is of t^2.
struct AdThreshold {
    double t, lo, hi;
    AD_HD explicit AdThreshold(double t_) : t(t_), lo(t_ * t_ * (1.0 - 0x1p-50)), hi(t_ * t_ * (1.0 + 0x1p-50)) {}
};

AD_HD bool ad_inlier(const double *rt, const AdThreshold &th, double x0, double x1, double x2, double y0, double y1, double y2) {
    const double e0 = x0 - (rt[0] * y0 + rt[1] * y1 + rt[2] * y2 + rt[9]);
    const double e1 = x1 - (rt[3] * y0 + rt[4] * y1 + rt[5] * y2 + rt[10]);
    const double e2 = x2 - (rt[6] * y0 + rt[7] * y1 + rt[8] * y2 + rt[11]);
    const double s = e0 * e0 + e1 * e1 + e2 * e2;
    if (!(th.t > 0.0)) return false;
    if (s < th.lo) return true;
    if (s > th.hi) return false;
    return sqrt(s) < th.t;
}

// ---- the walk (ransac.m:131-229) ----------------------------------------------------------------------------------------------------
struct AdWalk {
    double N;
    int32_t best, best_trial, trials, status;
};

AD_HD void ad_walk_init(AdWalk &w) {
    w.N = 1.0;
    w.best = 0; w.best_trial = -1; w.trials = 0; w.status = 0;
}

AD_HD bool ad_walk_wants(const AdWalk &w) { return w.status == 0 && w.N > (double)w.trials; }   // `while N > trialcount`

// trial w.trials scored `count` of n; true when it is the new best (the caller keeps its model)
AD_HD bool ad_walk_step(AdWalk &w, int count, int n) {
    bool record = false;
    if (count >= w.best) {   // `>=`: among equal counts the later trial wins
        record = true;
        w.best = count;
        w.best_trial = w.trials;
        const double frac = (double)count / (double)n;
        double p_no = 1.0 - frac * frac * frac;
        p_no = p_no > DBL_EPSILON ? p_no : DBL_EPSILON;
        p_no = p_no < 1.0 - DBL_EPSILON ? p_no : 1.0 - DBL_EPSILON;
        const double N = log(1.0 - 0.99) / log(p_no);
        w.N = N > 100.0 ? N : 100.0;
    }
    w.trials += 1;
    if (w.trials > CAELO_ADAPTIVE_MAX_TRIALS) {
        w.trials = CAELO_ADAPTIVE_MAX_TRIALS;
        w.status = 1;
    }
    return record;
}

AD_HD void ad_identity(double *rt) {
#pragma unroll
    for (int k = 0; k < 12; ++k) rt[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
}

AD_HD void ad_store(caelo_adaptive_result *res, const double *rt, const double *rt_ransac, int n, int n_inliers, int trials, int best_trial,
                    int status) {
#pragma unroll
    for (int k = 0; k < 9; ++k) { res->R[k] = rt[k]; res->R_ransac[k] = rt_ransac[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { res->T[k] = rt[9 + k]; res->T_ransac[k] = rt_ransac[9 + k]; }
    res->n_pairs = n; res->n_inliers = n_inliers; res->trials = trials; res->best_trial = best_trial; res->status = status;
    res->reserved = 0;
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------
struct AdArgs {
    caelo_adaptive_table t;     // t.rows null: ONE pair from p0 / p1 [n][3] f64
    const double *p0, *p1;
    int32_t n, mask_len;
};

// v[0:K] summed over the workgroup into tot[0:K] (each wavefront by a butterfly, the wavefronts' rows in ascending order)
template <int K>
__device__ __forceinline__ void ad_block_sum(double *v, double (*red)[AD_TERMS], double *tot, int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < K) {
        double s = red[0][tid];
        for (int w = 1; w < AD_WAVES; ++w) s += red[w][tid];
        tot[tid] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(AD_THREADS) void k_adaptive(const AdArgs a) {
    __shared__ double sx[3 * AD_THREADS], sy[3 * AD_THREADS];   // the pair's points: 48 KB
    __shared__ double smodel[AD_C][12];                         // a chunk's models: 12 KB
    __shared__ double red[AD_WAVES][AD_TERMS], tot[AD_TERMS], sbest[12];
    __shared__ int scount[AD_C];
    __shared__ AdWalk swalk;
    __shared__ int sdone;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t q = blockIdx.x;
    int n;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, y0 = 0.0, y1 = 0.0, y2 = 0.0;
    if (a.t.rows) {
        const int64_t fa = a.t.pairs[2 * q], fb = a.t.pairs[2 * q + 1];   // (checked on the host before any launch, like n_key)
        n = min(max(a.t.n_key[fa], 0), AD_THREADS);
        if (tid < n) {
            const float *pa = a.t.rows + (fa * CAELO_MAX_KEYPTS + tid) * 64 + 60;
            const int64_t j = min(max(a.t.pair_idx[q * CAELO_MAX_KEYPTS + tid], (int64_t)0), (int64_t)(CAELO_MAX_KEYPTS - 1));
            const float *pb = a.t.rows + (fb * CAELO_MAX_KEYPTS + j) * 64 + 60;
            x0 = (double)pa[0]; x1 = (double)pa[1]; x2 = (double)pa[2];
            y0 = (double)pb[0]; y1 = (double)pb[1]; y2 = (double)pb[2];
        }
    } else {
        n = min(max(a.n, 0), AD_THREADS);
        if (tid < n) {
            x0 = a.p0[3 * tid]; x1 = a.p0[3 * tid + 1]; x2 = a.p0[3 * tid + 2];
            y0 = a.p1[3 * tid]; y1 = a.p1[3 * tid + 1]; y2 = a.p1[3 * tid + 2];
        }
    }
    caelo_adaptive_result *res = a.t.result + q;
    uint8_t *mask = a.t.mask + q * (int64_t)a.mask_len;
    const bool valid = tid < n;
    sx[tid] = x0; sx[AD_THREADS + tid] = x1; sx[2 * AD_THREADS + tid] = x2;
    sy[tid] = y0; sy[AD_THREADS + tid] = y1; sy[2 * AD_THREADS + tid] = y2;
    if (tid == 0) {
        ad_walk_init(swalk);
        sdone = 0;
    }
    __syncthreads();
    const AdPoints P = {sx, sy};
    const AdThreshold th(a.t.threshold);
    if (n <= 3) {   // ransacfitRt.m:23-33: nothing to fit, or the direct fit with every pair an inlier
        if (tid == 0) {
            double rt[12];
            if (n == 3) ad_fit3(P, 0, 1, 2, rt); else ad_identity(rt);
            ad_store(res, rt, rt, n, n == 3 ? 3 : 0, 0, -1, n == 3 ? 0 : 2);
        }
        if (tid < a.mask_len) mask[tid] = (n == 3 && valid) ? 1 : 0;
        return;
    }
    for (int base = 0;; base += AD_C) {
        const int c_end = min(AD_C, CAELO_ADAPTIVE_DRAWS - base);   // trials base .. base + c_end - 1 have draws
        if (tid < AD_C) {
            scount[tid] = 0;
            if (tid < c_end) {
                int i0, i1, i2;
                ad_sample(a.t.draws + 3 * (int64_t)(base + tid), n, i0, i1, i2);
                double rt[12];
                ad_fit3(P, i0, i1, i2, rt);
#pragma unroll
                for (int k = 0; k < 12; ++k) smodel[tid][k] = rt[k];
            }
        }
        __syncthreads();
        int mine0 = 0, mine1 = 0;   // this wavefront's counts of trials lane and 64 + lane of the chunk
        for (int c = 0; c < c_end; ++c) {
            const bool in = valid && ad_inlier(smodel[c], th, x0, x1, x2, y0, y1, y2);
            const int cnt = __popcll(__ballot(in));
            if (lane == (c & 63)) {
                if (c < 64) mine0 = cnt; else mine1 = cnt;
            }
        }
        if (mine0) atomicAdd(&scount[lane], mine0);
        if (mine1) atomicAdd(&scount[64 + lane], mine1);
        __syncthreads();
        if (tid == 0) {
            AdWalk w = swalk;
            for (int c = 0; c < c_end && ad_walk_wants(w); ++c)
                if (ad_walk_step(w, scount[c], n))
#pragma unroll
                    for (int k = 0; k < 12; ++k) sbest[k] = smodel[c][k];
            swalk = w;
            sdone = ad_walk_wants(w) ? 0 : 1;
        }
        __syncthreads();
        if (sdone || base + AD_C >= CAELO_ADAPTIVE_DRAWS) break;   // (the walk is over by trial 10 000 whatever it met)
    }
    const AdWalk w = swalk;
    if (w.status != 0) {   // ransac.m:217-226
        if (tid == 0) {
            double rt[12];
            ad_identity(rt);
            ad_store(res, rt, rt, n, 0, w.trials, -1, 1);
        }
        if (tid < a.mask_len) mask[tid] = 0;
        return;
    }
    // the best trial's inliers again, then the least-squares fit to them (ransacfitRt.m:41-50)
    double rb[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) rb[k] = sbest[k];
    const bool in = valid && ad_inlier(rb, th, x0, x1, x2, y0, y1, y2);
    double v[AD_TERMS];
    v[0] = in ? 1.0 : 0.0;
    v[1] = in ? x0 : 0.0; v[2] = in ? x1 : 0.0; v[3] = in ? x2 : 0.0;
    v[4] = in ? y0 : 0.0; v[5] = in ? y1 : 0.0; v[6] = in ? y2 : 0.0;
    ad_block_sum<7>(v, red, tot, tid);
    const int count = (int)tot[0];
    const bool fit = count >= 3;
    double xc[3], yc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xc[k] = fit ? tot[1 + k] / (double)count : 0.0;
        yc[k] = fit ? tot[4 + k] / (double)count : 0.0;
    }
    __syncthreads();   // (tot is written again below)
#pragma unroll
    for (int k = 0; k < AD_TERMS; ++k) v[k] = 0.0;
    if (in) ad_terms(v, x0 - xc[0], x1 - xc[1], x2 - xc[2], y0 - yc[0], y1 - yc[1], y2 - yc[2]);
    ad_block_sum<AD_TERMS>(v, red, tot, tid);
    if (tid == 0) {
        double rt[12], S[AD_TERMS];
#pragma unroll
        for (int k = 0; k < AD_TERMS; ++k) S[k] = tot[k];
        if (fit) ad_solve(S, xc, yc, rt); else ad_identity(rt);
        ad_store(res, rt, rb, n, fit ? count : 0, w.trials, w.best_trial, 0);
    }
    if (tid < a.mask_len) mask[tid] = (fit && in) ? 1 : 0;
}

static int adaptive_launch(const AdArgs &a, int64_t blocks, hipStream_t s) {
    if (blocks == 0) return CAELO_OK;
    hipLaunchKernelGGL(k_adaptive, dim3((unsigned)blocks), dim3(AD_THREADS), 0, s, a);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

int adaptive_table(const caelo_adaptive_table &at, hipStream_t s) {
    AdArgs a = {};
    a.t = at;
    a.mask_len = CAELO_MAX_KEYPTS;
    return adaptive_launch(a, at.n_pairs, s);
}

CAELO_API int caelo_ransac_adaptive(caelo_ctx *c, const double *p0, const double *p1, int64_t n, const double *draws, double threshold,
                                    caelo_adaptive_result *result, uint8_t *mask, void *ws, void *stream) {
    (void)ws;
    CAELO_REQUIRE(c && draws && result, "null argument");
    CAELO_REQUIRE(n >= 0 && n <= CAELO_MAX_KEYPTS, "n must lie in [0, 1024]");
    CAELO_REQUIRE(n == 0 || (p0 && p1 && mask), "null argument");
    CAELO_REQUIRE((((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)draws | (uintptr_t)result) & 7u) == 0, "p0, p1, draws and result must be 8-byte aligned");
    AdArgs a = {};
    a.t.draws = draws; a.t.threshold = threshold; a.t.result = result; a.t.mask = mask; a.t.n_pairs = 1;
    a.p0 = p0; a.p1 = p1; a.n = (int32_t)n; a.mask_len = (int32_t)n;
    return adaptive_launch(a, 1, caelo_stream(stream));
}

// ---- the host twin ----------------------------------------------------------------------------------------------------------------
CAELO_API int caelo_host_ransac_adaptive(const double *p0, const double *p1, int64_t n64, const double *draws, double threshold,
                                         caelo_adaptive_result *result, uint8_t *mask) {
    CAELO_REQUIRE(draws && result, "null argument");
    CAELO_REQUIRE(n64 >= 0 && n64 <= CAELO_MAX_KEYPTS, "n must lie in [0, 1024]");
    CAELO_REQUIRE(n64 == 0 || (p0 && p1 && mask), "null argument");
    const int n = (int)n64;
    static thread_local double hx[3 * AD_THREADS], hy[3 * AD_THREADS];
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { hx[k * AD_THREADS + i] = p0[3 * i + k]; hy[k * AD_THREADS + i] = p1[3 * i + k]; }
    const AdPoints P = {hx, hy};
    const AdThreshold th(threshold);
    double rt[12], rb[12];
    if (n <= 3) {
        if (n == 3) ad_fit3(P, 0, 1, 2, rt); else ad_identity(rt);
        ad_store(result, rt, rt, n, n == 3 ? 3 : 0, 0, -1, n == 3 ? 0 : 2);
        for (int i = 0; i < n; ++i) mask[i] = n == 3 ? 1 : 0;
        return CAELO_OK;
    }
    auto inlier = [&](const double *m, int i) { return ad_inlier(m, th, P.X(0, i), P.X(1, i), P.X(2, i), P.Y(0, i), P.Y(1, i), P.Y(2, i)); };
    AdWalk w;
    ad_walk_init(w);
    ad_identity(rb);
    while (ad_walk_wants(w)) {
        int i0, i1, i2;
        ad_sample(draws + 3 * (int64_t)w.trials, n, i0, i1, i2);
        ad_fit3(P, i0, i1, i2, rt);
        int count = 0;
        for (int i = 0; i < n; ++i) count += inlier(rt, i) ? 1 : 0;
        if (ad_walk_step(w, count, n)) memcpy(rb, rt, sizeof rb);
    }
    if (w.status != 0) {
        ad_identity(rt);
        ad_store(result, rt, rt, n, 0, w.trials, -1, 1);
        memset(mask, 0, (size_t)n);
        return CAELO_OK;
    }
    int count = 0;
    double xc[3] = {0, 0, 0}, yc[3] = {0, 0, 0}, S[AD_TERMS] = {};
    for (int i = 0; i < n; ++i) {
        mask[i] = inlier(rb, i) ? 1 : 0;
        if (mask[i]) {
            ++count;
            for (int k = 0; k < 3; ++k) { xc[k] += P.X(k, i); yc[k] += P.Y(k, i); }
        }
    }
    if (count >= 3) {
        for (int k = 0; k < 3; ++k) { xc[k] = xc[k] / (double)count; yc[k] = yc[k] / (double)count; }
        for (int i = 0; i < n; ++i)
            if (mask[i]) ad_terms(S, P.X(0, i) - xc[0], P.X(1, i) - xc[1], P.X(2, i) - xc[2], P.Y(0, i) - yc[0], P.Y(1, i) - yc[1], P.Y(2, i) - yc[2]);
        ad_solve(S, xc, yc, rt);
    } else {
        ad_identity(rt);
        memset(mask, 0, (size_t)n);
        count = 0;
    }
    ad_store(result, rt, rb, n, count, w.trials, w.best_trial, 0);
    return CAELO_OK;
}
