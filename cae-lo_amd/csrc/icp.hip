// icp.hip -- the re-registration that follows the odometry, device resident.
//
// Reference behaviour restated here (never its code):
//   ICP                      MyICP.py:26-72     point-to-point on the extended key points
//   GetPtsInliners           MyICP.py:75-85     nearest neighbour (sklearn, exact f64 Euclidean) + distance gate
//   GetPlanarPtsInliners     MyICP.py:88-114    the same on planar points, then the foot of the perpendicular onto the
//                                               plane through the frame-1 point (its stored normal) and a second gate
//   ICP_Pt2PtAndPt2Plane     MyICP.py:127-201   both pair sets in one SolveRT per iteration (caller: RefinePoses.py:291-295)
// The whole iteration loop runs on the device: per iteration one nearest-neighbour launch per point set and one
// single-workgroup update (SolveRT over the pairs, move the frame-1 sets, accumulate R_star / T_star in float64, the
// Euler-angle stop rule and the threshold decay of the reference's loop).  Every launch starts by reading a `done`
// word of the state record, so after the loop has ended the remaining launches fall through; the host reads the
// record once.  Round 1 synchronised twice per iteration (Python loop around caelo_icp_step).
// Then caelo_icp_step, one iteration on its own (k_icp_nn, k_icp_fit_apply) with the loop's walk, fit and move; at the end
// caelo_icp_grid, the loop with its nearest neighbours from a cell grid over frame 0 (for extended sets of 10^5 points).
#include "caelo_internal.h"
#include "caelo_rigid.h"

#define ICP_TILE 1024
#define ICP_STATE_BYTES 512  // the state record's share of the workspace

struct IcpState {
    double R_star[9], T_star[3];
    double thr0, thr1;
    int32_t iter;       // iterations completed
    int32_t done;       // the loop has ended
    int32_t success;
    int32_t n_pts, n_planar;  // pairs of the last evaluated iteration
    int32_t cnt_pts, cnt_planar;  // scratch: inlier counters of the iteration in flight
    int32_t pad;
    // ICP_Pt2PtAndPt2Plane from iteration 100 on (:151-153): the pair count and the fifteen sums over the planar pairs of
    // iteration 99.  Both arrays of those pairs are fitted again as they were then, so their sums are all that is needed
    double stale[RIGID_TERMS];
};
static_assert(sizeof(IcpState) <= ICP_STATE_BYTES, "the state record outgrew its share of the workspace");

// The brute-force walk of both nearest-neighbour kernels, by a whole 256-thread workgroup: set 0 (stride ld0, n0 points) passes
// through the LDS tile and every thread returns the index of the point nearest to its query q, `best` the squared distance.
// Exact f64 distance, first minimum, like sklearn's kd-tree on these inputs.
__device__ inline int icp_nn_walk(const float *__restrict__ p0, int ld0, int n0, double qx, double qy, double qz, float *tile,
                                  double &best) {
    const int tid = threadIdx.x;
    double b = 1.0e300;
    int bi = 0;
    for (int base = 0; base < n0; base += ICP_TILE) {
        const int m = min(ICP_TILE, n0 - base);
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const float *s = p0 + (size_t)ld0 * (base + i);
            tile[3 * i] = s[0]; tile[3 * i + 1] = s[1]; tile[3 * i + 2] = s[2];
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {  // all lanes read the same address: LDS broadcast
            const double dx = (double)tile[3 * i] - qx, dy = (double)tile[3 * i + 1] - qy, dz = (double)tile[3 * i + 2] - qz;
            const double d2 = dx * dx + dy * dy + dz * dz;  // sequential x, y, z like the kd-tree's reduced distance
            if (d2 < b) { b = d2; bi = base + i; }
        }
    }
    best = b;  // (updated through the reference inside the loop, the minimum was kept twice there: caelo_icp 8 % slower)
    return bi;
}

// nearest neighbour in set 0 (stride ld0) of every point of set 1 (stride ld1); pairs closer than the threshold of the
// state record (which = 0: thr0, 1: thr1).
__global__ void __launch_bounds__(256) k_icp_nn2(const float *__restrict__ p0, int ld0, int n0, const float *__restrict__ p1, int ld1, int n1,
                                                 IcpState *st, int which, int64_t *__restrict__ idx0, uint8_t *__restrict__ mask) {
    if (st->done || (which && st->iter >= 100)) return;  // from iteration 100 on the planar pairs are not searched again (:151-153)
    __shared__ float tile[ICP_TILE * 3];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const double thr = which ? st->thr1 : st->thr0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (j < n1) { qx = p1[(size_t)ld1 * j]; qy = p1[(size_t)ld1 * j + 1]; qz = p1[(size_t)ld1 * j + 2]; }
    double best;
    const int besti = icp_nn_walk(p0, ld0, n0, qx, qy, qz, tile, best);
    if (j < n1) {
        idx0[j] = besti;
        mask[j] = (n0 > 0 && sqrt(best) < thr) ? 1 : 0;  // distances < inlierThreshold (:80, :100)
    }
}

// planar pair of frame-1 planar point j (MyICP.py:103-113): returns false when it is gated out
__device__ inline bool planar_pair(const float *pn0, const float *pn1, const int64_t *idx0, const uint8_t *mask, int j, double thr0,
                                   float pedal[3], float in1[3]) {
    if (!mask[j]) return false;
    const float *a = pn0 + 6 * (size_t)idx0[j];  // inliers0 (xyz of the frame-0 neighbour)
    const float *b = pn1 + 6 * (size_t)j;        // inliers1 | norms1
    const float v0 = __fsub_rn(a[0], b[0]), v1 = __fsub_rn(a[1], b[1]), v2 = __fsub_rn(a[2], b[2]);                    // :104
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(b[3], v0), __fmul_rn(b[4], v1)), __fmul_rn(b[5], v2));              // :105
    pedal[0] = __fadd_rn(b[0], __fmul_rn(b[3], d)); pedal[1] = __fadd_rn(b[1], __fmul_rn(b[4], d)); pedal[2] = __fadd_rn(b[2], __fmul_rn(b[5], d));  // :106
    const float e0 = __fsub_rn(pedal[0], b[0]), e1 = __fsub_rn(pedal[1], b[1]), e2 = __fsub_rn(pedal[2], b[2]);
    const float dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(e0, e0), __fmul_rn(e1, e1)), __fmul_rn(e2, e2)));          // :108
    in1[0] = b[0]; in1[1] = b[1]; in1[2] = b[2];
    return (double)dist < thr0;                                                                                         // :109
}

struct IcpParams {
    int32_t max_iter, min_iter, min_pairs, fail_only_first;  // fail_only_first: too few pairs is a failure only at iteration 0 (:166-169)
    double decay0, decay1, small_shift, ep;
    int32_t planar;  // the planar sets take part
    int32_t pad;
};

__global__ void __launch_bounds__(256) k_icp_update(const float *__restrict__ pc0, float *__restrict__ pc1, int n1, const int64_t *__restrict__ idx_p,
                                                    const uint8_t *__restrict__ mask_p, const float *__restrict__ pn0, float *__restrict__ pn1, int m1,
                                                    const int64_t *__restrict__ idx_q, const uint8_t *__restrict__ mask_q, IcpState *st, IcpParams prm) {
    if (st->done) return;
    __shared__ double red[4][RIGID_TERMS], red_n[4][2];
    __shared__ float s_rt[12];
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const double thr0 = st->thr0;
    // :147-153: from iteration 100 on ICP_Pt2PtAndPt2Plane fits neither the point pairs nor new planar pairs but the planar
    // pairs of iteration 99, pedals and frame-1 points as they were then (the reference's maxIterTimes = 50 never gets
    // there; ICP has no such branch)
    const int iter0 = st->iter;
    const bool stale = prm.planar && iter0 >= 100;
    const int lane = tid & 63, wave = tid >> 6;
    RigidSums sums;
    double n_pts = 0.0, n_planar = 0.0;  // point pairs (counted from iteration 100 on as well) and planar pairs of this iteration
    if (prm.planar && iter0 == 99) {  // the planar pairs on their own, kept for the iterations that follow
        for (int j = tid; j < m1; j += 256) {
            float pedal[3], in1[3];
            if (!planar_pair(pn0, pn1, idx_q, mask_q, j, thr0, pedal, in1)) continue;
            sums.add(pedal[0], pedal[1], pedal[2], in1[0], in1[1], in1[2]);
        }
        sums.reduce_wave(red, lane, wave);
        sums = RigidSums();
        __syncthreads();
        if (tid < RIGID_TERMS) st->stale[tid] = RigidSums::combine(red, 4, tid);
        __syncthreads();
    }
    for (int i = tid; i < n1; i += 256) {
        if (!mask_p[i]) continue;
        n_pts += 1.0;
        if (stale) continue;
        const float *u = pc0 + 3 * (size_t)idx_p[i], *v = pc1 + 3 * (size_t)i;
        sums.add(u[0], u[1], u[2], v[0], v[1], v[2]);
    }
    if (prm.planar && !stale) {
        for (int j = tid; j < m1; j += 256) {
            float pedal[3], in1[3];
            if (!planar_pair(pn0, pn1, idx_q, mask_q, j, thr0, pedal, in1)) continue;
            n_planar += 1.0;
            sums.add(pedal[0], pedal[1], pedal[2], in1[0], in1[1], in1[2]);
        }
    }
    sums.reduce_wave(red, lane, wave);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n_pts += __shfl_xor(n_pts, o); n_planar += __shfl_xor(n_planar, o); }
    if (lane == 0) { red_n[wave][0] = n_pts; red_n[wave][1] = n_planar; }
    __syncthreads();
    if (tid == 0) {
        double s[RIGID_TERMS];
        for (int t = 0; t < RIGID_TERMS; ++t) s[t] = RigidSums::combine(red, 4, t);
        if (stale)  // the count that the reference goes on printing is the one of iteration 99 as well (:199)
            for (int t = 0; t < RIGID_TERMS; ++t) s[t] = st->stale[t];
        st->n_pts = (int)(red_n[0][0] + red_n[1][0] + red_n[2][0] + red_n[3][0]);
        st->n_planar = (int)(stale ? s[0] : red_n[0][1] + red_n[1][1] + red_n[2][1] + red_n[3][1]);
        const int pairs = (int)s[0];
        int stop = 0;
        if (pairs < prm.min_pairs) {  // ICP :38-40 / Pt2Plane :166-169
            if (!prm.fail_only_first || st->iter < 1) st->success = 0;
            stop = 1;
        } else {
            float R[9], T[3];
            rigid_from_sums(s, R, T);
            for (int i = 0; i < 9; ++i) s_rt[i] = R[i];
            for (int i = 0; i < 3; ++i) s_rt[9 + i] = T[i];
            // R_star = R R_star, T_star = R T_star + T in float64 (:50-51)
            double Rn[9], Tn[3];
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j)
                    Rn[3 * i + j] = (double)R[3 * i] * st->R_star[j] + (double)R[3 * i + 1] * st->R_star[3 + j] + (double)R[3 * i + 2] * st->R_star[6 + j];
                Tn[i] = (double)R[3 * i] * st->T_star[0] + (double)R[3 * i + 1] * st->T_star[1] + (double)R[3 * i + 2] * st->T_star[2] + (double)T[i];
            }
            for (int i = 0; i < 9; ++i) st->R_star[i] = Rn[i];
            for (int i = 0; i < 3; ++i) st->T_star[i] = Tn[i];
            // stop rule and threshold decay (:54-65): Euler angles in degrees (Transformations.py:181-186), norm of T in float32
            const double r2d = 180.0 / 3.14159265358979323846;
            const double e0 = atan2((double)R[7], (double)R[8]) * r2d;
            const double e1 = atan2(-(double)R[6], sqrt((double)R[7] * (double)R[7] + (double)R[8] * (double)R[8])) * r2d;
            const double e2 = atan2((double)R[3], (double)R[0]) * r2d;
            const double normE = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            const double normT = (double)sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(T[0], T[0]), __fmul_rn(T[1], T[1])), __fmul_rn(T[2], T[2])));
            const int it = st->iter;
            if (it >= prm.min_iter && normE < prm.ep && normT < prm.ep) stop = 2;  // converged: this iteration's move still applies
            else if (normE < prm.small_shift && normT < prm.small_shift) { st->thr0 *= prm.decay0; st->thr1 *= prm.decay1; }
            st->iter = it + 1;
            if (it + 1 >= prm.max_iter) stop = stop ? stop : 2;
        }
        s_stop = stop;
        if (stop) st->done = 1;
    }
    __syncthreads();
    if (s_stop == 1) return;  // too few pairs: nothing is moved
    rigid_move(pc1, 3, n1, s_rt);                   // :49
    if (prm.planar) rigid_move(pn1, 6, m1, s_rt);   // the planar points move, their normals do not (:177)
}

__global__ void k_icp_init(IcpState *st, double thr0, double thr1) {
    for (int i = 0; i < 9; ++i) st->R_star[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) st->T_star[i] = 0.0;
    st->thr0 = thr0; st->thr1 = thr1;
    st->iter = 0; st->done = 0; st->success = 1; st->n_pts = 0; st->n_planar = 0;
}

__global__ void k_icp_result(const IcpState *st, caelo_icp_result *out) {
    for (int i = 0; i < 9; ++i) out->R_star[i] = st->R_star[i];
    for (int i = 0; i < 3; ++i) out->T_star[i] = st->T_star[i];
    out->threshold0 = st->thr0; out->threshold1 = st->thr1;
    out->iterations = st->iter; out->success = st->success; out->n_inliers_pts = st->n_pts; out->n_inliers_planar = st->n_planar;
}

CAELO_API int64_t caelo_icp_loop_ws_bytes(int64_t n1, int64_t m1) {
    return ICP_STATE_BYTES + ((n1 + m1) * 9 + 255) / 256 * 256 + 256;
}

CAELO_API int caelo_icp(caelo_ctx *c, const float *pc0, int64_t n0, float *pc1, int64_t n1, const float *planar0, int64_t m0,
                        float *planar1, int64_t m1, const caelo_icp_params *prm, caelo_icp_result *result, void *ws, void *stream) {
    CAELO_REQUIRE(c && pc0 && pc1 && prm && result && ws, "null argument");
    CAELO_REQUIRE(n0 > 0 && n1 > 0 && n0 < (1 << 30) && n1 < (1 << 30), "bad shape");
    const bool planar = prm->use_planar != 0;
    if (planar) {
        // sklearn's NearestNeighbors.fit refuses an empty set (MyICP.py:94): the reference raises ValueError -- and
        // GetKeyPtsByAE always returns an empty PlanarPts (SphericalRing.py:219,285)
        CAELO_REQUIRE(planar0 && planar1 && m0 > 0 && m1 > 0, "Found array with 0 sample(s) while a minimum of 1 is required (planar points)");
        CAELO_REQUIRE(m0 < (1 << 30) && m1 < (1 << 30), "bad shape");
    }
    CAELO_REQUIRE(prm->max_iter >= 1 && prm->max_iter <= 1000, "max_iter must be in [1, 1000]");
    hipStream_t s = caelo_stream(stream);
    IcpState *st = (IcpState *)ws;
    int64_t *idx_p = (int64_t *)((char *)ws + ICP_STATE_BYTES);
    int64_t *idx_q = idx_p + n1;
    uint8_t *mask_p = (uint8_t *)(idx_q + (planar ? m1 : 0));
    uint8_t *mask_q = mask_p + n1;
    IcpParams kp;
    kp.max_iter = prm->max_iter; kp.min_iter = prm->min_iter; kp.min_pairs = prm->min_pairs; kp.fail_only_first = prm->fail_only_first;
    kp.decay0 = prm->decay0; kp.decay1 = prm->decay1; kp.small_shift = prm->small_shift; kp.ep = prm->ep;
    kp.planar = planar ? 1 : 0; kp.pad = 0;
    k_icp_init<<<1, 1, 0, s>>>(st, prm->threshold0, prm->threshold1);
    CAELO_LAUNCH_CHECK();
    for (int it = 0; it < prm->max_iter; ++it) {
        k_icp_nn2<<<(unsigned)((n1 + 255) / 256), 256, 0, s>>>(pc0, 3, (int)n0, pc1, 3, (int)n1, st, 0, idx_p, mask_p);
        CAELO_LAUNCH_CHECK();
        if (planar) {
            k_icp_nn2<<<(unsigned)((m1 + 255) / 256), 256, 0, s>>>(planar0, 6, (int)m0, planar1, 6, (int)m1, st, 1, idx_q, mask_q);
            CAELO_LAUNCH_CHECK();
        }
        k_icp_update<<<1, 256, 0, s>>>(pc0, pc1, (int)n1, idx_p, mask_p, planar0, planar1, planar ? (int)m1 : 0, idx_q, mask_q, st, kp);
        CAELO_LAUNCH_CHECK();
    }
    k_icp_result<<<1, 1, 0, s>>>(st, result);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

// ------------------------------------------------------------------------------------------------
// ICP step: MyICP.py:26-72 / :75-85 -- the refinement that follows the odometry
// ------------------------------------------------------------------------------------------------
// One iteration of the reference's point-to-point ICP: for every point of PC1 its nearest neighbour in PC0
// (sklearn NearestNeighbors(n_neighbors=1): exact Euclidean distance in float64), the pairs closer than the
// threshold, SolveRT on them, PC1 <- R PC1 + T.  The iteration control (threshold decay, Euler-angle stop rule)
// stays on the host, like the reference's Python loop.
__global__ void __launch_bounds__(256) k_icp_nn(const float *__restrict__ pc0, int n0, const float *__restrict__ pc1, int n1,
                                                double thr, int64_t *__restrict__ idx0, uint8_t *__restrict__ mask,
                                                int32_t *__restrict__ n_in) {
    __shared__ float tile[ICP_TILE * 3];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int j = blockIdx.x * blockDim.x + tid;
    if (tid == 0) s_cnt = 0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (j < n1) { qx = pc1[3 * (size_t)j]; qy = pc1[3 * (size_t)j + 1]; qz = pc1[3 * (size_t)j + 2]; }
    double best;
    const int besti = icp_nn_walk(pc0, 3, n0, qx, qy, qz, tile, best);
    const bool in = j < n1 && sqrt(best) < thr;  // GetPtsInliners: distances < inlierThreshold (:80)
    if (j < n1) { idx0[j] = besti; mask[j] = in ? 1 : 0; }
    const unsigned long long bal = __ballot(in);
    if ((tid & 63) == 0 && bal) atomicAdd(&s_cnt, __popcll(bal));
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(n_in, s_cnt);
}

// SolveRT on the inlier pairs and PC1 <- R PC1 + T (one workgroup; float32 like the reference's arrays)
__global__ void __launch_bounds__(256) k_icp_fit_apply(const float *__restrict__ pc0, float *__restrict__ pc1, int n1,
                                                       const int64_t *__restrict__ idx0, const uint8_t *__restrict__ mask,
                                                       const int32_t *__restrict__ n_in, int min_inliers, float *__restrict__ rt) {
    if (*n_in < min_inliers) return;  // the host stops the iteration (MyICP.py:38-40)
    __shared__ double red[4][RIGID_TERMS];
    const int tid = threadIdx.x;
    RigidSums sums;
    for (int i = tid; i < n1; i += 256) {  // (k_icp_update's walk over the point pairs)
        if (!mask[i]) continue;
        const float *u = pc0 + 3 * (size_t)idx0[i], *v = pc1 + 3 * (size_t)i;
        sums.add(u[0], u[1], u[2], v[0], v[1], v[2]);
    }
    sums.reduce_wave(red, tid & 63, tid >> 6);
    __syncthreads();
    if (tid == 0) {
        double s[RIGID_TERMS];
        for (int t = 0; t < RIGID_TERMS; ++t) s[t] = RigidSums::combine(red, 4, t);
        if (s[0] >= 1.0) rigid_from_sums(s, rt, rt + 9);  // (min_inliers <= 0 and no pair: rt stays the caller's)
    }
    __syncthreads();
    rigid_move(pc1, 3, n1, rt);  // :50
}

CAELO_API int64_t caelo_icp_ws_bytes(int64_t n1) { return ((n1 * 9 + 255) / 256) * 256 + 256; }

CAELO_API int caelo_icp_step(caelo_ctx *c, const float *pc0, int64_t n0, float *pc1, int64_t n1, double threshold,
                             int min_inliers, float *rt, int32_t *n_inliers, void *ws, void *stream) {
    CAELO_REQUIRE(c && pc0 && pc1 && rt && n_inliers && ws, "null argument");
    CAELO_REQUIRE(n0 > 0 && n1 > 0 && n0 < (1 << 30) && n1 < (1 << 30), "bad shape");
    hipStream_t s = caelo_stream(stream);
    int64_t *idx0 = (int64_t *)ws;
    uint8_t *mask = (uint8_t *)(idx0 + n1);
    CAELO_HIP(hipMemsetAsync(n_inliers, 0, sizeof(int32_t), s));
    k_icp_nn<<<(unsigned)((n1 + 255) / 256), 256, 0, s>>>(pc0, (int)n0, pc1, (int)n1, threshold, idx0, mask, n_inliers);
    CAELO_LAUNCH_CHECK();
    k_icp_fit_apply<<<1, 256, 0, s>>>(pc0, pc1, (int)n1, idx0, mask, n_inliers, min_inliers, rt);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

// ------------------------------------------------------------------------------------------------
// caelo_icp_grid: the same loop with the nearest-neighbour search over a cell grid
// ------------------------------------------------------------------------------------------------
// Frame 0 never moves during a call and the thresholds only decay, so its points are binned ONCE per call into cubic cells whose
// edge is the smallest power of two not below the call's initial threshold; every iteration a frame-1 point looks at the 3 x 3 x 3
// cells around its own.  A pair closer than the threshold differs by less than one cell edge per axis, hence by at most one cell
// index; the cell index floor(x / edge) - origin is exact in float64 (a power-of-two scaling, a floor, an integer difference) and
// the clamp to the grid's box is monotone and 1-Lipschitz, so it keeps "at most one".  The distance expression, its type and order
// and the gate are icp_nn_walk's / k_icp_nn2's; the minimum is kept by (squared distance, original index), which is what the
// all-pairs walk's strict < over ascending indices keeps.  Where the gate fails idx0 is 0 or the nearest of the neighbourhood, not
// the global nearest: nothing reads idx0 behind a zero mask (k_icp_update, planar_pair).
#include <new>
#include <vector>

#define GRID_CELLS_PTS (1 << 22)     // most cells of the grid over pc0 (a 160 m x 160 m x 32 m box at 0.5 m cells is 3.3 M)
#define GRID_CELLS_PLANAR (1 << 18)  // ... over planar0 (8 m cells at the reference's 5.0 m threshold)
#define GRID_SCAN_CHUNK 2048         // cells per workgroup of the scan: 256 threads x 8

struct IcpGrid {
    double inv;         // 1 / cell edge, a power of two
    double ox, oy, oz;  // the box's first cell per axis, in cells (integers held in doubles)
    int32_t nx, ny, nz, ncell;
};

__host__ __device__ inline int grid_axis(float x, double inv, double o, int n) {
    return (int)fmin(fmax(floor((double)x * inv) - o, 0.0), (double)(n - 1));
}
__host__ __device__ inline int grid_cell(const IcpGrid &g, float x, float y, float z) {
    return (grid_axis(z, g.inv, g.oz, g.nz) * g.ny + grid_axis(y, g.inv, g.oy, g.ny)) * g.nx + grid_axis(x, g.inv, g.ox, g.nx);
}

__global__ void __launch_bounds__(256) k_grid_count(const float *__restrict__ p0, int ld0, int n0, IcpGrid g, int *__restrict__ cursor) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n0) return;
    const float *s = p0 + (size_t)ld0 * i;
    atomicAdd(&cursor[grid_cell(g, s[0], s[1], s[2])], 1);
}

// exclusive prefix of cnt inside each chunk of GRID_SCAN_CHUNK cells -> start, the chunk's total -> bsum[chunk].  (cnt and start may
// be the same array: a thread reads its eight cells before it writes them.)
__global__ void __launch_bounds__(256) k_grid_scan_chunks(const int *cnt, int *start, int *bsum, int ncell) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * GRID_SCAN_CHUNK + tid * 8;
    int v[8], s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = base + k < ncell ? cnt[base + k] : 0; s += v[k]; }
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    int run = off + inc - s;
#pragma unroll
    for (int k = 0; k < 8; ++k) { if (base + k < ncell) start[base + k] = run; run += v[k]; }
    if (tid == 255 && bsum) bsum[blockIdx.x] = off + inc;
}

__global__ void __launch_bounds__(256) k_grid_scan_add(int *__restrict__ start, const int *__restrict__ bsum, int ncell, int n0) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncell) start[c] += bsum[c / GRID_SCAN_CHUNK];
    if (c == 0) start[ncell] = n0;
}

// (point, original index) in cell order; the order inside a cell is whatever the atomics give and the query does not depend on it.
// cursor holds the counts and is back at zero afterwards
__global__ void __launch_bounds__(256) k_grid_scatter(const float *__restrict__ p0, int ld0, int n0, IcpGrid g, const int *__restrict__ start,
                                                      int *__restrict__ cursor, int4 *__restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n0) return;
    const float *s = p0 + (size_t)ld0 * i;
    const int c = grid_cell(g, s[0], s[1], s[2]);
    const int pos = start[c] + atomicSub(&cursor[c], 1) - 1;
    sorted[pos] = make_int4(__float_as_int(s[0]), __float_as_int(s[1]), __float_as_int(s[2]), i);
}

// k_icp_nn2 over the grid: a thread per frame-1 point, nine runs of up to three x-adjacent cells each (x is the fastest cell index,
// so such a run is one contiguous range of `sorted`).  The ranges are read straight from global memory: neighbouring threads hold
// unrelated queries, so there is no tile a workgroup could share, and the whole table (16 bytes a point) stays in L2.
__global__ void __launch_bounds__(256) k_icp_nn_grid(const int4 *__restrict__ sorted, const int *__restrict__ start, IcpGrid g,
                                                     const float *__restrict__ p1, int ld1, int n1, IcpState *st, int which,
                                                     int64_t *__restrict__ idx0, uint8_t *__restrict__ mask) {
    if (st->done || (which && st->iter >= 100)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n1) return;
    const double thr = which ? st->thr1 : st->thr0;
    const float *q = p1 + (size_t)ld1 * j;
    const double qx = q[0], qy = q[1], qz = q[2];
    const int cx = grid_axis(q[0], g.inv, g.ox, g.nx), cy = grid_axis(q[1], g.inv, g.oy, g.ny), cz = grid_axis(q[2], g.inv, g.oz, g.nz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    double b = 1.0e300;
    int bi = 0x7fffffff;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
            const int row = (z * g.ny + y) * g.nx;
            const int hi = start[row + x1 + 1];
            for (int e = start[row + x0]; e < hi; ++e) {
                const int4 s = sorted[e];
                const double dx = (double)__int_as_float(s.x) - qx, dy = (double)__int_as_float(s.y) - qy, dz = (double)__int_as_float(s.z) - qz;
                const double d2 = dx * dx + dy * dy + dz * dz;  // icp_nn_walk's expression
                if (d2 < b || (d2 == b && s.w < bi)) { b = d2; bi = s.w; }
            }
        }
    const bool found = bi != 0x7fffffff;
    idx0[j] = found ? bi : 0;
    mask[j] = (found && sqrt(b) < thr) ? 1 : 0;
}

// the coordinates of a device array on the host: all finite?  and their range, in cells
static bool grid_scan_host(const std::vector<float> &h, int ld, int64_t n, double inv, double lo[3], double hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = 1.0e300; hi[a] = -1.0e300; }
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float x = h[(size_t)ld * i + a];
            if (!(x - x == 0.0f)) return false;  // NaN or infinite
            const double c = floor((double)x * inv);
            lo[a] = c < lo[a] ? c : lo[a];
            hi[a] = c > hi[a] ? c : hi[a];
        }
    return true;
}

// the grid over a set whose points span cells lo .. hi: that box, shrunk about its middle along its longest axis until it has at
// most `cap` cells (points outside land in the edge cells)
static IcpGrid grid_make(double edge, const double lo[3], const double hi[3], int64_t cap) {
    double o[3], n[3];
    for (int a = 0; a < 3; ++a) {
        o[a] = lo[a] < -1.0e12 ? -1.0e12 : lo[a];
        const double top = hi[a] > 1.0e12 ? 1.0e12 : hi[a];
        n[a] = top - o[a] + 1.0;
        if (n[a] > 1048576.0) { o[a] += floor((n[a] - 1048576.0) / 2.0); n[a] = 1048576.0; }
    }
    while (n[0] * n[1] * n[2] > (double)cap) {
        const int a = n[0] >= n[1] && n[0] >= n[2] ? 0 : (n[1] >= n[2] ? 1 : 2);
        const double m = ceil(n[a] / 2.0);
        o[a] += floor((n[a] - m) / 2.0);
        n[a] = m;
    }
    IcpGrid g;
    g.inv = 1.0 / edge; g.ox = o[0]; g.oy = o[1]; g.oz = o[2];
    g.nx = (int)n[0]; g.ny = (int)n[1]; g.nz = (int)n[2]; g.ncell = g.nx * g.ny * g.nz;
    return g;
}

// smallest power of two not below a positive finite threshold
static double grid_edge(double thr) {
    int e;
    const double m = frexp(thr, &e);  // thr = m 2^e, m in [0.5, 1)
    return ldexp(1.0, m == 0.5 ? e - 1 : e);
}

static int64_t grid_align(int64_t b) { return (b + 255) / 256 * 256; }

CAELO_API int caelo_icp_grid_ws_layout(int64_t n0, int64_t n1, int64_t m0, int64_t m1, int64_t out[8]) {
    CAELO_REQUIRE(out && n0 > 0 && n1 > 0 && m0 >= 0 && m1 >= 0 && n0 < (1 << 30) && n1 < (1 << 30) && m0 < (1 << 30) && m1 < (1 << 30),
                  "bad argument");
    int64_t o = grid_align(caelo_icp_loop_ws_bytes(n1, m1));
    out[0] = o; o += grid_align(((int64_t)GRID_CELLS_PTS + 1) * 4);     // start of the cells of pc0
    out[1] = o; o += grid_align((int64_t)GRID_CELLS_PTS * 4);           // their counters
    out[2] = o; o += grid_align(n0 * 16);                               // pc0 in cell order: x, y, z, index
    out[3] = o; o += grid_align(((int64_t)GRID_CELLS_PLANAR + 1) * 4);  // the same three for planar0
    out[4] = o; o += grid_align((int64_t)GRID_CELLS_PLANAR * 4);
    out[5] = o; o += grid_align(m0 * 16);
    out[6] = o; o += grid_align((int64_t)(GRID_CELLS_PTS / GRID_SCAN_CHUNK) * 4);  // chunk totals of the scan
    out[7] = o;                                                         // bytes in all
    return CAELO_OK;
}

static int grid_build(const float *p0, int ld0, int64_t n0, const IcpGrid &g, int *start, int *cursor, int4 *sorted, int *bsum, hipStream_t s) {
    const unsigned nb = (unsigned)((n0 + 255) / 256), chunks = (unsigned)((g.ncell + GRID_SCAN_CHUNK - 1) / GRID_SCAN_CHUNK);
    CAELO_HIP(hipMemsetAsync(cursor, 0, (size_t)g.ncell * 4, s));
    k_grid_count<<<nb, 256, 0, s>>>(p0, ld0, (int)n0, g, cursor);
    CAELO_LAUNCH_CHECK();
    k_grid_scan_chunks<<<chunks, 256, 0, s>>>(cursor, start, bsum, g.ncell);
    CAELO_LAUNCH_CHECK();
    k_grid_scan_chunks<<<1, 256, 0, s>>>(bsum, bsum, nullptr, (int)chunks);  // chunks <= GRID_SCAN_CHUNK: one workgroup
    CAELO_LAUNCH_CHECK();
    k_grid_scan_add<<<(unsigned)((g.ncell + 255) / 256), 256, 0, s>>>(start, bsum, g.ncell, (int)n0);
    CAELO_LAUNCH_CHECK();
    k_grid_scatter<<<nb, 256, 0, s>>>(p0, ld0, (int)n0, g, start, cursor, sorted);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

CAELO_API int caelo_icp_grid(caelo_ctx *c, const float *pc0, int64_t n0, float *pc1, int64_t n1, const float *planar0, int64_t m0,
                             float *planar1, int64_t m1, const caelo_icp_params *prm, caelo_icp_result *result, void *ws, void *stream) {
    static_assert(GRID_CELLS_PTS / GRID_SCAN_CHUNK <= GRID_SCAN_CHUNK && GRID_CELLS_PLANAR <= GRID_CELLS_PTS, "the chunk totals are scanned by one workgroup");
    CAELO_REQUIRE(c && pc0 && pc1 && prm && result && ws, "null argument");
    CAELO_REQUIRE(((uintptr_t)ws & 15) == 0, "ws must be 16-byte aligned");  // the (x, y, z, index) tables are read as int4
    CAELO_REQUIRE(n0 > 0 && n1 > 0 && n0 < (1 << 30) && n1 < (1 << 30), "bad shape");
    const bool planar = prm->use_planar != 0;
    if (planar) {
        CAELO_REQUIRE(planar0 && planar1 && m0 > 0 && m1 > 0, "Found array with 0 sample(s) while a minimum of 1 is required (planar points)");
        CAELO_REQUIRE(m0 < (1 << 30) && m1 < (1 << 30), "bad shape");
    }
    CAELO_REQUIRE(prm->max_iter >= 1 && prm->max_iter <= 1000, "max_iter must be in [1, 1000]");
    // a grid built for the initial thresholds answers for every later one only if they never grow
    CAELO_REQUIRE(prm->decay0 > 0.0 && prm->decay0 <= 1.0 && (!planar || (prm->decay1 > 0.0 && prm->decay1 <= 1.0)), "decay must be in (0, 1]: the thresholds must not grow");
    CAELO_REQUIRE(prm->threshold0 > 0.0 && prm->threshold0 < 1.0e30 && (!planar || (prm->threshold1 > 0.0 && prm->threshold1 < 1.0e30)),
                  "thresholds must be positive and finite");
    hipStream_t s = caelo_stream(stream);
    // the coordinates are looked at on the host before anything is launched: non-finite ones are refused, frame 0's range places the box
    const double edge_p = grid_edge(prm->threshold0), edge_q = planar ? grid_edge(prm->threshold1) : 1.0;
    std::vector<float> h0, h1, g0, g1;
    try {  // (an allocation failure must not leave through the C ABI)
        h0.resize((size_t)n0 * 3); h1.resize((size_t)n1 * 3);
        if (planar) { g0.resize((size_t)m0 * 6); g1.resize((size_t)m1 * 6); }
    } catch (const std::bad_alloc &) {
        caelo_set_error("%s: no host memory for the coordinate check", __func__);
        return CAELO_ERR_CAPACITY;
    }
    CAELO_HIP(hipMemcpyAsync(h0.data(), pc0, h0.size() * 4, hipMemcpyDeviceToHost, s));
    CAELO_HIP(hipMemcpyAsync(h1.data(), pc1, h1.size() * 4, hipMemcpyDeviceToHost, s));
    if (planar) {
        CAELO_HIP(hipMemcpyAsync(g0.data(), planar0, g0.size() * 4, hipMemcpyDeviceToHost, s));
        CAELO_HIP(hipMemcpyAsync(g1.data(), planar1, g1.size() * 4, hipMemcpyDeviceToHost, s));
    }
    CAELO_HIP(hipStreamSynchronize(s));
    double lo_p[3], hi_p[3], lo_q[3], hi_q[3], lo_x[3], hi_x[3];
    bool finite = grid_scan_host(h0, 3, n0, 1.0 / edge_p, lo_p, hi_p) && grid_scan_host(h1, 3, n1, 1.0 / edge_p, lo_x, hi_x);
    if (planar) finite = finite && grid_scan_host(g0, 6, m0, 1.0 / edge_q, lo_q, hi_q) && grid_scan_host(g1, 6, m1, 1.0 / edge_q, lo_x, hi_x);
    CAELO_REQUIRE(finite, "non-finite coordinate");
    const IcpGrid gp = grid_make(edge_p, lo_p, hi_p, GRID_CELLS_PTS);
    const IcpGrid gq = planar ? grid_make(edge_q, lo_q, hi_q, GRID_CELLS_PLANAR) : gp;

    int64_t lay[8];
    if (caelo_icp_grid_ws_layout(n0, n1, planar ? m0 : 0, planar ? m1 : 0, lay) != CAELO_OK) return CAELO_ERR_ARG;
    char *w = (char *)ws;
    IcpState *st = (IcpState *)ws;
    int64_t *idx_p = (int64_t *)(w + ICP_STATE_BYTES);
    int64_t *idx_q = idx_p + n1;
    uint8_t *mask_p = (uint8_t *)(idx_q + (planar ? m1 : 0));
    uint8_t *mask_q = mask_p + n1;
    int *start_p = (int *)(w + lay[0]), *cursor_p = (int *)(w + lay[1]), *start_q = (int *)(w + lay[3]), *cursor_q = (int *)(w + lay[4]);
    int4 *sorted_p = (int4 *)(w + lay[2]), *sorted_q = (int4 *)(w + lay[5]);
    int *bsum = (int *)(w + lay[6]);
    IcpParams kp;
    kp.max_iter = prm->max_iter; kp.min_iter = prm->min_iter; kp.min_pairs = prm->min_pairs; kp.fail_only_first = prm->fail_only_first;
    kp.decay0 = prm->decay0; kp.decay1 = prm->decay1; kp.small_shift = prm->small_shift; kp.ep = prm->ep;
    kp.planar = planar ? 1 : 0; kp.pad = 0;
    k_icp_init<<<1, 1, 0, s>>>(st, prm->threshold0, prm->threshold1);
    CAELO_LAUNCH_CHECK();
    if (grid_build(pc0, 3, n0, gp, start_p, cursor_p, sorted_p, bsum, s) != CAELO_OK) return CAELO_ERR_HIP;
    if (planar && grid_build(planar0, 6, m0, gq, start_q, cursor_q, sorted_q, bsum, s) != CAELO_OK) return CAELO_ERR_HIP;
    for (int it = 0; it < prm->max_iter; ++it) {
        k_icp_nn_grid<<<(unsigned)((n1 + 255) / 256), 256, 0, s>>>(sorted_p, start_p, gp, pc1, 3, (int)n1, st, 0, idx_p, mask_p);
        CAELO_LAUNCH_CHECK();
        if (planar) {
            k_icp_nn_grid<<<(unsigned)((m1 + 255) / 256), 256, 0, s>>>(sorted_q, start_q, gq, planar1, 6, (int)m1, st, 1, idx_q, mask_q);
            CAELO_LAUNCH_CHECK();
        }
        k_icp_update<<<1, 256, 0, s>>>(pc0, pc1, (int)n1, idx_p, mask_p, planar0, planar1, planar ? (int)m1 : 0, idx_q, mask_q, st, kp);
        CAELO_LAUNCH_CHECK();
    }
    k_icp_result<<<1, 1, 0, s>>>(st, result);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
