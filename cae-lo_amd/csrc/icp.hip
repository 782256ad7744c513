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
// At the end: caelo_icp_step, one iteration on its own (k_icp_nn, k_icp_fit_apply) with the loop's walk, fit and move.
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
