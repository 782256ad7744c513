// ransac.hip -- the pose of a frame pair from its matched key points: rigid fit, RANSAC scoring, inlier refit.
//
// Reference behaviour restated here (never its code):
//   SolveRT              Match.py:138-158   Kabsch via 3x3 SVD, reflection quirk at :151-155
//   RANSAC4RT            Match.py:162-218   4-point samples with replacement, 100..500 trials,
//                                            threshold escalation 0.4 -> 0.8 -> 1.6
//   SolveRelativePose    Match.py:260-283   inlier refit
//
// The reference draws from NumPy's global RNG inside the loop; here the caller hands over the uniform doubles in
// consumption order (3 levels x 500 trials x 4).  Up to three launches per set of pairs; what crosses
// workgroups crosses a launch (the note above RE_WAVES says why no workgroup finishes for the others):
//   k_ransac_hyp      the first level's 500 hypotheses scored in parallel, and the certificate's bounds (certify.hip)
//   k_ransac_hyp_up   only for pairs that leave a certificate and whose first level failed: the upper levels' bounds
//   k_ransac_finish   one workgroup per pair replays the sequential accept / early-exit rules over the counts as a
//                     prefix maximum (verified equivalent on the reference: SURVEY 8a-9), evaluates a next level
//                     itself if the level failed, writes the inlier mask and refits over the inliers
#include "caelo_internal.h"
#include "caelo_rigid.h"

// residual of Match.py:191-192 in f32
__device__ inline float residual(const float *R, const float *T, float ax, float ay, float az, float bx, float by, float bz) {
    const float px = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], bx), __fmul_rn(R[1], by)), __fmul_rn(R[2], bz)), T[0]);
    const float py = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3], bx), __fmul_rn(R[4], by)), __fmul_rn(R[5], bz)), T[1]);
    const float pz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[6], bx), __fmul_rn(R[7], by)), __fmul_rn(R[8], bz)), T[2]);
    const float dx = __fsub_rn(ax, px), dy = __fsub_rn(ay, py), dz = __fsub_rn(az, pz);
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

// SolveRT over n pairs (p0[i], p1[i]) by one workgroup (RigidSums, caelo_rigid.h)
__global__ void __launch_bounds__(256) k_solve_rt(const float *p0, const float *p1, int n, float *R, float *T, int *credible) {
    __shared__ double red[4][RIGID_TERMS];
    const int tid = threadIdx.x;
    RigidSums sums;
    for (int i = tid; i < n; i += 256) {
        const float *u = p0 + 3 * (size_t)i, *v = p1 + 3 * (size_t)i;
        sums.add(u[0], u[1], u[2], v[0], v[1], v[2]);
    }
    sums.reduce_wave(red, tid & 63, tid >> 6);
    __syncthreads();
    if (tid == 0) {
        double s[RIGID_TERMS];
        for (int t = 0; t < RIGID_TERMS; ++t) s[t] = RigidSums::combine(red, 4, t);
        const int cred = rigid_from_sums(s, R, T);
        if (credible) *credible = cred;
    }
}

CAELO_API int caelo_solve_rt(caelo_ctx *c, const float *p0, const float *p1, int64_t n, float *R, float *T,
                             int32_t *credible, void *stream) {
    CAELO_REQUIRE(c && p0 && p1 && R && T && n > 0, "bad argument");
    k_solve_rt<<<1, 256, 0, caelo_stream(stream)>>>(p0, p1, (int)n, R, T, credible);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

// ------------------------------------------------------------------------------------------------
// RANSAC
// ------------------------------------------------------------------------------------------------
// workspace of one pair: the inlier counts of the 500 hypotheses of the level being replayed.  Written by one kernel,
// read by the next (k_ransac_hyp -> k_ransac_finish) or inside one workgroup: nothing to initialise, nothing to clean.
struct RansacWs {
    int32_t counts[CAELO_RANSAC_MAX_TRIALS];
};

CAELO_API int64_t caelo_ransac_ws_bytes(void) { return (int64_t)sizeof(RansacWs); }

struct RansacVerdict {
    int iterations, success, best_trial;  // best_trial within the level, -1 = none accepted
};

// sequential accept / exit rules of Match.py:166-169,:181,:195-214 replayed over the counts (one wave:
// the counts are staged in LDS, lane 0 walks them)
__device__ __forceinline__ void ransac_replay(int N, const int32_t *counts, RansacVerdict *out, const int *preloaded = nullptr) {
    // The loop of :181-206 keeps the running maximum of the admissible counts (strict >: the FIRST
    // occurrence wins) and stops at the first iteration it >= 100 whose running maximum reached
    // 0.25 N, or at 500.  Restated as a prefix-max scan so one wavefront does it in parallel:
    //   M[i]  = max(c'[0..i]),  c'[i] = counts[i] if counts[i] >= leastInliers else 0
    //   it*   = 1 + min{ i >= 99 : M[i] >= 0.25 N }   (500 if none)
    //   best  = min{ j < it* : c'[j] == M[it*-1] }    (none if M[it*-1] == 0 -> the level failed)
    const int lane = threadIdx.x;
    const int least = (100 < (int)(0.2 * N)) ? 100 : (int)(0.2 * N);  // :166
    const double min_success = 0.25 * N;                              // :167
    const int PER = (CAELO_RANSAC_MAX_TRIALS + 63) / 64;              // 8 consecutive trials per lane
    int c[(CAELO_RANSAC_MAX_TRIALS + 63) / 64], pm[(CAELO_RANSAC_MAX_TRIALS + 63) / 64];
    int run = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = lane * PER + q;
        int v = preloaded ? preloaded[q] : (i < CAELO_RANSAC_MAX_TRIALS ? counts[i] : 0);
        v = v >= least ? v : 0;
        c[q] = v;
        run = run > v ? run : v;
        pm[q] = run;
    }
    // exclusive prefix max of the lane maxima
    int incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl = incl > up ? incl : up;
    }
    int excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 0;
    int stop = CAELO_RANSAC_MAX_TRIALS;  // it*
#pragma unroll
    for (int q = PER - 1; q >= 0; --q) {
        const int i = lane * PER + q;
        pm[q] = pm[q] > excl ? pm[q] : excl;
        if (i >= 99 && i < CAELO_RANSAC_MAX_TRIALS && (double)pm[q] >= min_success) stop = i + 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(stop, o); stop = stop < t ? stop : t; }
    // running maximum after `stop` iterations = M[stop-1]
    int target = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q)
        if (lane * PER + q == stop - 1) target = pm[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(target, o); target = target > t ? target : t; }
    int best = 0x7FFFFFFF;
#pragma unroll
    for (int q = PER - 1; q >= 0; --q) {
        const int i = lane * PER + q;
        if (i < stop && target > 0 && c[q] == target) best = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(best, o); best = best < t ? best : t; }
    if (lane != 0) return;
    // leastInliers == 0 (N < 5) admits every hypothesis.  N == 0 -- a frame without a single key point, where the reference's
    // sampling raises IndexError (Match.py:182-187) -- is reported as a failed pose, not as a success over nothing.
    const int success = N > 0 && ((target > 0) || (least <= 0));
    out->iterations = stop;
    out->success = success;
    out->best_trial = (success && target > 0) ? best : -1;  // N < 5: success without any accepted hypothesis -> identity (:177)
}

// the four sampled pairs of a hypothesis as SolveRT sees them (Match.py:141-146; means / centring in f32 like np.mean on
// f32 rows, covariance in f64).  Kept for the certificate's bound alone: sample_hypothesis repeats these statements, see there
struct Sample4 {
    double m0[3], m1[3], H[9];
    float c0[4][3], c1[4][3];
    int idx[4];
};
__device__ inline void sample4(const float *P0, int l0, const int64_t *pidx, const float *P1, int l1, int N, const double *r4, Sample4 &s) {
    float s0[4][3], s1[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = (int)(r4[q] * (double)N);  // :182-184 idx = int32(u * N), with replacement
        s.idx[q] = idx;
        const float *a = P0 + (size_t)l0 * (pidx ? pidx[idx] : idx);
        const float *b = P1 + (size_t)l1 * idx;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s0[q][c] = a[c]; s1[q][c] = b[c]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float mm0 = __fdiv_rn(__fadd_rn(__fadd_rn(__fadd_rn(s0[0][a], s0[1][a]), s0[2][a]), s0[3][a]), 4.0f);
        const float mm1 = __fdiv_rn(__fadd_rn(__fadd_rn(__fadd_rn(s1[0][a], s1[1][a]), s1[2][a]), s1[3][a]), 4.0f);
        s.m0[a] = mm0; s.m1[a] = mm1;
#pragma unroll
        for (int q = 0; q < 4; ++q) { s.c0[q][a] = __fsub_rn(s0[q][a], mm0); s.c1[q][a] = __fsub_rn(s1[q][a], mm1); }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double h = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) h += (double)s.c1[q][i] * (double)s.c0[q][j];
            s.H[3 * i + j] = h;
        }
}

// hypothesis from 4 sampled pairs (SolveRT on the sample, Match.py:141-157)
// The same arithmetic as sample4 followed by rigid_from_H<false>(s.H, s.m0, s.m1, R, T), written out on purpose: through a Sample4
// the compiler keeps the whole record live and k_ransac_hyp goes from 168 to 208 registers (wave_hypotheses says what leaving 168
// costs), k_ransac_finish from 160 to 176 bytes of scratch.  sample4 stays the certificate's.
__device__ inline void sample_hypothesis(const float *P0, int l0, const int64_t *pidx, const float *P1, int l1, int N,
                                         const double *r4, float R[9], float T[3]) {
    float s0[4][3], s1[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = (int)(r4[q] * (double)N);  // :182-184 idx = int32(u * N), with replacement
        const float *a = P0 + (size_t)l0 * (pidx ? pidx[idx] : idx);
        const float *b = P1 + (size_t)l1 * idx;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s0[q][c] = a[c]; s1[q][c] = b[c]; }
    }
    double m0[3], m1[3], H[9];
    float c0[4][3], c1[4][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float mm0 = __fdiv_rn(__fadd_rn(__fadd_rn(__fadd_rn(s0[0][a], s0[1][a]), s0[2][a]), s0[3][a]), 4.0f);
        const float mm1 = __fdiv_rn(__fadd_rn(__fadd_rn(__fadd_rn(s1[0][a], s1[1][a]), s1[2][a]), s1[3][a]), 4.0f);
        m0[a] = mm0; m1[a] = mm1;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c0[q][a] = __fsub_rn(s0[q][a], mm0); c1[q][a] = __fsub_rn(s1[q][a], mm1); }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double h = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) h += (double)c1[q][i] * (double)c0[q][j];
            H[3 * i + j] = h;
        }
    rigid_from_H<false>(H, m0, m1, R, T);   // (hypotheses: see rigid_from_H_jacobi)
}

// ---- how far the reference's own arithmetic can move a residual of this hypothesis (the certificate of caelo.h) ----------
// The reference forms H = P1^T P0 in float32 through its BLAS (rounding error <= ~4 eps32 sum |c1||c0| per entry, order and
// fusing unknown), takes the float64 SVD of THAT matrix, rounds U and Vh to float32, multiplies R and T in float32 and
// evaluates the residuals in float32 (Match.py:146-157,:190-192); this kernel fits the exact float64 covariance of the same
// centred float32 points.  The rotation of a Kabsch fit moves by at most 2 |dH| / (s2 + s3) under a perturbation dH of the
// covariance, so with kappa = s1 / s2 the two poses differ by O(eps32 (1 + kappa)) in R, and the residual of pair j by at most
//     band_j = CB eps32 [ (1 + kappa) |p1_j - mean1| + |p0_j| + |p1_j| + |T| ],      CB = 16
// (measured over 54 000 samples of the golden pairs against NumPy: the largest ratio residual difference / bracket is 3.5,
// the 99.9th percentile 2.7; CB = 16 leaves a factor 4.5.  The constant is CALIBRATED, not proven, so the bound is checked wherever
// a true count is known: tools/parity_soak.py compares every hypothesis count of the oracle's first-level loops with `hi`
// (profiles/r0x_parity_soak*.txt: 0 violations in > 400 k counts), and the host half compares every count it evaluates with its
// bound and, on a violation, decides the pair without bounds and counts the event -- caelo_host_bound_violations, certify.hip).
// kappa is bounded from the
// invariants I1 = |H|_F^2, I2 = |cof H|_F^2: kappa <= sqrt(2) I1 / sqrt(I2).  |p1_j - mean1| <= |p1_j| + |mean1|.  So
//     residual_ref_j < thr   ==>   residual_j < thr + a + b |p1_j| + g |p0_j|,   g = CB eps32, b = g (2 + kappa),
//                                                                                a = g ((2 + kappa) |mean1| + |mean0|)   (|T| <= |mean0| + |mean1|)
// and the number of pairs passing the right-hand test is an upper bound `hi` on the reference's inlier count.
// kind 1 -- the sign of det H is not safe against the float32 rounding of H (|det| <= 64 eps32 sum |cof_ij| A_ij: a sample with
// a repeated point, four coplanar points): the reference's SVD picks the third singular vectors' signs, its pose is one of the
// two of rigid_two_candidates; both are scored and the larger bound is kept.  kind 2 -- rank <= 1: no bound (hi = N).
// Evaluated BEFORE the pose is derived, so that nothing of the sample but (a, b, kind) stays live across the residual pass.
#define RB_G 9.5367431640625e-7f  // CB eps32 = 16 * 2^-24
struct HypBound {
    float a, b;
    int kind;
};
__device__ inline void hypothesis_bound(const Sample4 &s, HypBound &hb) {
    const double *H = s.H;
    const double C0 = H[4] * H[8] - H[5] * H[7], C1 = H[5] * H[6] - H[3] * H[8], C2 = H[3] * H[7] - H[4] * H[6];
    const double C3 = H[2] * H[7] - H[1] * H[8], C4 = H[0] * H[8] - H[2] * H[6], C5 = H[1] * H[6] - H[0] * H[7];
    const double C6 = H[1] * H[5] - H[2] * H[4], C7 = H[2] * H[3] - H[0] * H[5], C8 = H[0] * H[4] - H[1] * H[3];
    const double det = H[0] * C0 + H[1] * C1 + H[2] * C2;
    double I1 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) I1 += H[i] * H[i];
    const double I2 = C0 * C0 + C1 * C1 + C2 * C2 + C3 * C3 + C4 * C4 + C5 * C5 + C6 * C6 + C7 * C7 + C8 * C8;
    // sum |cof_ij| A_ij, A_ij = sum_q |c1_qi| |c0_qj|: what a relative rounding error of every product can do to det H
    float sumCA = 0.f;
    const float aC[9] = {(float)fabs(C0), (float)fabs(C1), (float)fabs(C2), (float)fabs(C3), (float)fabs(C4), (float)fabs(C5), (float)fabs(C6), (float)fabs(C7), (float)fabs(C8)};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) t += fabsf(s.c1[q][i]) * fabsf(s.c0[q][j]);
            sumCA += aC[3 * i + j] * t;
        }
    hb.kind = 0;
    hb.a = 0.f;
    hb.b = 0.f;
    if (!(I2 > 1e-10 * I1 * I1) || !(I1 > 0.0)) { hb.kind = 2; return; }
    const double kappa = 1.41421356237309515 * I1 / sqrt(I2);
    if (fabs(det) <= 64.0 * 5.9604644775390625e-8 * 1.001 * (double)sumCA) hb.kind = 1;
    // ... nor against the float64 SVD's own backward error (|E| ~ 1e2 eps64 |H|: det moves by <= |cof H|_F |E|_F) when the four points are
    // coplanar to a part in 1e12 -- key points on the ground plane of a mm-quantised scan (round 6, tests/golden/ransac_bound_case.npz)
    if (det * det <= 1e-24 * I1 * I2) hb.kind = 1;   // |det| <= 1e-12 |H|_F |cof H|_F
    const double nm0 = sqrt(s.m0[0] * s.m0[0] + s.m0[1] * s.m0[1] + s.m0[2] * s.m0[2]);
    const double nm1 = sqrt(s.m1[0] * s.m1[0] + s.m1[1] * s.m1[1] + s.m1[2] * s.m1[2]);
    // |T|_inf <= |mean0| + |R mean1| = |mean0| + |mean1| for every candidate pose (T = mean0 - R mean1, Match.py:157)
    // (rounded up: the float conversions and the float evaluation of the test are covered by the 1.0001)
    hb.a = (float)(1.0001 * (double)RB_G * ((2.0 + kappa) * nm1 + nm0));
    hb.b = (float)(1.0001 * (double)RB_G * (2.0 + kappa));
}

// Two launches per set of pairs (a third between them, k_ransac_hyp_up below, when a pair leaves a certificate).
//   k_ransac_hyp     the 500 hypotheses of the first threshold level (0.4 m), sixteen per wavefront, 64 per workgroup:
//                    the matched pairs (P0[pair_idx[i]], P1[i]) are gathered once per workgroup into LDS (coalesced;
//                    the residual loop then never touches global memory), Kabsch on the 4-samples (one hypothesis
//                    per group of four lanes), residuals of four poses per pass, ballot + popcount -> counts[trial].
//   k_ransac_finish  one workgroup per pair: replays the sequential accept / early-exit rules over the counts
//                    (Match.py:181-206) as a prefix maximum; if the level failed (no hypothesis reached leastInliers,
//                    :207-214) it evaluates the next level's 500 hypotheses itself, sixteen per wavefront on eight
//                    wavefronts (150 us per level; one per wavefront on four took 1.2 ms, which a pipeline felt) -- up to 1.6 m; then the winner's pose, the inlier mask (:193-194), the inlier count
//                    and the refit over all inliers (:273-282).
// Everything that crosses workgroups crosses a kernel boundary.  Round 1 finished inside the last workgroup of a
// per-level launch (tickets, a `finished` flag, a self-cleaning workspace) and evaluated the mask from the pairs that
// workgroup had staged in LDS; under concurrent streams ~1 call in 3 000 then stored 64-element runs of constant 0 / 1
// from some of its wavefronts although the inlier COUNT summed from the same registers was right (tools/stress_mask.py:
// sentinel-filled buffer, D2H cross-check, exactly one replay per call counted) -- the "3 of 41 suite runs" of round 1.
// The hand-off protocol was not involved.  This structure shows 0 mismatches in 72 000 frames.
#define RE_WAVES 4
#define RE_LDS_PAIRS 1024

// Every lane of a wavefront derives the same hypothesis from the same four pairs; lanes that disagree mean the hardware
// mis-executed something (with packed-f32 instructions enabled, gfx950 sporadically drops the subtrahend of
// one `v_pk_add_f32 ... op_sel:[0,1]` in lanes 48-63 when three queues are busy -- the library is built without them).
// The check costs a dozen v_readfirstlane per hypothesis and turns a silent wrong inlier count into a counter that
// caelo_lane_faults() reports and the tests and bench.py assert to be zero.
__device__ inline void lane_agreement(const float R[9], const float T[3], int lane, int32_t *faults) {
    if (!faults) return;
    unsigned int diff = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) diff |= __float_as_uint(R[q]) ^ (unsigned int)__builtin_amdgcn_readfirstlane((int)__float_as_uint(R[q]));
#pragma unroll
    for (int q = 0; q < 3; ++q) diff |= __float_as_uint(T[q]) ^ (unsigned int)__builtin_amdgcn_readfirstlane((int)__float_as_uint(T[q]));
    if (__ballot(diff != 0) != 0ull && lane == 0) atomicAdd(faults, 1);
}

// inlier count of one hypothesis by one wavefront (every lane returns it)
__device__ inline int hypothesis_count(const float *P0, int l0, const int64_t *pidx, const float *P1, int l1, int N, const double *r4,
                                       float thr, int lane, int32_t *faults) {
    float R[9], T[3];
    sample_hypothesis(P0, l0, pidx, P1, l1, N, r4, R, T);
    lane_agreement(R, T, lane, faults);
    int cnt = 0;  // residuals + inlier count (:191-194): ballot + popcount per 64 pairs
    for (int i = lane; i < ((N + 63) & ~63); i += 64) {
        bool in = false;
        if (i < N) {
            const float *a = P0 + (size_t)l0 * (pidx ? pidx[i] : i);
            const float *b = P1 + (size_t)l1 * i;
            in = residual(R, T, a[0], a[1], a[2], b[0], b[1], b[2]) < thr;
        }
        cnt += __popcll(__ballot(in));
    }
    return cnt;
}

// One wavefront = PW hypotheses, PW = 16 or 4: lane l derives hypothesis l & (PW - 1) (the Kabsch step is a long serial f64 chain
// that costs the same for 1 or 64 lanes -- about 20 us of a launch, against 4 us for a pass over 1 024 pairs; the 64 / PW lanes
// that share a hypothesis must agree -- the hardware self-check).  Then PW / RH_PER_PASS scoring passes: each broadcasts four poses
// through scalar registers (the scalar register budget holds no more) and counts the inliers of all four in ONE walk over the
// staged pairs (a pair is read from LDS once per pass).  Lane l < PW collects the count (and bound) of hypothesis l and stores it.
// Sixteen per wavefront is a quarter of the wavefronts, each holding its 168 registers for the same chain and three more passes:
// what a batch of pairs inside the pipeline launches.  Four per wavefront is one pass behind the chain: the shortest
// launch, for a call of fewer than RH_WIDE_FROM pairs, which waits for it.  Round 2: one hypothesis per wavefront, 35 us per 8 pairs.
// `rnd`: the draws of the level (trial t at rnd + 4 t); counts[trial0 .. trial0 + PW - 1] are written.
#define RH_WIDE 16
#define RH_NARROW 4
#define RH_WIDE_FROM 4   // pairs per call from which the hypothesis kernels score RH_WIDE per wavefront (measured at one pair and at eight only: nothing in between)
#define RH_PER_PASS 4
#define RH_BLOCKS(PW) ((CAELO_RANSAC_MAX_TRIALS + RE_WAVES * (PW) - 1) / (RE_WAVES * (PW)))   // workgroups per level and pair: 8 or 32, one round
// CERT: also the certificate's bound (sN: per pair (|p1_j|, g |p0_j|); cert: the record `hi` / `idx` of the trials go to)
template <bool CERT, int PW>
__device__ __forceinline__ void wave_hypotheses(const float *sP0, const float *sP1, int N, const double *rnd, int trial0, float thr, int lane,
                                       int32_t *faults, int32_t *counts, const float2 *sN = nullptr, caelo_ransac_cert *cert = nullptr,
                                       int level = 0) {
    // (__forceinline__: with a second caller -- k_ransac_hyp_up -- hipcc stopped inlining this function, and a CALL costs the callers
    // the full register budget: k_ransac_hyp went from 168 to 248 registers, no longer fitted beside two stage-1 workgroups, and its
    // launch stretched from 74 to 199 us inside the pipeline, profiles/r06_kernel_stats_bench.txt)
    // ---- lane l: hypothesis trial0 + (l & (PW - 1)) (a trial past the last repeats the last one; its count is not stored)
    const int mine = min(trial0 + (lane & (PW - 1)), CAELO_RANSAC_MAX_TRIALS - 1);
    const bool stores = lane < PW && trial0 + lane < CAELO_RANSAC_MAX_TRIALS;   // lane l < PW keeps hypothesis l's results
    float R[9], T[3];
    HypBound hb = {0.f, 0.f, 0};
    if (CERT) {
        Sample4 smp;
        sample4(sP0, 3, nullptr, sP1, 3, N, rnd + (size_t)mine * 4, smp);
        hypothesis_bound(smp, hb);
        if (stores)
#pragma unroll
            for (int q = 0; q < 4; ++q) (level ? cert->idx_up[level - 1] : cert->idx)[trial0 + lane][q] = smp.idx[q];
        rigid_from_H<false>(smp.H, smp.m0, smp.m1, R, T);   // (a rank-2 sample is kind 1: both poses are scored below)
    } else {
        sample_hypothesis(sP0, 3, nullptr, sP1, 3, N, rnd + (size_t)mine * 4, R, T);
    }
    if (faults) {  // the 64 / PW lanes of a hypothesis hold the same pose, bit for bit
        unsigned int hsh = 0;
#pragma unroll
        for (int q = 0; q < 9; ++q) hsh = hsh * 0x9E3779B1u + __float_as_uint(R[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) hsh = hsh * 0x9E3779B1u + __float_as_uint(T[q]);
        bool bad = false;
#pragma unroll
        for (int o = PW; o < 64; o <<= 1) bad = bad || hsh != (unsigned int)__shfl_xor((int)hsh, o);
        if (__ballot(bad) != 0ull && lane == 0) atomicAdd(faults, 1);
    }
    int my_cnt = 0, my_hi = 0;
    // ---- PW / 4 passes: the poses of lanes l0 .. l0 + 3 in scalar registers, one walk over the pairs each
#pragma unroll 1
    for (int l0 = 0; l0 < PW && trial0 + l0 < CAELO_RANSAC_MAX_TRIALS; l0 += RH_PER_PASS) {   // (wave-uniform: a pass of trials past the last stores nothing)
        float Rs[RH_PER_PASS][9], Ts[RH_PER_PASS][3];
#pragma unroll
        for (int h = 0; h < RH_PER_PASS; ++h) {
#pragma unroll
            for (int q = 0; q < 9; ++q) Rs[h][q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(R[q]), l0 + h));
#pragma unroll
            for (int q = 0; q < 3; ++q) Ts[h][q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T[q]), l0 + h));
        }
        int cnt[RH_PER_PASS] = {0, 0, 0, 0};
        const int hh = lane - l0;   // 0 .. 3: the lane that keeps hypothesis l0 + hh
        if (!CERT) {
            for (int i = lane; i < ((N + 63) & ~63); i += 64) {
                const bool live = i < N;
                const int ii = live ? i : 0;
                const float ax = sP0[3 * ii], ay = sP0[3 * ii + 1], az = sP0[3 * ii + 2];
                const float bx = sP1[3 * ii], by = sP1[3 * ii + 1], bz = sP1[3 * ii + 2];
#pragma unroll
                for (int h = 0; h < RH_PER_PASS; ++h) {
                    const bool in = live && residual(Rs[h], Ts[h], ax, ay, az, bx, by, bz) < thr;
                    cnt[h] += __popcll(__ballot(in));
                }
            }
        } else {
            // ---- the same pass with the certificate's second test (hypothesis_bound)
            float as[RH_PER_PASS], bs[RH_PER_PASS];
#pragma unroll
            for (int h = 0; h < RH_PER_PASS; ++h) {
                as[h] = thr + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hb.a), l0 + h));
                bs[h] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hb.b), l0 + h));
            }
            int hi[RH_PER_PASS] = {0, 0, 0, 0};
            for (int i = lane; i < ((N + 63) & ~63); i += 64) {
                const bool live = i < N;
                const int ii = live ? i : 0;
                const float ax = sP0[3 * ii], ay = sP0[3 * ii + 1], az = sP0[3 * ii + 2];
                const float bx = sP1[3 * ii], by = sP1[3 * ii + 1], bz = sP1[3 * ii + 2];
                const float2 nn = sN[ii];
#pragma unroll
                for (int h = 0; h < RH_PER_PASS; ++h) {
                    const float r = residual(Rs[h], Ts[h], ax, ay, az, bx, by, bz);
                    cnt[h] += __popcll(__ballot(live && r < thr));
                    hi[h] += __popcll(__ballot(live && r < as[h] + fmaf(bs[h], nn.x, nn.y)));
                }
            }
            if (hh >= 0 && hh < RH_PER_PASS) my_hi = hh == 0 ? hi[0] : (hh == 1 ? hi[1] : (hh == 2 ? hi[2] : hi[3]));
        }
        if (hh >= 0 && hh < RH_PER_PASS) my_cnt = hh == 0 ? cnt[0] : (hh == 1 ? cnt[1] : (hh == 2 ? cnt[2] : cnt[3]));
    }
    if (CERT) {
        // ---- rank-2 samples (kind 1) get their two candidate poses scored as well, rank-1 samples (kind 2) no bound
        if (__ballot(stores && hb.kind == 1) != 0ull) {  // wave-uniform: some hypothesis of this wavefront has two candidate poses
            // (derived again from the sample: cheaper than carrying 24 more registers through the passes every wavefront runs)
            float Ra[9], Ta[3], Rb[9], Tb[3];
            bool two;
            {
                Sample4 smp;
                sample4(sP0, 3, nullptr, sP1, 3, N, rnd + (size_t)mine * 4, smp);
                two = rigid_two_candidates(smp.H, smp.m0, smp.m1, Ra, Ta, Rb, Tb);
            }
#pragma unroll 1
            for (int h = 0; h < PW && trial0 + h < CAELO_RANSAC_MAX_TRIALS; ++h) {
                if (__builtin_amdgcn_readlane(hb.kind, h) != 1) continue;  // (scalar condition)
                int ha = N;
                if (__builtin_amdgcn_readlane((int)two, h)) {
                    const float as = thr + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hb.a), h));
                    const float bs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hb.b), h));
                    float Ras[9], Tas[3], Rbs[9], Tbs[3];
#pragma unroll
                    for (int q = 0; q < 9; ++q) {
                        Ras[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Ra[q]), h));
                        Rbs[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Rb[q]), h));
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        Tas[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Ta[q]), h));
                        Tbs[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Tb[q]), h));
                    }
                    int na = 0, nb = 0;
                    for (int i = lane; i < ((N + 63) & ~63); i += 64) {
                        const bool live = i < N;
                        const int ii = live ? i : 0;
                        const float ax = sP0[3 * ii], ay = sP0[3 * ii + 1], az = sP0[3 * ii + 2];
                        const float bx = sP1[3 * ii], by = sP1[3 * ii + 1], bz = sP1[3 * ii + 2];
                        const float2 nn = sN[ii];
                        const float lim = as + fmaf(bs, nn.x, nn.y);
                        na += __popcll(__ballot(live && residual(Ras, Tas, ax, ay, az, bx, by, bz) < lim));
                        nb += __popcll(__ballot(live && residual(Rbs, Tbs, ax, ay, az, bx, by, bz) < lim));
                    }
                    ha = max(na, nb);
                }
                if (lane == h) my_hi = max(my_hi, ha);
            }
        }
        if (hb.kind == 2) my_hi = N;
        if (stores) (level ? cert->hi_up[level - 1] : cert->hi)[trial0 + lane] = my_hi;
    }
    if (stores) counts[trial0 + lane] = my_cnt;
}

template <int PW>
static __device__ __forceinline__ void ransac_hyp_body(const caelo_pair_set &ps, int ld0, int ld1, int64_t k1_max) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    const float *__restrict__ pc0 = P.pc0, *__restrict__ pc1 = P.pc1;
    const int64_t *__restrict__ pair_idx = P.pair_idx;
    RansacWs *ws = (RansacWs *)P.ws_ransac;
    __shared__ float sP0[RE_LDS_PAIRS * 3], sP1[RE_LDS_PAIRS * 3];
    __shared__ float2 sN[RE_LDS_PAIRS];  // certificate: (|p1_j|, g |p0_j|) of hypothesis_bound
    caelo_ransac_cert *cert = P.cert;
    // no pairs at all when EITHER frame has no key point (frame 0 empty: the match kernel wrote index 0 everywhere, the
    // reference's argmin over an empty axis raises): the pose fails as a value
    const int N = (P.n0 && *P.n0 <= 0) ? 0 : (P.n1 ? min(max(*P.n1, 0), (int)k1_max) : (int)k1_max);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // pairs -> LDS (falls back to the global arrays when they do not fit)
    const bool in_lds = N <= RE_LDS_PAIRS;
    if (in_lds) {
        for (int i = tid; i < N; i += 64 * RE_WAVES) {
            const float *a = pc0 + (size_t)ld0 * pair_idx[i];
            const float *b = pc1 + (size_t)ld1 * i;
            const float a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
            sP0[3 * i] = a0; sP0[3 * i + 1] = a1; sP0[3 * i + 2] = a2;
            sP1[3 * i] = b0; sP1[3 * i + 1] = b1; sP1[3 * i + 2] = b2;
            if (cert) sN[i] = make_float2(1.0001f * sqrtf(b0 * b0 + b1 * b1 + b2 * b2), 1.0001f * RB_G * sqrtf(a0 * a0 + a1 * a1 + a2 * a2));
        }
    }
    __syncthreads();
    if (cert && blockIdx.x == 0 && tid == 0) cert->levels_up = 0;   // (k_ransac_hyp_up, the next launch, sets it when it writes the higher levels' bounds)
    if (cert && P.cert_only && blockIdx.x == 0) {
        // the host half takes the pair from here (caelo_pipeline with result_host): the certificate's pairs and header leave with
        // this launch and k_ransac_finish is not launched at all -- what it computes (the kernels' own winner, mask and refit) is
        // exactly what the host half replaces
        if (in_lds) {
            float *d0 = &cert->p0[0][0], *d1 = &cert->p1[0][0];
            for (int i = tid; i < 3 * N; i += 64 * RE_WAVES) { d0[i] = sP0[i]; d1[i] = sP1[i]; }
        }
        if (tid == 0) {
            cert->n_pairs = N;
            cert->flags = in_lds ? 0 : CAELO_CERT_NO_BOUNDS;
            cert->magic = CAELO_CERT_MAGIC;
        }
    }
    const int trial0 = (blockIdx.x * RE_WAVES + wave) * PW;  // wave-uniform
    if (trial0 >= CAELO_RANSAC_MAX_TRIALS) return;
    if (!in_lds) {  // more pairs than the LDS stage holds: one hypothesis at a time from global memory (a wavefront walks its PW trials
                    // serially: at sixteen four times as many on a quarter of the wavefronts -- the same counts, never timed)
        for (int h = 0; h < PW && trial0 + h < CAELO_RANSAC_MAX_TRIALS; ++h) {
            const int cnt = hypothesis_count(pc0, ld0, pair_idx, pc1, ld1, N, P.rand + (size_t)(trial0 + h) * 4, 0.4f, lane, ps.faults);
            if (lane == 0) ws->counts[trial0 + h] = cnt;
        }
        return;
    }
    if (cert) wave_hypotheses<true, PW>(sP0, sP1, N, P.rand, trial0, 0.4f, lane, ps.faults, ws->counts, sN, cert, 0);
    else wave_hypotheses<false, PW>(sP0, sP1, N, P.rand, trial0, 0.4f, lane, ps.faults, ws->counts);
}
template <int PW> __global__ void __launch_bounds__(64 * RE_WAVES) k_ransac_hyp(const caelo_pair_set ps, int ld0, int ld1, int64_t k1_max) { ransac_hyp_body<PW>(ps, ld0, ld1, k1_max); }


// Round 6: certificates for the 0.8 m and 1.6 m levels (Match.py:207-214).  A pair escalates when no hypothesis of a level reaches
// leastInliers; without bounds for the next level the host half evaluates all of its (up to 500) hypotheses like the reference's loop --
// 2.7 ms of a host core per level, and on data with real failures the exact path becomes a CPU path (missing 3).  Launched
// behind k_ransac_hyp (before k_ransac_finish reuses the counts) for pairs that leave a certificate: a workgroup first looks at the first level's 500 counts and
// returns unless none reached leastInliers (the device's own float64 counts: the reference's may differ by a pair at the threshold,
// in which case the host half meets a level without bounds and evaluates it the long way -- still exact); otherwise blockIdx.y's level
// (0.8 m, 1.6 m: both, the second is wasted when the first succeeds, and escalations are rare) gets its `hi_up` / `idx_up` exactly as
// the first level got `hi` / `idx`.  The inlier counts of these levels are not kept (scratch): the host half derives them.
// (RH_BLOCKS(PW) workgroups per level and pair cover its 500 trials in one round.  At four per wavefront 8 workgroups needed four rounds and a batch with a failing pair took 4 x longer: 32 there)
template <int PW>
static __device__ __forceinline__ void ransac_hyp_up_body(const caelo_pair_set &ps, int ld0, int ld1, int64_t k1_max) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    caelo_ransac_cert *cert = P.cert;
    if (!cert) return;
    RansacWs *ws = (RansacWs *)P.ws_ransac;
    const int N = (P.n0 && *P.n0 <= 0) ? 0 : (P.n1 ? min(max(*P.n1, 0), (int)k1_max) : (int)k1_max);
    if (N > RE_LDS_PAIRS) return;
    const int least = min(100, (int)(0.2 * (double)N));   // :166
    if (least <= 0) return;                                // N < 5: the first level "succeeds" without any inlier (:195-205)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool reached = false;
    for (int t = tid; t < CAELO_RANSAC_MAX_TRIALS; t += 64 * RE_WAVES) reached = reached || ws->counts[t] >= least;
    if (__syncthreads_or(reached)) return;
    __shared__ float sP0[RE_LDS_PAIRS * 3], sP1[RE_LDS_PAIRS * 3];
    __shared__ float2 sN[RE_LDS_PAIRS];
    __shared__ int32_t s_scratch[CAELO_RANSAC_MAX_TRIALS];
    const float *__restrict__ pc0 = P.pc0, *__restrict__ pc1 = P.pc1;
    const int64_t *__restrict__ pair_idx = P.pair_idx;
    for (int i = tid; i < N; i += 64 * RE_WAVES) {
        const float *a = pc0 + (size_t)ld0 * pair_idx[i];
        const float *b = pc1 + (size_t)ld1 * i;
        const float a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
        sP0[3 * i] = a0; sP0[3 * i + 1] = a1; sP0[3 * i + 2] = a2;
        sP1[3 * i] = b0; sP1[3 * i + 1] = b1; sP1[3 * i + 2] = b2;
        sN[i] = make_float2(1.0001f * sqrtf(b0 * b0 + b1 * b1 + b2 * b2), 1.0001f * RB_G * sqrtf(a0 * a0 + a1 * a1 + a2 * a2));
    }
    __syncthreads();
    const int level = 1 + (int)blockIdx.y;   // 1, 2
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) cert->levels_up = 1;   // (k_ransac_hyp wrote 0 with the header)
    // (RH_BLOCKS(PW) workgroups per level and pair, each walking its share of the 500 trials; most launches only look at the 500 counts
    // and leave, and every workgroup of 33 KB of LDS has to be scheduled beside the encoder's persistent grids first)
    for (int trial0 = (blockIdx.x * RE_WAVES + wave) * PW; trial0 < CAELO_RANSAC_MAX_TRIALS; trial0 += RH_BLOCKS(PW) * RE_WAVES * PW)
        wave_hypotheses<true, PW>(sP0, sP1, N, P.rand + (size_t)level * CAELO_RANSAC_MAX_TRIALS * 4, trial0, 0.4f * (float)(1 << level), lane, ps.faults,
                              s_scratch, sN, cert, level);
}
template <int PW> __global__ void __launch_bounds__(64 * RE_WAVES) k_ransac_hyp_up(const caelo_pair_set ps, int ld0, int ld1, int64_t k1_max) { ransac_hyp_up_body<PW>(ps, ld0, ld1, k1_max); }


#define RF_WAVES 8   // the accept rules, the mask and the refit use four of them; all eight evaluate a next level's hypotheses
static __device__ __forceinline__ void ransac_finish_body(const caelo_pair_set &ps, int ld0, int ld1, int64_t k1_max) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    if (P.cert && P.cert_only) return;   // (a mixed set: this pair's result comes from the host half)
    const float *__restrict__ pc0 = P.pc0, *__restrict__ pc1 = P.pc1;
    const int64_t *__restrict__ pair_idx = P.pair_idx;
    const double *__restrict__ rnd = P.rand;
    RansacWs *ws = (RansacWs *)P.ws_ransac;
    caelo_pose_result *res = P.result;
    uint8_t *mask = P.mask;
    __shared__ float sP0[RE_LDS_PAIRS * 3], sP1[RE_LDS_PAIRS * 3];
    __shared__ float Rs[9], Ts[3];
    __shared__ RansacVerdict s_v;
    __shared__ double red[4][RIGID_TERMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // no pairs at all when EITHER frame has no key point (frame 0 empty: the match kernel wrote index 0 everywhere, the
    // reference's argmin over an empty axis raises): the pose fails as a value
    const int N = (P.n0 && *P.n0 <= 0) ? 0 : (P.n1 ? min(max(*P.n1, 0), (int)k1_max) : (int)k1_max);
    // ---- the first level's counts (wavefront 0, eight per lane) are fetched while all four wavefronts gather the matched
    // pairs into LDS once: the winner's sample, the inlier mask and the refit below then never touch global memory again
    // (round 2 before: three passes of dependent global gathers in this one-workgroup kernel, 27 us)
    int c0[(CAELO_RANSAC_MAX_TRIALS + 63) / 64];
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < (CAELO_RANSAC_MAX_TRIALS + 63) / 64; ++q) {
            const int i = lane * ((CAELO_RANSAC_MAX_TRIALS + 63) / 64) + q;
            c0[q] = i < CAELO_RANSAC_MAX_TRIALS ? ws->counts[i] : 0;
        }
    }
    const bool in_lds = N <= RE_LDS_PAIRS;
    if (in_lds) {
        for (int i = tid; i < N; i += 64 * RF_WAVES) {
            const float *a = pc0 + (size_t)ld0 * pair_idx[i];
            const float *b = pc1 + (size_t)ld1 * i;
            sP0[3 * i] = a[0]; sP0[3 * i + 1] = a[1]; sP0[3 * i + 2] = a[2];
            sP1[3 * i] = b[0]; sP1[3 * i + 1] = b[1]; sP1[3 * i + 2] = b[2];
        }
    }
    // ---- accept rules, level by level (:207-214: thr doubles while no hypothesis reaches leastInliers, up to 1.6)
    if (tid < 64) ransac_replay(N, ws->counts, &s_v, c0);
    __syncthreads();  // also the end of the staging above
    if (P.cert) {  // the certificate's header and the matched pairs (k_ransac_hyp wrote `hi` and `idx`)
        caelo_ransac_cert *cert = P.cert;
        if (in_lds) {
            float *d0 = &cert->p0[0][0], *d1 = &cert->p1[0][0];
            for (int i = tid; i < 3 * N; i += 64 * RF_WAVES) { d0[i] = sP0[i]; d1[i] = sP1[i]; }
        }
        if (tid == 0) {
            cert->n_pairs = N;
            cert->flags = in_lds ? 0 : CAELO_CERT_NO_BOUNDS;
            cert->magic = CAELO_CERT_MAGIC;
        }
    }
    int level = 0;
    while (!s_v.success && level < CAELO_RANSAC_LEVELS - 1) {  // rare: the next level's 500 hypotheses, sixteen per wavefront like k_ransac_hyp
        __syncthreads();  // everyone has read s_v before it is overwritten
        ++level;
        const float thr_l = 0.4f * (float)(1 << level);
        const double *rnd_l = rnd + (size_t)level * CAELO_RANSAC_MAX_TRIALS * 4;
        if (in_lds) {
            for (int trial0 = wave * RH_WIDE; trial0 < CAELO_RANSAC_MAX_TRIALS; trial0 += RF_WAVES * RH_WIDE)   // (one workgroup walks the level: four rounds of the chain, not sixteen)
                wave_hypotheses<false, RH_WIDE>(sP0, sP1, N, rnd_l, trial0, thr_l, lane, ps.faults, ws->counts);
        } else {
            for (int trial = wave; trial < CAELO_RANSAC_MAX_TRIALS; trial += RF_WAVES) {
                const int cnt = hypothesis_count(pc0, ld0, pair_idx, pc1, ld1, N, rnd_l + (size_t)trial * 4, thr_l, lane, ps.faults);
                if (lane == 0) ws->counts[trial] = cnt;
            }
        }
        __threadfence_block();
        __syncthreads();
        if (tid < 64) ransac_replay(N, ws->counts, &s_v);
        __syncthreads();
    }
    const int success = s_v.success, best = s_v.best_trial;
    const float thr = 0.4f * (float)(1 << level);  // 0.4, 0.8, 1.6 (:171,:210)
    // ---- the winner is recomputed from its sample (deterministic), identity if every level failed (:177)
    if (tid < 64) {
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, T[3] = {0.f, 0.f, 0.f};
        if (best >= 0) {
            const double *r4 = rnd + ((size_t)level * CAELO_RANSAC_MAX_TRIALS + best) * 4;
            if (in_lds) sample_hypothesis(sP0, 3, nullptr, sP1, 3, N, r4, R, T);
            else sample_hypothesis(pc0, ld0, pair_idx, pc1, ld1, N, r4, R, T);
        }
        lane_agreement(R, T, lane, ps.faults);
        if (tid < 9) Rs[tid] = R[tid];
        if (tid < 3) Ts[tid] = T[tid];
    }
    __syncthreads();
    // ---- one pass: inlier mask (four consecutive pairs per thread, one aligned 32-bit store: the whole mask row goes out as full
    // dwords) and the sums of the refit over the inliers (:193-194, :273-282)
    // (the sums, their reduction and the fit below are RigidSums / rigid_from_sums of caelo_rigid.h written out.  This kernel runs in
    // the pipeline's pair stage and was held instruction for instruction when this file was split off match.hip; with the helpers it is
    // the same arithmetic in other instructions -- 128 registers, scratch 160 -> 124 bytes -- compiled, never timed)
    double acc[RIGID_TERMS];
#pragma unroll
    for (int t = 0; t < RIGID_TERMS; ++t) acc[t] = 0.0;
    const bool word_ok = (((uintptr_t)mask) & 3u) == 0;
    for (int i0 = tid * 4; tid < 256 && i0 < (int)k1_max; i0 += 4 * 256) {   // (the first four wavefronts, as before there were eight)
        unsigned int packed = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            if (i < N && best >= 0) {
                const float *a = in_lds ? sP0 + 3 * i : pc0 + (size_t)ld0 * pair_idx[i];
                const float *b = in_lds ? sP1 + 3 * i : pc1 + (size_t)ld1 * i;
                const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
                if (residual(Rs, Ts, ax, ay, az, bx, by, bz) < thr) {
                    packed |= 1u << (8 * q);
                    const double x0 = ax, y0 = ay, z0 = az, x1 = bx, y1 = by, z1 = bz;
                    acc[0] += 1.0;
                    acc[1] += x0; acc[2] += y0; acc[3] += z0;
                    acc[4] += x1; acc[5] += y1; acc[6] += z1;
                    acc[7] += x1 * x0; acc[8] += x1 * y0; acc[9] += x1 * z0;   // P1^T P0  (:146)
                    acc[10] += y1 * x0; acc[11] += y1 * y0; acc[12] += y1 * z0;
                    acc[13] += z1 * x0; acc[14] += z1 * y0; acc[15] += z1 * z0;
                }
            }
        }
        if (word_ok && i0 + 3 < (int)k1_max) *(unsigned int *)(mask + i0) = packed;
        else
            for (int q = 0; q < 4 && i0 + q < (int)k1_max; ++q) mask[i0 + q] = (uint8_t)((packed >> (8 * q)) & 1u);
    }
#pragma unroll
    for (int t = 0; t < RIGID_TERMS; ++t)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[t] += __shfl_xor(acc[t], o);
    if (lane == 0 && wave < 4)
#pragma unroll
        for (int t = 0; t < RIGID_TERMS; ++t) red[wave][t] = acc[t];
    __syncthreads();
    if (tid < 9) { res->R_ransac[tid] = Rs[tid]; }
    if (tid < 3) { res->T_ransac[tid] = Ts[tid]; }
    if (tid == 0) {
        double sm[RIGID_TERMS];
#pragma unroll
        for (int t = 0; t < RIGID_TERMS; ++t) sm[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        const int n_in = (int)sm[0];
        res->threshold = thr;
        res->success = success;
        res->iterations = s_v.iterations;
        res->n_inliers = n_in;
        res->best_trial = best >= 0 ? level * CAELO_RANSAC_MAX_TRIALS + best : -1;
        res->n_pairs = N;
        float R[9], T[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = Rs[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) T[q] = Ts[q];
        if (n_in > 0) {  // :277-282: the pose over all inliers
            const double cnt = sm[0];
            const double m0[3] = {sm[1] / cnt, sm[2] / cnt, sm[3] / cnt}, m1[3] = {sm[4] / cnt, sm[5] / cnt, sm[6] / cnt};
            double H[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) H[3 * i + j] = sm[7 + 3 * i + j] - cnt * m1[i] * m0[j];
            rigid_from_H(H, m0, m1, R, T);
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) res->R[q] = R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) res->T[q] = T[q];
    }
}
__global__ void __launch_bounds__(64 * RF_WAVES, 4) k_ransac_finish(const caelo_pair_set ps, int ld0, int ld1, int64_t k1_max) { ransac_finish_body(ps, ld0, ld1, k1_max); }


CAELO_API int caelo_ransac(caelo_ctx *c, const float *pc0, int ld0, const float *pc1, int ld1, const int64_t *pair_idx,
                           int64_t k1_max, const int32_t *n1, const double *rnd, caelo_pose_result *result,
                           uint8_t *inlier_mask, void *wsv, caelo_ransac_cert *cert, void *stream) {
    CAELO_REQUIRE(c && pc0 && pc1 && pair_idx && rnd && result && inlier_mask && wsv, "null argument");
    CAELO_REQUIRE((((uintptr_t)cert) & 15u) == 0, "certificate not 16-byte aligned");
    caelo_pair_set ps = {};
    ps.n = 1;
    ps.faults = c->faults;
    caelo_pair_dev &p = ps.p[0];
    p.pc0 = pc0; p.pc1 = pc1; p.pair_idx = const_cast<int64_t *>(pair_idx); p.n1 = n1; p.rand = rnd; p.result = result;
    p.mask = inlier_mask; p.ws_ransac = wsv; p.cert = cert;
    return ransac_set(ps, ld0, ld1, k1_max, caelo_stream(stream));
}

// Every launch of the RANSAC kernels over one set of pairs.  `any_cert`: some pair leaves a certificate -- bounds for the
// 0.8 / 1.6 m levels of the pairs whose first level failed (workgroups of the others return at once); `all_cert_only`: the host half
// decides every pair, no finishing kernel.  Sets of RH_WIDE_FROM pairs and more score RH_WIDE hypotheses per wavefront.
static int ransac_launch(const caelo_pair_set &ps, int ld0, int ld1, int64_t k1_max, bool any_cert, bool all_cert_only, hipStream_t s) {
    const bool wide = ps.n >= RH_WIDE_FROM;
    const int blocks = wide ? RH_BLOCKS(RH_WIDE) : RH_BLOCKS(RH_NARROW);
    auto hyp = wide ? k_ransac_hyp<RH_WIDE> : k_ransac_hyp<RH_NARROW>;
    auto hyp_up = wide ? k_ransac_hyp_up<RH_WIDE> : k_ransac_hyp_up<RH_NARROW>;
    hyp<<<dim3(blocks, 1, ps.n), 64 * RE_WAVES, 0, s>>>(ps, ld0, ld1, k1_max);
    CAELO_LAUNCH_CHECK();
    if (any_cert) {
        hyp_up<<<dim3(blocks, 2, ps.n), 64 * RE_WAVES, 0, s>>>(ps, ld0, ld1, k1_max);
        CAELO_LAUNCH_CHECK();
    }
    if (all_cert_only) return CAELO_OK;
    k_ransac_finish<<<dim3(1, 1, ps.n), 64 * RF_WAVES, 0, s>>>(ps, ld0, ld1, k1_max);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

int ransac_set(const caelo_pair_set &ps, int ld0, int ld1, int64_t k1_max, hipStream_t s) {
    CAELO_REQUIRE(ps.n >= 1 && ps.n <= CAELO_FB_MAX, "bad pair count");
    CAELO_REQUIRE(k1_max > 0 && ld0 >= 3 && ld1 >= 3, "bad shape");
    bool any_cert = false, all_cert_only = true;
    for (int i = 0; i < ps.n; ++i) {
        any_cert = any_cert || ps.p[i].cert != nullptr;
        all_cert_only = all_cert_only && ps.p[i].cert && ps.p[i].cert_only;
    }
    return ransac_launch(ps, ld0, ld1, k1_max, any_cert, all_cert_only, s);
}
