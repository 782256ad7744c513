// iss_common.h -- what the all-pairs float64 key point detectors share (iss.hip, harris.hip): the tile and chunk sizes, the walk of a
// tile of query points over its frame (the prologue ap_query, the summing walk AP_WALK_SUMS, the suppression walk ap_walk_flags, the
// six-sum accumulator), the cyclic Jacobi, and the host side of an entry point (argument checks, frame slices, ordered compaction).
// Every device function here is a pure function of its arguments with every operation rounded on its own; a translation unit that
// includes this header sets `#pragma clang fp contract(off)` before it does.
#pragma once
#include "caelo_internal.h"

#define ISS_TILE 256
#define ISS_CHUNK 1024
#define ISS_GROUP 4        // points per step of the inner loop of the passes that sum (k_iss_scatter, k_harris_normals, k_harris_response)
#define ISS_SCAN 1024      // threads of k_iss_compact
#define ISS_SWEEPS 12      // a 3 x 3 matrix is through after 5 or 6; the bound is what ends a matrix of NaNs
#define ISS_MAX_GRID_Y 65535

// ---- the cyclic Jacobi ---------------------------------------------------------------------------------------------------------
// __host__ __device__: planar.hip runs it in a kernel and in its host twin.  The device pass compiles the same intrinsics as before;
// the host pass takes the IEEE division and square root they stand for.
#define ISS_HD __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define ISS_DIV(a, b) __ddiv_rn((a), (b))
#define ISS_SQRT(a) __dsqrt_rn(a)
#else
#define ISS_DIV(a, b) ((a) / (b))
#define ISS_SQRT(a) sqrt(a)
#endif

// (x, y) <- (c * x - s * y, s * x + c * y)
ISS_HD void iss_turn(double &x, double &y, double c, double s) {
    const double x0 = x, y0 = y;
    x = c * x0 - s * y0;
    y = s * x0 + c * y0;
}

// One Jacobi rotation that annihilates a_pq; a_rp and a_rq are the other two off-diagonal entries (r the third index).
// An entry that changes neither diagonal neighbour when added to it is set to zero without a rotation.  A zero a_pq is left alone,
// and a row and column of zeros stay zeros: c * 0 - s * 0 and s * 0 + c * 0 are 0, and the diagonal entry is never touched.
// WITH_V: an applied rotation (cosine c, sine s) turns columns P and Q of v as well.
template <bool WITH_V, int P, int Q>
ISS_HD void iss_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double (*v)[3]) {
    if (apq == 0.0) return;
    const double g = fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        apq = 0.0;
        return;
    }
    const double theta = ISS_DIV(aqq - app, 2.0 * apq);
    const double t = ISS_DIV(copysign(1.0, theta), fabs(theta) + ISS_SQRT(theta * theta + 1.0));   // (theta^2 = inf: t = 0)
    const double c = ISS_DIV(1.0, ISS_SQRT(t * t + 1.0));
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    iss_turn(arp, arq, c, s);
    if constexpr (WITH_V) {
        iss_turn(v[0][P], v[0][Q], c, s);
        iss_turn(v[1][P], v[1][Q], c, s);
        iss_turn(v[2][P], v[2][Q], c, s);
    }
}

// The symmetric matrix (a00 a01 a02; a01 a11 a12; a02 a12 a22) brought to its diagonal: rotations in the order (0,1), (0,2), (1,2),
// until the off-diagonal is exactly zero or ISS_SWEEPS sweeps are done.  WITH_V: v (row r, column c; the identity at the start)
// collects the rotations, and column c is then the eigenvector of the diagonal entry c; a row and column that are exactly zero keep
// their unit vector exactly.  Without it v is not read (nullptr).  A pure function of the six entries.
template <bool WITH_V>
ISS_HD void iss_jacobi(double &a00, double &a01, double &a02, double &a11, double &a12, double &a22, double (*v)[3]) {
    for (int sweep = 0; sweep < ISS_SWEEPS; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        iss_rotate<WITH_V, 0, 1>(a00, a11, a01, a02, a12, v);
        iss_rotate<WITH_V, 0, 2>(a00, a22, a02, a01, a12, v);
        iss_rotate<WITH_V, 1, 2>(a11, a22, a12, a01, a02, v);
    }
}

// ---- the all-pairs walk --------------------------------------------------------------------------------------------------------
// A workgroup is (tile of ISS_TILE query points, frame).  The frame's points go through LDS as float64 in chunks of ISS_CHUNK, every
// lane reading the same address (a broadcast), and every lane meets them in ascending index.  j is a neighbour of i <=> d2 < r2
// (strict), d = double(P[j]) - double(P[i]), d2 = (dx*dx + dy*dy) + dz*dz.  The __shared__ arrays belong to the kernel, which hands
// them in; what a pass does with a neighbour is its own (a small struct: the passes below and in the two .hip files).

// What every thread of such a kernel starts from: its frame f and the frame's points P, the clamped point count n, its query point i
// (valid when i < n; qx, qy, qz its coordinates, else 0) and the number of points its workgroup walks over.
struct ApQuery {
    size_t f;
    int tid, n, i;
    const float *P;
    bool valid;
    double qx, qy, qz;
    int n_loop;   // n, or 0 for a tile past the frame's end, which only writes defaults (uniform over the workgroup)
};

__device__ __forceinline__ ApQuery ap_query(const float *__restrict__ pts, const int32_t *__restrict__ n_pts, int ld) {
    ApQuery q;
    q.f = blockIdx.y;
    q.tid = threadIdx.x;
    q.n = min(max(n_pts[q.f], 0), ld);
    q.i = blockIdx.x * ISS_TILE + q.tid;
    q.P = pts + q.f * (size_t)ld * 3;
    q.valid = q.i < q.n;
    q.qx = q.qy = q.qz = 0.0;
    if (q.valid) {
        const float *p = q.P + (size_t)q.i * 3;
        q.qx = (double)p[0]; q.qy = (double)p[1]; q.qz = (double)p[2];
    }
    q.n_loop = (int)blockIdx.x * ISS_TILE < q.n ? q.n : 0;
    return q;
}

__device__ __forceinline__ double iss_d2(double dx, double dy, double dz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Between two chunks: points base .. base + m - 1 staged as float64, beside them what pass.stage(base, m, tid) stages, and the barriers.
template <class Pass>
__device__ __forceinline__ void ap_stage(const ApQuery &q, int base, int m, double *sx, double *sy, double *sz, Pass &pass) {
    __syncthreads();
    for (int k = q.tid; k < m; k += ISS_TILE) {
        const float *s = q.P + (size_t)(base + k) * 3;
        sx[k] = (double)s[0]; sy[k] = (double)s[1]; sz[k] = (double)s[2];
    }
    pass.stage(base, m, q.tid);
    __syncthreads();
}

// The walk of the passes that sum.  Four points at a time: the distances are branch-free, and the sums are visited (in the same
// ascending order) only when one of the four is a neighbour of some lane -- one point in a hundred is; then a scalar tail.
// pass.counts(k): whether staged point k, if in the radius, counts; pass.add(k, dx, dy, dz): it does.
// A macro, expanded in the kernel's body: the same loop inlined from a function is scheduled with the first distances waiting in
// front of the last LDS reads, which cost k_iss_scatter 5 %.
#define AP_WALK_SUMS(q, r2, sx, sy, sz, pass)                                                                                        \
    for (int base = 0; base < (q).n_loop; base += ISS_CHUNK) {                                                                       \
        const int m = min(ISS_CHUNK, (q).n_loop - base);                                                                             \
        ap_stage(q, base, m, sx, sy, sz, pass);                                                                                      \
        int k = 0;                                                                                                                   \
        for (; k + ISS_GROUP <= m; k += ISS_GROUP) {                                                                                 \
            double dx[ISS_GROUP], dy[ISS_GROUP], dz[ISS_GROUP];                                                                      \
            bool in[ISS_GROUP], any = false;                                                                                         \
            _Pragma("unroll") for (int u = 0; u < ISS_GROUP; ++u) {                                                                  \
                dx[u] = __dsub_rn(sx[k + u], (q).qx); dy[u] = __dsub_rn(sy[k + u], (q).qy); dz[u] = __dsub_rn(sz[k + u], (q).qz);    \
                in[u] = (iss_d2(dx[u], dy[u], dz[u]) < (r2)) & (pass).counts(k + u);                                                 \
                any |= in[u];                                                                                                        \
            }                                                                                                                        \
            if (any) {                                                                                                               \
                _Pragma("unroll") for (int u = 0; u < ISS_GROUP; ++u)                                                                \
                    if (in[u]) (pass).add(k + u, dx[u], dy[u], dz[u]);                                                               \
            }                                                                                                                        \
        }                                                                                                                            \
        for (; k < m; ++k) {                                                                                                         \
            const double dx = __dsub_rn(sx[k], (q).qx), dy = __dsub_rn(sy[k], (q).qy), dz = __dsub_rn(sz[k], (q).qz);                \
            if ((iss_d2(dx, dy, dz) < (r2)) & (pass).counts(k)) (pass).add(k, dx, dy, dz);                                           \
        }                                                                                                                            \
    }

// The neighbour count and acc = acc + (a * b), six sums: of d d^T (k_iss_scatter, k_harris_normals) or of n n^T (k_harris_response)
struct ApSums {
    int cnt = 0;
    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    __device__ __forceinline__ void add(double x, double y, double z) {
        ++cnt;
        cxx = __dadd_rn(cxx, __dmul_rn(x, x)); cxy = __dadd_rn(cxy, __dmul_rn(x, y)); cxz = __dadd_rn(cxz, __dmul_rn(x, z));
        cyy = __dadd_rn(cyy, __dmul_rn(y, y)); cyz = __dadd_rn(cyz, __dmul_rn(y, z)); czz = __dadd_rn(czz, __dmul_rn(z, z));
    }
};

// The suppression pass and its walk: the scores S of the frame staged beside the points in ss, the neighbours counted, and `beaten`
// set when one of them has a larger score than the query's qs (equal scores both survive).  Branch-free: a compare, an add and two
// mask operations per pair.
struct ApSuppress {
    const double *S;
    double *ss;
    double qs;
    int cnt = 0;
    bool beaten = false;
    __device__ __forceinline__ ApSuppress(const ApQuery &q, const double *score, int ld, double *ss_)
        : S(score + q.f * (size_t)ld), ss(ss_), qs(q.valid ? S[q.i] : -1.0) {}
    __device__ __forceinline__ void stage(int base, int m, int tid) {
        for (int k = tid; k < m; k += ISS_TILE) ss[k] = S[base + k];
    }
};

__device__ __forceinline__ void ap_walk_flags(const ApQuery &q, double r2, double *sx, double *sy, double *sz, ApSuppress &pass) {
    for (int base = 0; base < q.n_loop; base += ISS_CHUNK) {
        const int m = min(ISS_CHUNK, q.n_loop - base);
        ap_stage(q, base, m, sx, sy, sz, pass);
#pragma unroll 4
        for (int k = 0; k < m; ++k) {
            const double dx = __dsub_rn(sx[k], q.qx), dy = __dsub_rn(sy[k], q.qy), dz = __dsub_rn(sz[k], q.qz);
            const bool in = iss_d2(dx, dy, dz) < r2;
            pass.cnt += in ? 1 : 0;
            pass.beaten |= in & (pass.qs < pass.ss[k]);
        }
    }
}

// ---- the host side of an entry point -------------------------------------------------------------------------------------------

static inline bool iss_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

static inline int64_t iss_round256(int64_t v) { return (v + 255) / 256 * 256; }

// the arguments caelo_iss_keypoints and caelo_harris_keypoints share (a macro: the error text names the entry point)
#define ISS_REQUIRE_FRAMES(c, prm, n_frames, ld)                                                             \
    CAELO_REQUIRE((c) && (prm), "null argument");                                                            \
    CAELO_REQUIRE((n_frames) >= 0 && (n_frames) < (1LL << 31), "bad shape");                                 \
    CAELO_REQUIRE((ld) >= 1 && (ld) <= CAELO_ISS_MAX_POINTS, "ld must lie in [1, CAELO_ISS_MAX_POINTS]")

// k_iss_compact (iss.hip) for n_frames frames on `s`: per frame the flagged indices of is_key [n_frames][ld] in ascending order into
// key_idx [n_frames][ld], -1 behind them, and their number into n_key.  -> CAELO_OK or CAELO_ERR_HIP (the error text is set).
int iss_launch_compact(const uint8_t *is_key, const int32_t *n_pts, int32_t *key_idx, int32_t *n_key, int ld, int64_t n_frames, hipStream_t s);

// The frame is blockIdx.y: passes(grid, f0, o) launches a detector's all-pairs kernels for each slice of what a grid's y takes
// (frames f0 .. f0 + grid.y - 1, whose rows start at o = f0 * ld), then the flags they left are compacted.  -> CAELO_OK or CAELO_ERR_HIP
template <class Passes>
static int iss_run_frames(int64_t n_frames, int ld, const uint8_t *is_key, const int32_t *n_pts, int32_t *key_idx, int32_t *n_key,
                          hipStream_t s, Passes passes) {
    const unsigned tiles = (unsigned)((ld + ISS_TILE - 1) / ISS_TILE);
    for (int64_t f0 = 0; f0 < n_frames; f0 += ISS_MAX_GRID_Y) {
        const int64_t nf = n_frames - f0 < ISS_MAX_GRID_Y ? n_frames - f0 : ISS_MAX_GRID_Y;
        const int rc = passes(dim3(tiles, (unsigned)nf), f0, (size_t)f0 * ld);
        if (rc != CAELO_OK) return rc;
    }
    return iss_launch_compact(is_key, n_pts, key_idx, n_key, ld, n_frames, s);
}
