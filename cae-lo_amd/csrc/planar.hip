// planar.hip -- planar points with normals for ICP_Pt2PtAndPt2Plane (RefinePoses.py:291-294): the producer the reference wrote down
// inside GetKeyPtsByAE's commented per-pixel loop (SphericalRing.py:236-282; PlanarThreshold = 0.4 at :129, radiusX = radiusY = 2 at
// :117-118, the PCA block at :268-276).  include/caelo.h states the contract; DESIGN.md 9m the design.
//
// The per-pixel rule pl_rule is ONE __host__ __device__ function over a window accessor: k_planar_rule runs it with a pixel per
// thread on a tile staged in LDS, caelo_host_planar_points loops it over host arrays (the CPU tests pin every branch there, and a
// stand-alone host program can call it under a sanitizer).  Both sides perform the same operations in the same order.
//
// Two launches.  k_planar_rule: k_kp_score's geometry (ring.hip) -- a 4 x 64 pixel tile per 256-thread workgroup, the 8 x 68 halo
// of response vectors, x/y/z and occupancy bits in LDS -- a wavefront is one image row x 64 columns; it writes its lanes' rows into
// a dense per-pixel scratch and its survivor ballot (one plain 8-byte store per wavefront).  k_planar_compact: every workgroup adds up
// the popcounts of the ballots in front of its four wavefronts and scatters their rows by popcount(ballot below lane).  Positions
// come from the ballots alone -- no atomics -- so the output is in row-major pixel order (the subsample of MyICP.py:137-140 indexes
// into it) and the same input gives the same bytes on every run.
#include "iss_common.h"

#include <math.h>

#pragma clang fp contract(off)

#define PL_HD __host__ __device__ __forceinline__
#define PL_ROWS 4
#define PL_COLS 64
#define PL_HR (PL_ROWS + 4)
#define PL_HC (PL_COLS + 4)
#define PL_Y0 8                                      // AllPixelIndexes_WithoutWindowEdge (:64-68): rows 8..55, columns 8..1783
#define PL_Y1 (CAELO_NET_H - 8)
#define PL_X0 8
#define PL_X1 (CAELO_NET_W - 8)
#define PL_TILES_X (CAELO_NET_W / PL_COLS)
#define PL_WAVES ((PL_Y1 - PL_Y0) * PL_TILES_X)      // 1 344 wavefronts, in row-major pixel order
#define PL_SCAN_WAVES 4                              // wavefronts per workgroup of k_planar_compact
static_assert(CAELO_NET_W % PL_COLS == 0 && (PL_Y1 - PL_Y0) % PL_ROWS == 0, "whole tiles");
static_assert(PL_WAVES % PL_SCAN_WAVES == 0, "whole workgroups");
static_assert(CAELO_PLANAR_MAX == (PL_Y1 - PL_Y0) * (PL_X1 - PL_X0), "one row per interior pixel");

// ---- the rule ----------------------------------------------------------------------------------------------------------------------
// The squared float32 distance of two response vectors in NumPy's 8-lane pairwise order, every operation rounded on its own: the
// expression k_kp_score reproduces bit for bit (ring.hip:647-656).
PL_HD float pl_dist2(const float *q, const float *p) {
    float d;
    d = q[0] - p[0]; const float s0 = d * d;
    d = q[1] - p[1]; const float s1 = d * d;
    d = q[2] - p[2]; const float s2 = d * d;
    d = q[3] - p[3]; const float s3 = d * d;
    d = q[4] - p[4]; const float s4 = d * d;
    d = q[5] - p[5]; const float s5 = d * d;
    d = q[6] - p[6]; const float s6 = d * d;
    d = q[7] - p[7]; const float s7 = d * d;
    return ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
}

// One pixel.  W is its 5 x 5 window, entry k = 5 r + c (window row r, column c; the centre is k = 12):
//   bits()      the occupancy (counter > 0) of the 25 entries, entry k at bit k
//   resp(k, v)  the 8 response channels of entry k;   xyz(k, p)  its ring channels 0:3
// -> true and row = [x, y, z, n_x, n_y, n_z] when the pixel is a planar point.
template <class W>
PL_HD bool pl_rule(const W &w, float *row) {
    const unsigned win = w.bits();
    if (!((win >> 12) & 1u)) return false;                                // :243
    const unsigned nb = win & ~(1u << 12);                                // :246-247: the window's mask with its centre cleared
    const int cnt = __builtin_popcount(nb);
    if (cnt < 5) return false;                                            // :250
    float pa[8];
    w.resp(12, pa);
    // min over sqrt(t) = sqrt(min t): the square root is monotone and correctly rounded.  A NaN among the occupied neighbours'
    // distances stays a NaN (t < NaN is false) and fails every comparison below.
    float best = __builtin_inff();
#pragma unroll
    for (int k = 0; k < 25; ++k) {
        if (k == 12) continue;
        float q[8];
        w.resp(k, q);
        const float t = pl_dist2(q, pa);
        const bool o = (nb >> k) & 1u;
        best = (o && (t < best || t != t)) ? t : best;
    }
    const float minDiff = sqrtf(best);                                    // :253
    float c[3];
    w.xyz(12, c);
    if ((double)minDiff > 0.2) {                                          // :259-262: a key point candidate below VisibleBottom
        const float n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];       //           `continue`s past the planar block as well
        if (sqrtf(n2) < 10.0f) return false;
    }
    if (!((double)minDiff < 0.4)) return false;                           // :268 PlanarThreshold
    // np.cov(pts, rowvar=0) over the occupied entries without the centre, in window order (:269-271): mean = sum / N, then the
    // centred second moments / (N - 1), float64, summed one after the other
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int k = 0; k < 25; ++k) {
        float p[3];
        w.xyz(k, p);
        if ((nb >> k) & 1u) { sx = sx + (double)p[0]; sy = sy + (double)p[1]; sz = sz + (double)p[2]; }
    }
    const double n = (double)cnt, mx = sx / n, my = sy / n, mz = sz / n;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
#pragma unroll
    for (int k = 0; k < 25; ++k) {
        float p[3];
        w.xyz(k, p);
        if ((nb >> k) & 1u) {
            const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
            a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz;
            a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
        }
    }
    const double f = n - 1.0;
    a00 = a00 / f; a01 = a01 / f; a02 = a02 / f; a11 = a11 / f; a12 = a12 / f; a22 = a22 / f;
    // the eigenvector of the smallest eigenvalue (:272-274); among equal eigenvalues the first, like a stable argsort.  A covariance
    // of NaNs (a non-finite coordinate in the window) leaves the bounded sweeps with a NaN vector, which fails :275.
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    iss_jacobi<true>(a00, a01, a02, a11, a12, a22, v);
    int e = 0;
    double lam = a00;
    if (a11 < lam) { lam = a11; e = 1; }
    if (a22 < lam) e = 2;
    double nx = e == 0 ? v[0][0] : e == 1 ? v[0][1] : v[0][2];
    double ny = e == 0 ? v[1][0] : e == 1 ? v[1][1] : v[1][2];
    double nz = e == 0 ? v[2][0] : e == 1 ? v[2][1] : v[2][2];
    if (!(fabs(nz) > 0.9)) return false;                                  // :275
    if (nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }                       // LAPACK's sign is arbitrary; ours is n_z > 0
    row[0] = c[0]; row[1] = c[1]; row[2] = c[2];                          // :276, :285
    row[3] = (float)nx; row[4] = (float)ny; row[5] = (float)nz;
    return true;
}

// a pixel's window read from the images themselves (the host twin)
struct PlImage {
    const float *ring;
    int ring_w, ring_c;
    const int32_t *counter;
    int cnt_w;
    const float *resp_img;
    int y, x;   // the centre: rows 8..55, columns 8..1783, so that every entry lies inside the images
    PL_HD unsigned bits() const {
        unsigned b = 0u;
        for (int k = 0; k < 25; ++k)
            if (counter[(int64_t)(y - 2 + k / 5) * cnt_w + (x - 2 + k % 5)] > 0) b |= 1u << k;
        return b;
    }
    PL_HD void resp(int k, float *v) const {
        const float *q = resp_img + ((int64_t)(y - 2 + k / 5) * CAELO_NET_W + (x - 2 + k % 5)) * 8;
        for (int ch = 0; ch < 8; ++ch) v[ch] = q[ch];
    }
    PL_HD void xyz(int k, float *p) const {
        const float *q = ring + ((int64_t)(y - 2 + k / 5) * ring_w + (x - 2 + k % 5)) * ring_c;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
};

// ---- the kernels -------------------------------------------------------------------------------------------------------------------
// a pixel's window in the tile's LDS image: halo entry (ly + r, lx + c) is window entry (r, c)
struct PlTile {
    const float4 *sR;
    const float *sP;
    const unsigned int (*sBits)[4];
    int lx, ly;
    __device__ __forceinline__ unsigned bits() const {
        unsigned win = 0u;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const unsigned int *w = sBits[ly + r];
            const int k = lx >> 5, sh = lx & 31;
            const unsigned long long two = (unsigned long long)w[k] | ((unsigned long long)w[k + 1] << 32);
            win |= ((unsigned int)(two >> sh) & 31u) << (5 * r);
        }
        return win;
    }
    __device__ __forceinline__ void resp(int k, float *v) const {
        const int q = (ly + k / 5) * PL_HC + lx + k % 5;
        const float4 a = sR[2 * q], b = sR[2 * q + 1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    __device__ __forceinline__ void xyz(int k, float *p) const {
        const int q = (ly + k / 5) * PL_HC + lx + k % 5;
        p[0] = sP[3 * q]; p[1] = sP[3 * q + 1]; p[2] = sP[3 * q + 2];
    }
};

// rows [48][1792][6] f32: the row of every surviving pixel; masks [PL_WAVES] u64: a wavefront's survivors, lane l = column 64 tile + l
__global__ void __launch_bounds__(256) k_planar_rule(const float *__restrict__ ring, int ring_w, int ring_c, const int32_t *__restrict__ counter,
                                                     int cnt_w, const float *__restrict__ resp, float *__restrict__ rows,
                                                     unsigned long long *__restrict__ masks) {
    __shared__ float4 sR[PL_HR * PL_HC * 2];
    __shared__ float sP[PL_HR * PL_HC * 3];
    __shared__ unsigned int sBits[PL_HR][4];   // occupancy of a halo row as bits (68 columns: three words)
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PL_COLS, y0 = PL_Y0 + blockIdx.y * PL_ROWS;
    if (tid < PL_HR * 4) (&sBits[0][0])[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < PL_HR * PL_HC; i += 256) {
        const int hy = i / PL_HC, hx = i % PL_HC;
        const int yy = y0 - 2 + hy, xx = x0 - 2 + hx;   // rows 6..57 always lie inside the images; columns -2, -1, 1792, 1793 do not
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        float px = 0.f, py = 0.f, pz = 0.f;
        bool occ = false;
        if (xx >= 0 && xx < CAELO_NET_W) {
            const float4 *rq4 = (const float4 *)(resp + ((int64_t)yy * CAELO_NET_W + xx) * 8);
            a = rq4[0];
            b = rq4[1];
            occ = counter[(int64_t)yy * cnt_w + xx] > 0;
            const float *p = ring + ((int64_t)yy * ring_w + xx) * ring_c;
            px = p[0]; py = p[1]; pz = p[2];
        }
        sR[2 * i] = a;
        sR[2 * i + 1] = b;
        sP[3 * i] = px; sP[3 * i + 1] = py; sP[3 * i + 2] = pz;
        if (occ) atomicOr(&sBits[hy][hx >> 5], 1u << (hx & 31));
    }
    __syncthreads();
    const int lx = tid & (PL_COLS - 1), ly = tid / PL_COLS;
    const int x = x0 + lx, y = y0 + ly;
    float row[6];
    bool keep = false;
    if (x >= PL_X0 && x < PL_X1) {
        const PlTile w = {sR, sP, sBits, lx, ly};
        keep = pl_rule(w, row);
    }
    const int pixel = (y - PL_Y0) * CAELO_NET_W + x;
    if (keep) {
        float2 *out = (float2 *)(rows + (int64_t)pixel * 6);
        out[0] = make_float2(row[0], row[1]);
        out[1] = make_float2(row[2], row[3]);
        out[2] = make_float2(row[4], row[5]);
    }
    const unsigned long long m = __ballot(keep);
    if (lx == 0) masks[(y - PL_Y0) * PL_TILES_X + blockIdx.x] = m;
}

__global__ void __launch_bounds__(64 * PL_SCAN_WAVES) k_planar_compact(const float *__restrict__ rows, const unsigned long long *__restrict__ masks,
                                                                       float *__restrict__ planar, int32_t *__restrict__ pixels,
                                                                       int32_t *__restrict__ n_planar) {
    __shared__ int s_part[PL_SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w0 = blockIdx.x * PL_SCAN_WAVES;
    int before = 0;   // survivors of the wavefronts in front of this workgroup's (integer adds: any order gives the same sum)
    for (int i = tid; i < w0; i += 64 * PL_SCAN_WAVES) before += __popcll(masks[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 0) s_part[wave] = before;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int k = 0; k < PL_SCAN_WAVES; ++k) base += s_part[k];
    unsigned long long m = 0ull;
#pragma unroll
    for (int k = 0; k < PL_SCAN_WAVES; ++k) {
        const unsigned long long mk = masks[w0 + k];
        if (k < wave) base += __popcll(mk);
        if (k == wave) m = mk;
    }
    if ((m >> lane) & 1ull) {
        const int w = w0 + wave;
        const int r = w / PL_TILES_X, x = (w % PL_TILES_X) * PL_COLS + lane;
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));   // < CAELO_PLANAR_MAX: a bit is only ever set for an interior pixel
        const float2 *in = (const float2 *)(rows + ((int64_t)r * CAELO_NET_W + x) * 6);
        float2 *out = (float2 *)(planar + (int64_t)pos * 6);
        out[0] = in[0];
        out[1] = in[1];
        out[2] = in[2];
        if (pixels) {
            pixels[2 * pos] = PL_Y0 + r;
            pixels[2 * pos + 1] = x;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 64 * PL_SCAN_WAVES - 1) *n_planar = base + __popcll(m);   // the last wavefront's last lane: everything
}

// ---- the entry points --------------------------------------------------------------------------------------------------------------
#define PL_ROWS_BYTES ((int64_t)(PL_Y1 - PL_Y0) * CAELO_NET_W * 6 * 4)

#define PL_REQUIRE_IMAGES(ring, ring_w, ring_c, counter, cnt_w, resp, planar, n_planar)                          \
    CAELO_REQUIRE((ring) && (counter) && (resp) && (planar) && (n_planar), "null argument");                     \
    CAELO_REQUIRE((ring_w) >= CAELO_NET_W && (cnt_w) >= CAELO_NET_W && ((ring_c) == 3 || (ring_c) == 5), "bad ring shape")

CAELO_API int64_t caelo_planar_ws_bytes(void) {
    return PL_ROWS_BYTES + (int64_t)PL_WAVES * 8;
}

CAELO_API int caelo_planar_points(caelo_ctx *c, const float *ring, int ring_w, int ring_c, const int32_t *counter, int cnt_w,
                                  const float *resp, void *ws, float *planar, int32_t *pixels, int32_t *n_planar, void *stream) {
    CAELO_REQUIRE(c && ws, "null argument");
    PL_REQUIRE_IMAGES(ring, ring_w, ring_c, counter, cnt_w, resp, planar, n_planar);
    CAELO_REQUIRE(((uintptr_t)ws & 15u) == 0, "ws must be 16-byte aligned");
    hipStream_t s = caelo_stream(stream);
    float *rows = (float *)ws;
    unsigned long long *masks = (unsigned long long *)((char *)ws + PL_ROWS_BYTES);
    k_planar_rule<<<dim3(PL_TILES_X, (PL_Y1 - PL_Y0) / PL_ROWS), 256, 0, s>>>(ring, ring_w, ring_c, counter, cnt_w, resp, rows, masks);
    CAELO_LAUNCH_CHECK();
    k_planar_compact<<<PL_WAVES / PL_SCAN_WAVES, 64 * PL_SCAN_WAVES, 0, s>>>(rows, masks, planar, pixels, n_planar);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

// ---- the host twin -----------------------------------------------------------------------------------------------------------------
CAELO_API int caelo_host_planar_points(const float *ring, int ring_w, int ring_c, const int32_t *counter, int cnt_w, const float *resp,
                                       float *planar, int32_t *pixels, int32_t *n_planar) {
    PL_REQUIRE_IMAGES(ring, ring_w, ring_c, counter, cnt_w, resp, planar, n_planar);
    int n = 0;
    PlImage w = {ring, ring_w, ring_c, counter, cnt_w, resp, 0, 0};
    for (w.y = PL_Y0; w.y < PL_Y1; ++w.y)
        for (w.x = PL_X0; w.x < PL_X1; ++w.x) {
            float row[6];
            if (!pl_rule(w, row)) continue;
            memcpy(planar + (int64_t)n * 6, row, sizeof row);
            if (pixels) {
                pixels[2 * n] = w.y;
                pixels[2 * n + 1] = w.x;
            }
            ++n;
        }
    *n_planar = n;
    return CAELO_OK;
}
