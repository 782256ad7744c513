// loopclose_common.h -- the definitions of include/caelo.h's loop-closure section as __host__ __device__ functions: what the kernels of
// loopclose.hip and the host twins of loopclose_host.hip (plain C++) both run, and the entry points' argument checks.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/caelo.h"

void caelo_set_error(const char *fmt, ...);

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define LC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LC_HD static inline
#endif
#define LC_REFUSE(cond, msg)                             \
    do {                                                 \
        if (!(cond)) {                                   \
            caelo_set_error("%s: %s", __func__, msg);    \
            return CAELO_ERR_ARG;                        \
        }                                                \
    } while (0)
#define SC_RINGS 20
#define SC_SECTORS 60
#define SC_BINS (SC_RINGS * SC_SECTORS)
#define SC_PTS_WG 4096                     // points per workgroup of k_sc_build (16 passes of 256 threads)
#define LC_MASK60 ((1ull << SC_SECTORS) - 1ull)
#define LC_QT 16                           // queries per workgroup (the M of the MFMA)
#define LC_STRIP 64                        // candidates per workgroup: 16 per wavefront
#define LC_QSTRIDE 1202                    // floats between two queries' rows in LDS
#define LC_CSTRIDE 22                      // floats between two columns of the candidate's doubled image
#define LC_CCOLS 123                       // its columns: 0 .. 59 + 63
#define LC_CFLOATS (LC_CCOLS * LC_CSTRIDE)
#define LC_MAX_N (1 << 24)                 // a partial packs (shift << 24 | candidate)
#define LC_DENSE_MAX_N 4096
static_assert(SC_BINS == 1200 && SC_BINS % 4 == 0 && SC_RINGS % 4 == 0, "a k step of 4 stays inside one column");

// ---- the definitions, shared by the kernels and the host twins ---------------------------------------------------------------------
// order-preserving u32 image of a float that is no NaN; never 0, which stands for the empty bin
LC_HD uint32_t sc_encode(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LC_HD float sc_decode(uint32_t e) {
    if (e == 0u) return 0.0f;
    const uint32_t b = (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e;
    float v;
    memcpy(&v, &b, 4);
    return v;
}
// one point -> its bin (ring * 60 + sector) and encoded value; false: the point is skipped
LC_HD bool sc_point(float xf, float yf, float zf, int *bin, uint32_t *enc) {
    if (!(fabsf(xf) < __builtin_inff() && fabsf(yf) < __builtin_inff() && fabsf(zf) < __builtin_inff())) return false;
    const double x = (double)xf, y = (double)yf;
    const double r = sqrt(x * x + y * y);
    if (!(r < 80.0)) return false;
    double th = atan2(y, x);
    if (th < 0.0) th = th + 2.0 * M_PI;
    int ring = (int)floor(r / 4.0);
    int sector = (int)floor(th / (2.0 * M_PI) * 60.0);   // in this order: pi / 2 and pi divide to 0.25 and 0.5 exactly, the axes open sectors 15, 30, 45
    if (ring > SC_RINGS - 1) ring = SC_RINGS - 1;
    if (sector > SC_SECTORS - 1) sector = SC_SECTORS - 1;
    *bin = ring * SC_SECTORS + sector;
    *enc = sc_encode(zf + 2.0f);
    return true;
}
// one column: v[20] -> unit[20]; true when its norm is > 0
LC_HD bool sc_column(const float *v, float *unit) {
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < SC_RINGS; ++r) acc = fmaf(v[r], v[r], acc);
    const float norm = sqrtf(acc);
    const bool ok = norm > 0.0f;
#pragma unroll
    for (int r = 0; r < SC_RINGS; ++r) unit[r] = ok ? v[r] / norm : 0.0f;
    return ok;
}
// bit c of the result = bit (c + s) mod 60 of v, s in 0..59
LC_HD uint64_t lc_rot(uint64_t v, int s) {
    return s == 0 ? v : (((v >> s) | (v << (SC_SECTORS - s))) & LC_MASK60);
}
// the distance of one shift from its numerator; false: the shift is skipped (too few common columns, or no distance below +inf)
LC_HD bool lc_shift_dist(float num, uint64_t vi, uint64_t vj, int s, int min_cols, float *d) {
    const int n = __builtin_popcountll(vi & lc_rot(vj, s));
    if (n < min_cols) return false;
    *d = 1.0f - num / (float)n;
    return *d < __builtin_inff();
}
// the (d, then lower index) order of shifts and of candidates
LC_HD bool lc_better(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// ---- what the entry points refuse ---------------------------------------------------------------------------------------------------
#define SC_REQUIRE(pts, ld, c, n_pts, f, sc, u, valid)                                                  \
    LC_REFUSE((pts) && (n_pts) && (sc) && (u) && (valid), "null argument");                          \
    LC_REFUSE((c) == 3 || (c) == 4, "points have 3 or 4 columns");                                   \
    LC_REFUSE((ld) >= 1 && (ld) < ((int64_t)1 << 31) && (f) >= 0 && (f) <= 65535, "bad shape")

#define LC_REQUIRE(u, valid, n, q0, q1, min_gap, k, max_dist, min_cols, cand, dist, shift, dd, ds)                        \
    LC_REFUSE((u) && (valid) && (cand) && (dist) && (shift), "null argument");                                        \
    LC_REFUSE((n) >= 1 && (n) <= LC_MAX_N && (q0) >= 0 && (q0) <= (q1) && (q1) <= (n), "bad frame or query range"); \
    LC_REFUSE((k) >= 1 && (k) <= 8, "k outside 1..8");                                                                \
    LC_REFUSE((min_gap) >= 1, "min_gap < 1");                                                                         \
    LC_REFUSE((min_cols) >= 1 && (min_cols) <= SC_SECTORS, "min_cols outside 1..60");                                 \
    LC_REFUSE(!((max_dist) != (max_dist)), "max_dist is a NaN");                                                      \
    LC_REFUSE(((dd) != nullptr) == ((ds) != nullptr), "dense outputs come as a pair");                                \
    LC_REFUSE(!(dd) || (n) <= LC_DENSE_MAX_N, "dense outputs are refused above 4096 frames")
