// loopclose.hip -- place recognition for loop closure: the Scan Context descriptor (Kim & Kim, IROS 2018: a polar max-height image) of
// every scan and the exhaustive column-shifted cosine search over all causal frame pairs.  include/caelo.h states the definitions;
// DESIGN.md 9n the design.
//
// Descriptor.  k_sc_build: blockIdx.z = frame, a workgroup takes SC_PTS_WG consecutive points, one point per thread and pass; ring and
// sector in float64, the bin's maximum by an integer atomicMax on an order-preserving u32 image of (float)z + 2.0f (0 = empty) --
// first in the workgroup's private 1 200 bins in LDS, then one global atomicMax per bin the workgroup touched.  A maximum does not
// depend on the order, so the same input gives the same bytes on every run.  k_sc_prepare: one wavefront per frame, lane c = sector c:
// decodes the bins and writes SC, the unit columns u and the valid mask.
//
// Search.  k_loop_search on v_mfma_f32_16x16x4_f32, whose result is bit for bit a k-ordered fmaf chain: M = 16 queries, N = 16 shifts of
// one candidate, K = 1 200 in 300 ascending steps; four n-tiles (shifts 0..63, 60..63 ignored) are four independent accumulators of one
// wavefront.  The shifted B operand is never made: the candidate's columns stand twice back to back in LDS and element (k, s) is
// column k / 20 + s, row k % 20 of that image.  Its columns are 22 floats apart and a query's row 1 202: ds_read_b32 serves lanes
// 0..31 and 32..63 in turn over 32 banks, a group holds 16 shifts (or queries) x 2 k, and 22 n mod 32 (1 202 m mod 32 = 18 m mod 32)
// runs through the 16 even banks -- 32 distinct banks per group for both operands (strides of 20 and 1 200 would reach 16 and 4 banks).
// A workgroup is 16 queries x a strip of 64 candidates, its four wavefronts take a different candidate each (one wavefront per SIMD:
// the LDS reads are ordered two k steps ahead of their MFMAs, the next candidate travels through registers meanwhile); the epilogue turns the
// numerators into distances per lane and reduces over the shifts by (d, s); per-strip top-k goes to the workspace and k_loop_merge
// combines the strips by (d, j).  No atomic decides a result.
//
// The host twins (caelo_host_scan_context, caelo_host_loop_search; loopclose_host.hip) run the same __host__ __device__ pieces
// (loopclose_common.h) with fmaf, sqrtf and / in the same order; the CPU tests call them and the device is tested against them byte for byte.
#include "caelo_internal.h"
#include "loopclose_common.h"

#pragma clang fp contract(off)

// ---- the descriptor ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sc_build(const float *__restrict__ pts, int64_t ld, int c, const int32_t *__restrict__ n_pts,
                                                  uint32_t *__restrict__ bins) {
    __shared__ uint32_t s_bin[SC_BINS];
    const int f = blockIdx.z, tid = threadIdx.x;
    int64_t n = n_pts[f];
    if (n > ld) n = ld;
    const int64_t p0 = (int64_t)blockIdx.x * SC_PTS_WG;
    if (p0 >= n) return;
    for (int i = tid; i < SC_BINS; i += 256) s_bin[i] = 0u;
    __syncthreads();
    const float *base = pts + (int64_t)f * ld * c;
#pragma unroll 1
    for (int pass = 0; pass < SC_PTS_WG / 256; ++pass) {
        const int64_t p = p0 + pass * 256 + tid;
        if (p < n) {
            const float *q = base + p * c;
            int bin;
            uint32_t enc;
            if (sc_point(q[0], q[1], q[2], &bin, &enc)) atomicMax(&s_bin[bin], enc);
        }
    }
    __syncthreads();
    uint32_t *out = bins + (int64_t)f * SC_BINS;
    for (int i = tid; i < SC_BINS; i += 256) {
        const uint32_t e = s_bin[i];
        if (e) atomicMax(&out[i], e);
    }
}

__global__ void __launch_bounds__(64) k_sc_prepare(const uint32_t *__restrict__ bins, float *__restrict__ sc, float *__restrict__ u,
                                                   unsigned long long *__restrict__ valid) {
    const int f = blockIdx.x, col = threadIdx.x;
    bool ok = false;
    if (col < SC_SECTORS) {
        float v[SC_RINGS], unit[SC_RINGS];
#pragma unroll
        for (int r = 0; r < SC_RINGS; ++r) {
            v[r] = sc_decode(bins[(int64_t)f * SC_BINS + r * SC_SECTORS + col]);
            sc[(int64_t)f * SC_BINS + r * SC_SECTORS + col] = v[r];
        }
        ok = sc_column(v, unit);
        float4 *o = (float4 *)(u + (int64_t)f * SC_BINS + col * SC_RINGS);
#pragma unroll
        for (int r = 0; r < SC_RINGS; r += 4) o[r / 4] = make_float4(unit[r], unit[r + 1], unit[r + 2], unit[r + 3]);
    }
    const unsigned long long m = __ballot(ok);
    if (col == 0) valid[f] = m & LC_MASK60;
}

// ---- the search --------------------------------------------------------------------------------------------------------------------
struct LcArgs {
    const float *u;                       // [n][1200]
    const unsigned long long *valid;      // [n]
    int32_t n, q0, q1, min_gap, k, min_cols;
    float max_dist;                       // +inf: none
    float *part_d;                        // [tiles][strips][16][k]
    int32_t *part_j;                      //   shift << 24 | candidate, -1: empty
    int32_t strips;                       // strips a query tile has room for in the workspace
    float *dense_d;                       // [q1 - q0][n] or null
    int8_t *dense_s;
    int32_t *cand, *shift;                // [q1 - q0][k]
    float *dist;
};
// the strips that hold a candidate of one of the tile's queries: candidates 0 .. (its last query) - min_gap
LC_HD int lc_tile_strips(int q0, int q1, int tile, int min_gap) {
    int last = q0 + tile * LC_QT + LC_QT - 1;
    if (last > q1 - 1) last = q1 - 1;
    const int jmax = last - min_gap;
    return jmax < 0 ? 0 : jmax / LC_STRIP + 1;
}

#define LC_LDS_Q (LC_QT * LC_QSTRIDE)
#define LC_LDS_BYTES ((LC_LDS_Q + 4 * LC_CFLOATS + LC_QT * LC_STRIP) * 4 + LC_QT * LC_STRIP + LC_QT * 8)

// the k-th pick of a selection without a list: the best entry behind (pd, pj) in the (d, j) order
#define LC_PICK_INIT(bd, bj) float bd = __builtin_inff(); int bj = 0x7FFFFFFF
__device__ __forceinline__ bool lc_after(float d, int j, float pd, int pj) { return d > pd || (d == pd && j > pj); }

__global__ void __launch_bounds__(256) k_loop_search(const LcArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lc_lds[];
    float *sC = lc_lds;                                     // [4 wavefronts][123][22] a candidate's columns, twice (first: the B
                                                            // reads' tile offsets then fit the instruction's 16-bit offset field)
    float *sQ = sC + 4 * LC_CFLOATS;                        // [16][1202] the queries' unit columns
    float *sD = sQ + LC_LDS_Q;                              // [16][64] the strip's distances
    int8_t *sS = (int8_t *)(sD + LC_QT * LC_STRIP);         // [16][64] and shifts
    unsigned long long *sV = (unsigned long long *)(sS + LC_QT * LC_STRIP);   // [16] the queries' valid masks
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strip = blockIdx.x, tile = blockIdx.y;
    const int qb = a.q0 + tile * LC_QT, j0 = strip * LC_STRIP;
    const bool live = strip < lc_tile_strips(a.q0, a.q1, tile, a.min_gap);
    if (!live) {
        // nothing of this tile is a candidate here: only the dense images want their +inf / -1
        if (a.dense_d)
            for (int e = tid; e < LC_QT * LC_STRIP; e += 256) {
                const int m = e / LC_STRIP, j = j0 + e % LC_STRIP;
                if (qb + m < a.q1 && j < a.n) {
                    a.dense_d[(int64_t)(qb + m - a.q0) * a.n + j] = __builtin_inff();
                    a.dense_s[(int64_t)(qb + m - a.q0) * a.n + j] = -1;
                }
            }
        return;
    }
    // the queries: rows behind q1 are zero columns with an empty mask
    for (int e = tid; e < LC_QT * (SC_BINS / 4); e += 256) {
        const int m = e / (SC_BINS / 4), k4 = e % (SC_BINS / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (qb + m < a.q1) v = ((const float4 *)(a.u + (int64_t)(qb + m) * SC_BINS))[k4];
        float2 *o = (float2 *)(sQ + m * LC_QSTRIDE + 4 * k4);   // 1202 m + 4 k4 is even: 8-byte aligned
        o[0] = make_float2(v.x, v.y);
        o[1] = make_float2(v.z, v.w);
    }
    if (tid < LC_QT) sV[tid] = qb + tid < a.q1 ? a.valid[qb + tid] : 0ull;
    __syncthreads();
    int last = qb + LC_QT - 1;
    if (last > a.q1 - 1) last = a.q1 - 1;
    const int jmax = last - a.min_gap;                      // >= j0: the strip is live
    float *cw = sC + wave * LC_CFLOATS;
    const float *qa = sQ + (lane & 15) * LC_QSTRIDE + (lane >> 4);
    const float *cb = cw + (lane & 15) * LC_CSTRIDE + (lane >> 4);
    // a candidate's 300 float4 travel through registers: the next one's loads are in flight under this one's MFMAs
    float4 nx[5];
#define LC_FETCH(j_)                                                                  \
    do {                                                                              \
        const float4 *src_ = (const float4 *)(a.u + (int64_t)(j_) * SC_BINS);         \
        _Pragma("unroll") for (int i_ = 0; i_ < 5; ++i_)                              \
            if (lane + 64 * i_ < SC_BINS / 4) nx[i_] = src_[lane + 64 * i_];          \
    } while (0)
    if (j0 + wave <= jmax) LC_FETCH(j0 + wave);
#pragma unroll 1
    for (int it = 0; it < LC_STRIP / 4; ++it) {
        const int jl = wave + 4 * it, j = j0 + jl;          // uniform over the wavefront
        float bd[4];
        int bs[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { bd[r] = __builtin_inff(); bs[r] = 64; }
        if (j <= jmax) {                                    // (jmax < q1 <= n)
            // the candidate's columns, each at its own place and 60 columns on (and the first three 120 on): float4 p holds floats
            // 4 p .. 4 p + 3 of column p / 5
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int p = lane + 64 * i;
                if (p < SC_BINS / 4) {
                    const float4 v = nx[i];
                    const int col = p / 5, w = 4 * (p % 5);
                    for (int rep = col; rep < LC_CCOLS; rep += SC_SECTORS) {
                        float2 *o = (float2 *)(cw + rep * LC_CSTRIDE + w);
                        o[0] = make_float2(v.x, v.y);
                        o[1] = make_float2(v.z, v.w);
                    }
                }
            }
            if (it + 1 < LC_STRIP / 4 && j + 4 <= jmax) LC_FETCH(j + 4);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
#pragma unroll 1
            for (int col = 0; col < SC_SECTORS; col += 2) {
#pragma unroll
                for (int w = 0; w < 2 * SC_RINGS; w += 4) {     // k = 20 col + w .. + 3, ascending (two columns: ten k steps)
                    const float av = qa[col * SC_RINGS + w];
                    const float *b = cb + (col + w / SC_RINGS) * LC_CSTRIDE + w % SC_RINGS;
                    acc0 = MFMA16(av, b[0 * 16 * LC_CSTRIDE], acc0);
                    acc1 = MFMA16(av, b[1 * 16 * LC_CSTRIDE], acc1);
                    acc2 = MFMA16(av, b[2 * 16 * LC_CSTRIDE], acc2);
                    acc3 = MFMA16(av, b[3 * 16 * LC_CSTRIDE], acc3);
                }
                // With one wavefront per SIMD nothing but the order of this block hides the LDS latency: the reads of two k steps
                // (five ds_read2) go out before the eight MFMAs of the two steps before them.
                __builtin_amdgcn_sched_group_barrier(0x100, 10, 0);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
            }
            // lane: shift 16 t + (lane & 15) of tile t, queries 4 (lane >> 4) + r
            const unsigned long long vj = a.valid[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned long long vi = sV[4 * (lane >> 4) + r];
                const float num[4] = {acc0[r], acc1[r], acc2[r], acc3[r]};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int s = 16 * t + (lane & 15);
                    float d;
                    if (s < SC_SECTORS && lc_shift_dist(num[t], vi, vj, s, a.min_cols, &d) && lc_better(d, s, bd[r], bs[r])) {
                        bd[r] = d;
                        bs[r] = s;
                    }
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const float od = __shfl_xor(bd[r], o);
                    const int os = __shfl_xor(bs[r], o);
                    if (lc_better(od, os, bd[r], bs[r])) { bd[r] = od; bs[r] = os; }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next candidate overwrites what this one's reads saw
            __builtin_amdgcn_wave_barrier();
        }
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 4 * (lane >> 4) + r, i = qb + m;
                const bool in = i < a.q1 && j <= i - a.min_gap && bs[r] < 64;
                sD[m * LC_STRIP + jl] = in ? bd[r] : __builtin_inff();
                sS[m * LC_STRIP + jl] = in ? (int8_t)bs[r] : (int8_t)-1;
            }
        }
    }
#undef LC_FETCH
    __syncthreads();
    if (a.dense_d)
        for (int e = tid; e < LC_QT * LC_STRIP; e += 256) {
            const int m = e / LC_STRIP, j = j0 + e % LC_STRIP;
            if (qb + m < a.q1 && j < a.n) {
                a.dense_d[(int64_t)(qb + m - a.q0) * a.n + j] = sD[e];
                a.dense_s[(int64_t)(qb + m - a.q0) * a.n + j] = sS[e];
            }
        }
    // the strip's k best per query, by (d, j): pick after pick, each the best entry behind the one before
    if (tid < LC_QT) {
        const int m = tid;
        float pd = -__builtin_inff();
        int pj = -1;
        float *od = a.part_d + (((int64_t)tile * a.strips + strip) * LC_QT + m) * a.k;
        int32_t *oj = a.part_j + (((int64_t)tile * a.strips + strip) * LC_QT + m) * a.k;
        for (int t = 0; t < a.k; ++t) {
            LC_PICK_INIT(bd, bj);
            int bsh = -1;
            for (int jl = 0; jl < LC_STRIP; ++jl) {
                const float d = sD[m * LC_STRIP + jl];
                const int s = sS[m * LC_STRIP + jl];
                if (s >= 0 && d < a.max_dist && lc_after(d, jl, pd, pj) && lc_better(d, jl, bd, bj)) { bd = d; bj = jl; bsh = s; }
            }
            od[t] = bd;
            oj[t] = bsh < 0 ? -1 : ((bsh << 24) | (j0 + bj));
            if (bsh < 0) { pd = __builtin_inff(); pj = 0x7FFFFFFF; } else { pd = bd; pj = bj; }
        }
    }
}

__global__ void __launch_bounds__(64) k_loop_merge(const LcArgs a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.q1 - a.q0) return;
    const int tile = t / LC_QT, m = t % LC_QT;
    const int ns = lc_tile_strips(a.q0, a.q1, tile, a.min_gap);
    float pd = -__builtin_inff();
    int pj = -1;
    for (int out = 0; out < a.k; ++out) {
        LC_PICK_INIT(bd, bj);
        int bsh = -1;
        for (int strip = 0; strip < ns; ++strip) {
            const float *d = a.part_d + (((int64_t)tile * a.strips + strip) * LC_QT + m) * a.k;
            const int32_t *js = a.part_j + (((int64_t)tile * a.strips + strip) * LC_QT + m) * a.k;
            for (int e = 0; e < a.k; ++e) {
                const int w = js[e];
                if (w < 0) break;                                        // a strip's picks are in order, the empty ones last
                const int j = w & (LC_MAX_N - 1);
                if (lc_after(d[e], j, pd, pj) && lc_better(d[e], j, bd, bj)) { bd = d[e]; bj = j; bsh = w >> 24; }
            }
        }
        a.cand[(int64_t)t * a.k + out] = bsh < 0 ? -1 : bj;
        a.dist[(int64_t)t * a.k + out] = bd;
        a.shift[(int64_t)t * a.k + out] = bsh;
        if (bsh < 0) { pd = __builtin_inff(); pj = 0x7FFFFFFF; } else { pd = bd; pj = bj; }
    }
}

// ---- the entry points --------------------------------------------------------------------------------------------------------------
CAELO_API int64_t caelo_sc_ws_bytes(int64_t n_frames) {
    return n_frames < 0 ? 0 : (n_frames * SC_BINS * 4 + 15) / 16 * 16;
}

CAELO_API int caelo_scan_context(caelo_ctx *c, const float *pts, int64_t ld, int cols, const int32_t *n_pts, int64_t n_frames, float *sc,
                                 float *u, uint64_t *valid, void *ws, void *stream) {
    CAELO_REQUIRE(c && ws, "null argument");
    SC_REQUIRE(pts, ld, cols, n_pts, n_frames, sc, u, valid);
    CAELO_REQUIRE(((uintptr_t)ws & 15u) == 0 && ((uintptr_t)u & 15u) == 0, "ws and u must be 16-byte aligned");
    if (n_frames == 0) return CAELO_OK;
    hipStream_t s = caelo_stream(stream);
    CAELO_HIP(hipMemsetAsync(ws, 0, (size_t)caelo_sc_ws_bytes(n_frames), s));
    k_sc_build<<<dim3((unsigned)((ld + SC_PTS_WG - 1) / SC_PTS_WG), 1, (unsigned)n_frames), 256, 0, s>>>(pts, ld, cols, n_pts, (uint32_t *)ws);
    CAELO_LAUNCH_CHECK();
    k_sc_prepare<<<(unsigned)n_frames, 64, 0, s>>>((const uint32_t *)ws, sc, u, (unsigned long long *)valid);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

static int lc_ws_strips(int64_t q0, int64_t q1, int min_gap) {
    const int tiles = (int)((q1 - q0 + LC_QT - 1) / LC_QT);
    return tiles ? lc_tile_strips((int)q0, (int)q1, tiles - 1, min_gap) : 0;
}

CAELO_API int64_t caelo_loop_search_ws_bytes(int64_t n, int64_t q0, int64_t q1, int min_gap, int k) {
    if (n < 1 || n > LC_MAX_N || q0 < 0 || q0 > q1 || q1 > n || k < 1 || k > 8 || min_gap < 1) return 0;
    const int64_t tiles = (q1 - q0 + LC_QT - 1) / LC_QT;
    const int64_t entries = tiles * lc_ws_strips(q0, q1, min_gap) * LC_QT * k;
    return (entries * 8 + 15) / 16 * 16 + 16;
}

CAELO_API int caelo_loop_search(caelo_ctx *c, const float *u, const uint64_t *valid, int64_t n, int64_t q0, int64_t q1, int min_gap, int k,
                                float max_dist, int min_cols, int32_t *cand, float *dist, int32_t *shift, float *dense_dist,
                                int8_t *dense_shift, void *ws, void *stream) {
    CAELO_REQUIRE(c && ws, "null argument");
    LC_REQUIRE(u, valid, n, q0, q1, min_gap, k, max_dist, min_cols, cand, dist, shift, dense_dist, dense_shift);
    CAELO_REQUIRE(((uintptr_t)ws & 15u) == 0 && ((uintptr_t)u & 15u) == 0, "ws and u must be 16-byte aligned");
    if (q1 == q0) return CAELO_OK;
    hipStream_t s = caelo_stream(stream);
    static std::mutex mu;
    static int attr[CAELO_MAX_DEVICES];
    static bool have[CAELO_MAX_DEVICES];
    const int rc = per_device_once(c->device, attr, have, mu, [] {
        return (int)hipFuncSetAttribute((const void *)k_loop_search, hipFuncAttributeMaxDynamicSharedMemorySize, LC_LDS_BYTES);
    });
    CAELO_HIP((hipError_t)rc);
    const int tiles = (int)((q1 - q0 + LC_QT - 1) / LC_QT);
    LcArgs a;
    a.u = u; a.valid = (const unsigned long long *)valid;
    a.n = (int32_t)n; a.q0 = (int32_t)q0; a.q1 = (int32_t)q1; a.min_gap = min_gap; a.k = k; a.min_cols = min_cols;
    a.max_dist = max_dist;
    a.strips = lc_ws_strips(q0, q1, min_gap);
    const int64_t entries = (int64_t)tiles * a.strips * LC_QT * k;
    a.part_d = (float *)ws;
    a.part_j = (int32_t *)((char *)ws + (entries * 4 + 15) / 16 * 16);
    a.dense_d = dense_dist; a.dense_s = dense_shift;
    a.cand = cand; a.dist = dist; a.shift = shift;
    const int grid_x = dense_dist ? (int)((n + LC_STRIP - 1) / LC_STRIP) : a.strips;
    CAELO_REQUIRE(tiles <= 65535, "more than 65535 query tiles in one call");
    if (grid_x > 0) {
        k_loop_search<<<dim3((unsigned)grid_x, (unsigned)tiles), 256, LC_LDS_BYTES, s>>>(a);
        CAELO_LAUNCH_CHECK();
    }
    k_loop_merge<<<(unsigned)((q1 - q0 + 63) / 64), 64, 0, s>>>(a);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
