// match.hip -- brute-force descriptor matching: for every frame-1 descriptor its nearest frame-0 descriptor.
//
// Reference behaviour restated here (never its code):
//   NN match             Match.py:257-258   cdist (f64) + argmin(axis=0), first minimum wins
//
// Two launches per set of pairs: k_match_prep writes frame 0's f16 operand image, k_match_screen screens the all-pairs
// matrix on the f16 matrix cores and certifies each column's argmin in float64 (match_screen.inc; descriptors wider than 64:
// match_screen_wide.inc).  Descriptors 63 and 64 wide leave no room for the screen's two norm slots and take k_match_mfma below,
// the all-f64 kernel.  What follows the match -- RANSAC over the matched pairs and the refit -- is ransac.hip.
// The workspace of caelo_match is self-cleaning (zero-filled once by its owner).

#include "caelo_internal.h"

#define MT_MAXDIM 64

// ------------------------------------------------------------------------------------------------
// NN match, fast path: the all-pairs matrix on the f64 matrix cores, the argmin certified afterwards.
//   v[i][j] = |f0_i|^2 - 2 <f0_i, f1_j>  (= d^2 - |f1_j|^2) from v_mfma_f64_16x16x4_f64, with the
//   rigorous rounding bound e[i][j] = kappa (|f0_i|^2 + |f1_j|^2), kappa = (4 dim + 64) 2^-53.
//   The exact argmin i* of SciPy's cdist satisfies v[i*] - e[i*] <= min_i (v[i] + e[i]), so only rows
//   passing that test can win; they are re-evaluated exactly like cdist (sequential f64 sum of squared
//   differences, sqrt) and the first minimum is kept (Match.py:257-258).  With f64 products the window
//   is ~1e-13 wide: one row per column survives unless descriptors are duplicated.
//   (An f32 MFMA version of the same filter keeps ~100 rows per column on these descriptors -- the
//   |a|^2+|b|^2-2ab form cancels ~4 digits -- and was slower than the plain f64 scan.)
// Grid = (blocks of 2 column tiles = 32 frame-1 descriptors) x pairs of the set: 256 workgroups for 8 pairs, one per CU.
// A workgroup is 8 wavefronts: wavefront w owns column tile w & 1 (its B fragments stay in registers) and the 16-row
// tiles t of frame 0 with t % 4 == w >> 1.  The workgroup walks frame 0 ONCE: each step stages 8 row tiles (16 x 64 f32
// each) in LDS with four coalesced 16-byte loads per thread, in flight during the previous step's MFMAs, double buffered,
// and every wavefront reads its A fragments from there -- frame 0 is read from L2 once per 32 columns (8.4 MB per pair)
// instead of once per 16 (16.7 MB).
// The f64 MFMA is the slow one on this chip (16x16x4: 64 cycles of the pipe, SQ_VALU_MFMA_BUSY_CYCLES / SQ_INSTS_MFMA;
// peak 78.6 TFLOP/s) and a tile needs 16 of them and ~200 VALU instructions (f32 -> f64, norms, the top-3 bookkeeping):
// the two wavefronts of a SIMD run the loop in opposite phase (one in its MFMAs while the other does the bookkeeping of
// its previous tile).  Measured: 49 us per 8 pairs; 30 us with the MFMAs replaced by plain FMAs, 14.5 us is the MFMA time
// alone -- the f64 matrix instruction and the f64 VALU share their ALUs on this chip (matrix f64 peak = vector f64 peak
// = 78.6 TFLOP/s), so f64 bookkeeping next to f64 MFMAs adds up instead of overlapping; the remaining lever is fewer
// f64 VALU instructions per tile.
// Partial top-3 lists meet in LDS, one thread per column certifies.  Nothing crosses workgroups (round 1 split the rows
// over four 1024-thread workgroups per column tile that met through global tickets and starved behind the encoder's
// persistent grids).
// ------------------------------------------------------------------------------------------------
typedef double mm_f64x4 __attribute__((ext_vector_type(4)));
#define MM_WAVES 8
#define MM_CT 2        // column tiles per workgroup
#define MM_RQ 4        // row quarters: wavefront w owns column tile w & 1 and the row tiles t with t % 4 == w >> 1
#define MM_KSTEPS 16   // dim <= 64
#define MM_LDA 68      // floats per staged row (64 + 4: rows start 4 banks apart)
#define MM_TPS 2       // row tiles per wavefront and step: a step stages MM_RQ * MM_TPS tiles (128 rows), one barrier each
#define MM_STEP_TILES (MM_RQ * MM_TPS)

static inline int64_t ms_ws_bytes(int64_t kmax, int nb);
__host__ __device__ inline int msw_nb(int dim);
CAELO_API int64_t caelo_match_ws_bytes(int64_t k_max) {
    // [0] columns re-scanned exactly, [1] columns decided between two rows (statistics only), then frame 0's f16 operand image and
    // its rows' window shares (match_screen.inc); k_max = the larger of the two frames' row capacities
    return ms_ws_bytes(k_max > 0 ? k_max : 1, 1);
}
CAELO_API int64_t caelo_match_ws_bytes_dim(int64_t k_max, int dim) {
    // descriptors wider than 64: nb = ceil((dim + 2) / 64) operand images per 16-row tile of frame 0 (match_screen_wide.inc)
    if (dim <= MT_MAXDIM) return caelo_match_ws_bytes(k_max);
    return ms_ws_bytes(k_max > 0 ? k_max : 1, msw_nb(dim));
}

__device__ inline double exact_dist(const float *a, const float *b, int dim) {
    double acc = 0.0;
    for (int c = 0; c < dim; ++c) {
        const double d = __dsub_rn((double)a[c], (double)b[c]);
        acc = __dadd_rn(acc, __dmul_rn(d, d));
    }
    return sqrt(acc);
}

// ---- top-3 with the row index INSIDE the key.  The lower bound lo of a row is widened by 2^-30 (|v| + e) and its low
// MM_IDX_BITS mantissa bits are replaced by the row index (a change of < 2^-31 |lo|: the key is still a lower bound).  An
// ascending top-3 of such keys is a five-instruction min / max network -- no compares, no selects, no separate index registers
// (the compiler turned the select form into branches and register shuffles: 225 VALU instructions per tile, now ~100).
#define MM_IDX_BITS 21
#define MM_IDX_MASK ((1 << MM_IDX_BITS) - 1)
__device__ inline double mm_key(double lo, int i) {
    return __longlong_as_double((__double_as_longlong(lo) & ~(long long)MM_IDX_MASK) | (long long)i);
}
__device__ inline int mm_key_index(double key) { return (int)(__double_as_longlong(key) & (long long)MM_IDX_MASK); }
__device__ inline void mm_key_insert(double key, double &L1, double &L2, double &L3) {
    const double u1 = __builtin_fmax(L1, key);
    L1 = __builtin_fmin(L1, key);
    const double u2 = __builtin_fmax(L2, u1);
    L2 = __builtin_fmin(L2, u1);
    L3 = __builtin_fmin(L3, u2);
}

// 16 channels [16g, 16g+16) of one descriptor row as doubles (zero beyond dim / for an invalid row)
template <bool VEC>
__device__ inline void load_frag(const float *row, bool valid, int g, int dim, double out[MM_KSTEPS]) {
    if (VEC) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 16 * g + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && c < dim) v = *(const float4 *)(row + c);  // dim % 4 == 0 on this path
            out[4 * q] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < MM_KSTEPS; ++s) {
            const int c = 16 * g + s;
            out[s] = (valid && c < dim) ? (double)row[c] : 0.0;
        }
    }
}

// this thread's 16 bytes of a staged row tile: row (tid >> 4) & 15 of tile `t`, channels 4 (tid & 15) .. + 3
template <bool VEC>
__device__ inline float4 mm_stage_load(const float *f0, int ld0, int k0, int dim, int t, int tid) {
    const int row = (t << 4) + ((tid >> 4) & 15), c = (tid & 15) * 4;
    // rows past k0 (the tail of the last tile, whole tiles of the last step) are staged as a point 1e18 away on channel 0: their
    // distance to anything is ~1e36, so they never win a column and the bookkeeping needs no validity test
    float4 v = make_float4(c == 0 ? 1.0e18f : 0.f, 0.f, 0.f, 0.f);
    if (row < k0) {
        v.x = 0.f;
        const float *src = f0 + (size_t)row * ld0 + c;
        if (VEC) { if (c < dim) v = *(const float4 *)src; }  // dim % 4 == 0 on this path
        else {
            if (c < dim) v.x = src[0];
            if (c + 1 < dim) v.y = src[1];
            if (c + 2 < dim) v.z = src[2];
            if (c + 3 < dim) v.w = src[3];
        }
    }
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(64 * MM_WAVES) k_match_mfma(const caelo_pair_set ps, int ld0, int64_t k0_max, int ld1,
                                                              int64_t k1_max, int dim) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    const float *__restrict__ f0 = P.f0, *__restrict__ f1 = P.f1;
    const int32_t *n0p = P.n0, *n1p = P.n1;
    int64_t *__restrict__ pair_idx = P.pair_idx;
    int32_t *stats = (int32_t *)P.ws_match;
    __shared__ __attribute__((aligned(16))) float sA[2][MM_STEP_TILES][16 * MM_LDA];  // [buffer][row tile of the step][row][channel]
    __shared__ double sL[3][MM_WAVES][16];
    __shared__ double sU[MM_WAVES][16];
    __shared__ int s_rescan[16 * MM_CT];
    __shared__ double s_rd[MM_WAVES];
    __shared__ int s_ri[MM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, x = lane & 15;
    const int cw = wave & (MM_CT - 1), rh = wave / MM_CT;
    // counts live on the device; clamp so that a caller who forgot to order this launch after the
    // producer of n0/n1 reads garbage rows, never out of bounds
    const int k0 = n0p ? min(max(*n0p, 0), (int)k0_max) : (int)k0_max;
    const int k1 = n1p ? min(max(*n1p, 0), (int)k1_max) : (int)k1_max;
    const int jb = blockIdx.x * 16 * MM_CT;  // first column of the workgroup
    if (jb >= k1) return;
    if (k0 == 0) {         // no frame-0 descriptor at all (the reference's argmin would raise): index 0, the pose fails
        if (tid < 16 * MM_CT && jb + tid < k1) pair_idx[jb + tid] = 0;
        return;
    }
    const int j0 = jb + cw * 16;
    // (a wavefront whose column tile lies beyond k1 computes on zeros: same instruction stream, its results are never read)
    const double kappa = (4.0 * (double)dim + 64.0) * 1.1102230246251565e-16;  // >= 2x the worst-case bound (dim + 20) 2^-53
    const double BIG = 1.0e300;
    // B fragments (this column tile) and |f1_j|^2.  k-step s of lane group g <-> channel 16 g + s.
    double b[MM_KSTEPS];
    load_frag<VEC>(f1 + (size_t)(j0 + x) * ld1, j0 + x < k1, g, dim, b);
    double n1 = 0.0;
#pragma unroll
    for (int s = 0; s < MM_KSTEPS; ++s) n1 += b[s] * b[s];
    n1 += __shfl_xor(n1, 16);
    n1 += __shfl_xor(n1, 32);
    double L1 = BIG, L2 = BIG, L3 = BIG, U = BIG;  // keys (mm_key): BIG carries no index
    const int ntiles = (k0 + 15) >> 4;
    const int nsteps = (ntiles + MM_STEP_TILES - 1) / MM_STEP_TILES;
    // thread -> (tiles st_par, st_par + 2, ... of a step, position inside the tile): 4 loads of 16 B in flight per thread
    const int st_par = tid >> 8;
    float *st_dst0 = &sA[0][st_par][((tid >> 4) & 15) * MM_LDA + (tid & 15) * 4];
    float4 stage[MM_STEP_TILES / 2];
#pragma unroll
    for (int k = 0; k < MM_STEP_TILES / 2; ++k) {
        stage[k] = mm_stage_load<VEC>(f0, ld0, k0, dim, 2 * k + st_par, tid);
        *(float4 *)(st_dst0 + 2 * k * 16 * MM_LDA) = stage[k];
    }
    __syncthreads();
    // bookkeeping of one finished tile: rows i0 + g + 4 r of the accumulator against this lane's column
#define MM_BOOKKEEP(ACC, ACC2, PN, I0)                                                              \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                 \
        const int row = g + 4 * r; /* f64 C/D layout: row = (lane >> 4) + 4 * reg, col = lane & 15 */ \
        const double n0 = __shfl(PN, row); /* lane `row` (g = 0) holds that row's norm */           \
        const double v = __builtin_fma(-2.0, (ACC)[r] + (ACC2)[r], n0); /* = n0 - 2 dot, one rounding */ \
        const double e = kappa * (n0 + n1);                                                         \
        U = __builtin_fmin(U, v + e);                                                               \
        const double ew = __builtin_fma(__builtin_fabs(v) + e, 9.313225746154785e-10 /* 2^-30 */, e); \
        mm_key_insert(mm_key(v - ew, (I0) + row), L1, L2, L3);                                      \
    }
    mm_f64x4 accP = {0.0, 0.0, 0.0, 0.0}, acc2P = {0.0, 0.0, 0.0, 0.0};
    double pP = 0.0;
    int i0P = -1;  // no tile yet
    // The two wavefronts of a SIMD (w and w + 4) run the loop in opposite phase: one issues a tile's MFMAs and then the
    // bookkeeping of the tile before, the other the bookkeeping first -- while one occupies the matrix pipe the other
    // has VALU work, and the barrier at the end of a step re-aligns them to exactly that.
    auto main_loop = [&](auto vfirst_t) {
        constexpr bool VFIRST = decltype(vfirst_t)::value;
#pragma unroll 1
        for (int it = 0; it < nsteps; ++it) {
            const int buf = it & 1;
            if (it + 1 < nsteps) {  // the next step's rows: in flight during this step's MFMAs
#pragma unroll
                for (int k = 0; k < MM_STEP_TILES / 2; ++k)
                    stage[k] = mm_stage_load<VEC>(f0, ld0, k0, dim, MM_STEP_TILES * (it + 1) + 2 * k + st_par, tid);
            }
#pragma unroll
            for (int k = 0; k < MM_TPS; ++k) {
                if (VFIRST) {
                    if (i0P >= 0) { MM_BOOKKEEP(accP, acc2P, pP, i0P) }
                    __builtin_amdgcn_sched_barrier(0);
                }
                const int t = MM_STEP_TILES * it + k * MM_RQ + rh;  // tiles past the last hold zeros and fail i < k0
                const float *ar = &sA[buf][k * MM_RQ + rh][x * MM_LDA + 16 * g];
                double a[MM_KSTEPS];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = *(const float4 *)(ar + 4 * q);
                    a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
                }
                double p = 0.0;
#pragma unroll
                for (int s = 0; s < MM_KSTEPS; ++s) p = __builtin_fma(a[s], a[s], p);
                p += __shfl_xor(p, 16);
                p += __shfl_xor(p, 32);  // |f0_{i0+x}|^2 on every lane with this x
                // two accumulators: no MFMA waits for its predecessor (the rounding bound kappa holds for any summation order)
                mm_f64x4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < MM_KSTEPS; s += 2) {
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s + 1], b[s + 1], acc2, 0, 0, 0);
                }
                if (!VFIRST) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (i0P >= 0) { MM_BOOKKEEP(accP, acc2P, pP, i0P) }  // the previous tile: its MFMAs finished long ago
                }
                accP = acc; acc2P = acc2; pP = p; i0P = t << 4;
            }
            if (it + 1 < nsteps) {  // the other buffer: nobody reads it in this step
#pragma unroll
                for (int k = 0; k < MM_STEP_TILES / 2; ++k)
                    *(float4 *)(st_dst0 + ((buf ^ 1) * MM_STEP_TILES + 2 * k) * 16 * MM_LDA) = stage[k];
            }
            __syncthreads();
        }
    };
    if (__builtin_amdgcn_readfirstlane(wave) < 4) main_loop(std::false_type{});
    else main_loop(std::true_type{});
    if (i0P >= 0) { MM_BOOKKEEP(accP, acc2P, pP, i0P) }
#undef MM_BOOKKEEP
    // ---- workgroup top-3 per column: merge the 4 lane groups by shuffles, the four row quarters through LDS
#define MM_SHFL_MERGE(OFF)                                                                           \
    {                                                                                                \
        const double pL1 = __shfl_xor(L1, OFF), pL2 = __shfl_xor(L2, OFF), pL3 = __shfl_xor(L3, OFF); \
        U = __builtin_fmin(U, __shfl_xor(U, OFF));                                                   \
        mm_key_insert(pL1, L1, L2, L3);                                                              \
        mm_key_insert(pL2, L1, L2, L3);                                                              \
        mm_key_insert(pL3, L1, L2, L3);                                                              \
    }
    MM_SHFL_MERGE(16)
    MM_SHFL_MERGE(32)
    if (g == 0) {
        sL[0][wave][x] = L1; sL[1][wave][x] = L2; sL[2][wave][x] = L3;
        sU[wave][x] = U;
    }
    __syncthreads();
    // ---- merge the row quarters and certify: one thread per column of the workgroup's 32
    if (tid < 16 * MM_CT) {
        const int ct = tid >> 4, col = tid & 15;
        const int j = jb + tid;
        int rescan = 0;
        if (j < k1) {
            double a1 = BIG, a2 = BIG, a3 = BIG, Umin = BIG;
#pragma unroll
            for (int h = 0; h < MM_WAVES / MM_CT; ++h) {
                const int w = ct + MM_CT * h;
                Umin = __builtin_fmin(Umin, sU[w][col]);
                mm_key_insert(sL[0][w][col], a1, a2, a3);
                mm_key_insert(sL[1][w][col], a1, a2, a3);
                mm_key_insert(sL[2][w][col], a1, a2, a3);
            }
            const int i1 = mm_key_index(a1), i2 = mm_key_index(a2);
            if (a3 <= Umin) {
                rescan = 1;  // three or more rows inside the window
                if (stats) atomicAdd(&stats[0], 1);
            } else if (a2 <= Umin) {
                if (stats) atomicAdd(&stats[1], 1);
                const float *bj = f1 + (size_t)j * ld1;
                const double d1 = exact_dist(f0 + (size_t)i1 * ld0, bj, dim), d2 = exact_dist(f0 + (size_t)i2 * ld0, bj, dim);
                pair_idx[j] = (d2 < d1 || (d2 == d1 && i2 < i1)) ? i2 : i1;
            } else {
                pair_idx[j] = i1;  // certified without an exact evaluation
            }
        }
        s_rescan[tid] = rescan;
    }
    __syncthreads();
    // ---- exact re-scan of a column whose window holds three or more rows (whole workgroup)
    for (int cidx = 0; cidx < 16 * MM_CT; ++cidx) {
        if (!s_rescan[cidx]) continue;  // uniform
        const float *bj = f1 + (size_t)(jb + cidx) * ld1;
        double best = BIG;
        int besti = 0x7FFFFFFF;
        for (int i = tid; i < k0; i += 64 * MM_WAVES) {
            const double dd = exact_dist(f0 + (size_t)i * ld0, bj, dim);
            if (dd < best) { best = dd; besti = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int obi = __shfl_xor(besti, o);
            if (ob < best || (ob == best && obi < besti)) { best = ob; besti = obi; }
        }
        __syncthreads();
        if (lane == 0) { s_rd[wave] = best; s_ri[wave] = besti; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < MM_WAVES; ++w)
                if (s_rd[w] < best || (s_rd[w] == best && s_ri[w] < besti)) { best = s_rd[w]; besti = s_ri[w]; }
            pair_idx[jb + cidx] = besti;
        }
    }
}

#include "match_screen.inc"
#include "match_screen_wide.inc"

// Every launch of the screen: k_match_prep* + k_match_screen* over one set of pairs -- the padded row count, the 16-byte row test
// (`aligned`: every descriptor pointer of the launch is 16-byte aligned, rows16), the two grids; the kernels follow from the number of
// K = 64 blocks.  `between`: an event recorded after the prep kernel (caelo_match_profile).
static bool rows16(const caelo_pair_set &ps) {
    bool a = true;
    for (int i = 0; i < ps.n; ++i) a = a && (((uintptr_t)ps.p[i].f0 | (uintptr_t)ps.p[i].f1) & 15u) == 0;
    return a;
}
static int screen_launch(const caelo_pair_set &ps, bool aligned, int ld0, int64_t k0_max, int ld1, int64_t k1_max, int dim, hipStream_t s,
                         hipEvent_t between = nullptr) {
    const int nb = dim <= 62 ? 1 : msw_nb(dim);
    const int64_t kpad = ms_pad16(k0_max > k1_max ? k0_max : k1_max);
    const int v4 = (aligned && dim % 4 == 0 && ld0 % 4 == 0 && ld1 % 4 == 0) ? 1 : 0;
    const dim3 grid_prep((unsigned)((kpad / 16 + 3) / 4), 1, ps.n), grid((unsigned)((k1_max + 16 * MS_CT - 1) / (16 * MS_CT)), 1, ps.n);
    void (*screen)(caelo_pair_set, int, int64_t, int, int64_t, int, int64_t, int);
    if (nb == 1) {
        k_match_prep<<<grid_prep, 256, 0, s>>>(ps, ld0, k0_max, dim, kpad, v4);
        screen = k_match_screen;
    } else {
        k_match_prep_wide<<<grid_prep, 256, 0, s>>>(ps, ld0, k0_max, dim, nb, kpad, v4);
        screen = nb == 2 ? k_match_screen_wide<2> : nb == 3 ? k_match_screen_wide<3> : nb == 4 ? k_match_screen_wide<4> : k_match_screen_wide<5>;
    }
    CAELO_LAUNCH_CHECK();
    if (between) CAELO_HIP(hipEventRecord(between, s));
    screen<<<grid, 64 * MS_NW, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim, kpad, v4);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

CAELO_API int caelo_match(caelo_ctx *c, const float *f0, int ld0, int64_t k0_max, const int32_t *n0, const float *f1,
                          int ld1, int64_t k1_max, const int32_t *n1, int dim, int64_t *pair_idx, void *ws, void *stream) {
    CAELO_REQUIRE(c && f0 && f1 && pair_idx && ws, "null argument");
    caelo_pair_set ps = {};
    ps.n = 1;
    ps.p[0].f0 = f0; ps.p[0].n0 = n0; ps.p[0].f1 = f1; ps.p[0].n1 = n1; ps.p[0].pair_idx = pair_idx; ps.p[0].ws_match = ws;
    return match_set(ps, ld0, k0_max, ld1, k1_max, dim, caelo_stream(stream));
}

// The pipeline's launch shape of the NN match -- `n_pairs` pairs of consecutive frame rows ([1024][64] f32: descriptor 0:60) behind
// ONE k_match_prep + ONE k_match_screen launch -- repeated between HIP events on `stream`: ms_host[0] = both kernels, [1] =
// k_match_prep alone, averaged over `repeats` (bench.py's second roofline object; tools/roofline_launch.py for rocprofv3).
CAELO_API int caelo_match_profile(caelo_ctx *c, const float *const *rows, int n_pairs, const int32_t *const *n_key, int64_t *pair_idx,
                                  void *ws, int repeats, void *stream, float *ms_host) {
    CAELO_REQUIRE(c && rows && pair_idx && ws && ms_host && n_pairs >= 1 && n_pairs <= CAELO_FB_MAX && repeats >= 1, "bad argument");
    hipStream_t s = caelo_stream(stream);
    caelo_pair_set ps = {};
    ps.n = n_pairs;
    const size_t wsb = (size_t)caelo_match_ws_bytes(CAELO_MAX_KEYPTS);
    for (int i = 0; i < n_pairs; ++i) {
        ps.p[i].f0 = rows[i]; ps.p[i].f1 = rows[i + 1];
        ps.p[i].n0 = n_key ? n_key[i] : nullptr; ps.p[i].n1 = n_key ? n_key[i + 1] : nullptr;
        ps.p[i].pair_idx = pair_idx + (size_t)i * CAELO_MAX_KEYPTS;
        ps.p[i].ws_match = (char *)ws + (size_t)i * wsb;
    }
    hipEvent_t ev[3];
    for (hipEvent_t &e : ev) CAELO_HIP(hipEventCreate(&e));
    int rc = CAELO_OK;
    float both = 0.f, prep = 0.f;
    for (int r = 0; r < repeats && rc == CAELO_OK; ++r) {
        CAELO_HIP(hipEventRecord(ev[0], s));
        rc = screen_launch(ps, true, 64, CAELO_MAX_KEYPTS, 64, CAELO_MAX_KEYPTS, 60, s, ev[1]);   // (the pipeline's rows: 60-d, one block)
        if (rc != CAELO_OK) break;
        CAELO_HIP(hipEventRecord(ev[2], s));
        CAELO_HIP(hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        CAELO_HIP(hipEventElapsedTime(&a, ev[0], ev[2]));
        CAELO_HIP(hipEventElapsedTime(&b, ev[0], ev[1]));
        both += a; prep += b;
    }
    for (hipEvent_t &e : ev) (void)hipEventDestroy(e);
    ms_host[0] = both / (float)repeats;
    ms_host[1] = prep / (float)repeats;
    return rc;
}

int match_set(const caelo_pair_set &ps, int ld0, int64_t k0_max, int ld1, int64_t k1_max, int dim, hipStream_t s) {
    CAELO_REQUIRE(ps.n >= 1 && ps.n <= CAELO_FB_MAX, "bad pair count");
    CAELO_REQUIRE(dim > 0 && dim <= MSW_MAXDIM && ld0 >= dim && ld1 >= dim && k0_max > 0 && k1_max > 0, "bad shape");
    CAELO_REQUIRE(k0_max + 16 * MM_STEP_TILES < MM_IDX_MASK, "too many frame-0 rows (the row index travels in 21 key bits)");
    // the f16 screen + exact certification (match_screen.inc) for every descriptor width that leaves room for the two norm slots in
    // K = 64 (the reference's descriptors are 60 wide); wider ones: the all-f64 kernel.  Same pair_idx bit for bit
    // (tests/test_gpu_parity.py::test_match_shape_sweep_vs_oracle covers both).  Past 64 the screen again, over several K = 64
    // blocks (match_screen_wide.inc; the workspace is caelo_match_ws_bytes_dim's).
    if (dim <= 62 || dim > MT_MAXDIM) return screen_launch(ps, rows16(ps), ld0, k0_max, ld1, k1_max, dim, s);
    const int64_t tiles = (k1_max + 16 * MM_CT - 1) / (16 * MM_CT);  // workgroups of MM_CT column tiles
    const bool vec = rows16(ps) && (dim % 4 == 0) && (ld0 % 4 == 0) && (ld1 % 4 == 0);
    dim3 grid((unsigned)tiles, 1, ps.n);
    if (vec)
        k_match_mfma<true><<<grid, 64 * MM_WAVES, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim);
    else
        k_match_mfma<false><<<grid, 64 * MM_WAVES, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
