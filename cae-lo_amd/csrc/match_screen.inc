// match_screen.inc -- NN match, round 3: an f16-pipe screen with a rigorous error window, then SciPy-exact f64 on the survivors.
// Part of match.hip.
//
// Reference behaviour restated (never its code): Match.py:257-258, pairIdx = argmin(cdist(Codes0, Codes1), axis=0) -- for every
// frame-1 descriptor the FIRST frame-0 descriptor at minimal float64 Euclidean distance.
//
// k_match_mfma (round 2) evaluates all k0 x k1 distances on the f64 matrix cores: 1.07 GFLOP of f64 per 8 pairs, 43 us at 31 % of
// the pipe, and the f64 MFMA shares its ALUs with the f64 bookkeeping beside it.  But the argmin only needs the few rows that can
// be the minimum.  Round 2 dismissed a low-precision screen ("~100 of 1024 rows survive"); measured on the golden descriptors
// that is wrong by two orders of magnitude: with an error window of 1e-5 (|a|^2 + |b|^2) ONE row survives per column (two where
// descriptors repeat).  So:
//   * both frames become ready-made MFMA fragments of 2-way f16 splits (x = hi + lo, |x - hi - lo| <= max(2^-22 |x|, 2^-25);
//     the MFMA honours f16 subnormals, tools/micro/f16_mfma_subnormal.hip): frame 0 by k_match_prep, into the workspace, as A rows
//     a' = [a_0 .. a_{dim-1}, |a|^2 hi, |a|^2 lo]; frame 1 by the screen's own wavefronts for the columns they own (never in the
//     workspace), as B columns b' = [-2 b_0 .. -2 b_{dim-1}, 1, 1], so that ONE chain of six v_mfma_f32_16x16x32_f16 per 16 x 16 tile
//     (a_lo b_hi, a_hi b_lo, a_hi b_hi over two 32-deep k steps) delivers s_ij ~ |a_i|^2 - 2 <a_i, b_j> = d_ij^2 - |b_j|^2;
//   * k_match_screen sweeps frame 0 twice: first for each column's smallest UPPER bound s + e, then for the rows whose LOWER
//     bound s - e does not exceed it, e_ij = ea_i + eb_j = MS_C (2 |a_i|^2 + |b_j|^2) + MS_A (|a_i|_1 + 1 + 2 |b_j|_1) (the absolute
//     part: see MS_A): the split residuals and the dropped lo lo products are
//     < 4 2^-22 (|a|^2 + |b|^2); the 192 f32 additions of the chain, each assumed to round a partial sum <= 2 |a|^2 + |b|^2, give
//     1.15e-5 -- MS_C = 1.5e-5 covers both with margin (tests/test_gpu_parity.py measures the actual error: < 1e-6);
//   * rows whose lower bound is not above the smallest upper bound are the only ones that can win: one row -> certified without
//     any f64; two to eight -> evaluated exactly like cdist (sequential f64 sum of squared differences, sqrt), first minimum; more
//     (many repeated descriptors) -> the workgroup re-scans the column exactly.  pair_idx is bit-identical to the f64 kernel's.
// Workspace (caelo_match_ws_bytes(max(k0_max, k1_max))): 256 B of statistics | frame 0 as A fragments | ea_i (the row's share of
// the window; +inf for a row whose norm is out of the f16 range).
#define MS_C 1.5e-5f
// the same constant over nb blocks of K = 64 (derivation: match_screen_wide.inc); msw_c(1) is NOT MS_C (1.49976e-5)
__host__ __device__ constexpr float msw_c(int nb) {
    return (1.5f / 1.24f) * (4.0f * 2.384185791015625e-7f + 192.0f * (float)nb * 5.9604644775390625e-8f);
}
// Absolute part of the window (ADVICE r3): below 2^-3 the low half of a 2-way f16 split is an f16 SUBNORMAL (spacing 2^-24), so
// |x - hi - lo| <= max(2^-22 |x|, 2^-25) -- an absolute 2^-25 per element that the relative window above does not cover once the
// descriptors are small (uniform [-1e-3, 1e-3]: 2 of 256 columns certified a wrong row).  Every product carries at most
// 2^-25 (|a_k| + |2 b_k|) of it, the |a|^2 slot 2^-25 more: e_ij += MS_A (|a_i|_1 + 1) + 2 MS_A |b_j|_1 with MS_A = 2^-24.
#define MS_A 5.9604645e-8f
// |x|^2 above this (or not finite) does not go through f16 at all (65504 is the format's end): such a row makes every column of
// the pair, such a column itself, take the exact float64 scan
#define MS_NORM_MAX 3.0e4f
#define MS_FRAG_U4 (2 * 2 * 64)       // uint4 per 16-row tile image: [k step 2][term 2][lane 64]
typedef _Float16 ms_h8 __attribute__((ext_vector_type(8)));
typedef float ms_f4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t ms_pad16(int64_t k) { return (k + 15) / 16 * 16; }
// one pair's workspace: nb = 1 for descriptors up to 62 wide, msw_nb(dim) past 64 (match_screen_wide.inc)
struct MsWs {
    int32_t *stats;
    uint4 *img;     // frame 0 (A operand): [tile][block nb][k step 2][term 2][lane 64]; frame 1's fragments never leave the registers
    float *ea;      // ea_i = 2 C |a_i|^2 + MS_A (|a_i|_1 + 1), C = MS_C / msw_c(nb); +inf when |a_i|^2 is out of range
};
__host__ __device__ inline MsWs ms_ws(void *ws, int64_t kpad, int nb) {
    MsWs w;
    char *p = (char *)ws;
    w.stats = (int32_t *)p;
    w.img = (uint4 *)(p + 256);
    w.ea = (float *)(w.img + (size_t)(kpad / 16) * nb * MS_FRAG_U4);
    return w;
}
static inline int64_t ms_ws_bytes(int64_t kmax, int nb) {
    const int64_t kp = ms_pad16(kmax);
    return 256 + (kp / 16) * nb * MS_FRAG_U4 * 16 + kp * 4;
}

// ---- the operand path of both screens (this file's, over one K = 64 block, and match_screen_wide.inc's, over nb).  Lane (g, m) of a
// wavefront holds row m of a 16-row tile.  SIDE 0: the row itself with |a|^2 (hi, lo) in slots dim, dim + 1; SIDE 1: -2 x the row
// with 1, 1 there.
// channels 64 b + 32 ks + 8 g .. + 7 (ks = 0, 1) of one row; zero past dim and for an invalid row
static __device__ __forceinline__ void ms_load_block(const float *__restrict__ rowp, bool valid, int g, int b, int dim, bool vec, float v[2][8]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int c0 = 64 * b + 32 * ks + 8 * g;
        if (vec) {   // dim % 4 == 0, 16-byte aligned rows
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = p;
            if (valid && c0 < dim) p = *(const float4 *)(rowp + c0);
            if (valid && c0 + 4 < dim) q = *(const float4 *)(rowp + c0 + 4);
            v[ks][0] = p.x; v[ks][1] = p.y; v[ks][2] = p.z; v[ks][3] = p.w; v[ks][4] = q.x; v[ks][5] = q.y; v[ks][6] = q.z; v[ks][7] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[ks][i] = (valid && c0 + i < dim) ? rowp[c0 + i] : 0.0f;
        }
    }
}
// |row|^2 (f32 of the f64 sum; 0 for an invalid row) and |row|_1 over all nb blocks; the four lane groups of a row meet by shuffles
static __device__ __forceinline__ void ms_norms(const float *__restrict__ rowp, bool valid, int g, int nb, int dim, bool vec, float &nf, float &n1f) {
    double nsq = 0.0, n1 = 0.0;
    for (int b = 0; b < nb; ++b) {
        float v[2][8];
        ms_load_block(rowp, valid, g, b, dim, vec, v);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 8; ++i) { nsq += (double)v[ks][i] * (double)v[ks][i]; n1 += fabs((double)v[ks][i]); }
    }
    nsq += __shfl_xor(nsq, 16);
    nsq += __shfl_xor(nsq, 32);
    n1 += __shfl_xor(n1, 16);
    n1 += __shfl_xor(n1, 32);
    nf = valid ? (float)nsq : 0.0f;
    n1f = (float)n1;
}
// the row's (SIDE 0) / column's (SIDE 1) share of the window over nb blocks; +inf when the norm is out of the f16 range (or NaN)
template <int SIDE>
static __device__ __forceinline__ float ms_window(float nf, float n1f, int nb) {
    if (!(nf <= MS_NORM_MAX)) return __builtin_inff();
    const float c = msw_c(nb);
    return SIDE ? fmaf(c, nf, 2.0f * MS_A * n1f) : fmaf(2.0f * c, nf, MS_A * (n1f + 1.0f));
}
// one block of a row as this lane's fragment slots: out[2 ks] the high halves, out[2 ks + 1] the low halves of k step ks
template <int SIDE>
static __device__ __forceinline__ void ms_convert_block(const float v[2][8], int g, int b, int dim, bool in_range, float nf, uint4 out[4]) {
    const _Float16 nh = (_Float16)(in_range ? nf : 0.0f), nl = (_Float16)((in_range ? nf : 0.0f) - (float)nh);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        uint16_t hi[8], lo[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = 64 * b + 32 * ks + 8 * g + i;
            const float x = !in_range ? 0.0f : (SIDE ? -2.0f * v[ks][i] : v[ks][i]);
            _Float16 h = (_Float16)x, l = (_Float16)(x - (float)h);
            if (c == dim) { h = SIDE ? (_Float16)1.0f : nh; l = (_Float16)0.0f; }          // |a|^2 hi x 1
            if (c == dim + 1) { h = SIDE ? (_Float16)1.0f : nl; l = (_Float16)0.0f; }      // |a|^2 lo x 1
            hi[i] = __builtin_bit_cast(uint16_t, h);
            lo[i] = __builtin_bit_cast(uint16_t, l);
        }
        out[2 * ks] = make_uint4(hi[0] | (uint32_t)hi[1] << 16, hi[2] | (uint32_t)hi[3] << 16, hi[4] | (uint32_t)hi[5] << 16, hi[6] | (uint32_t)hi[7] << 16);
        out[2 * ks + 1] = make_uint4(lo[0] | (uint32_t)lo[1] << 16, lo[2] | (uint32_t)lo[3] << 16, lo[4] | (uint32_t)lo[5] << 16, lo[6] | (uint32_t)lo[7] << 16);
    }
}

// one descriptor of at most 62 channels: block 0 alone.  Returns |row|^2 (f32 of the f64 sum); `window` = the row's / column's share
// of the error window (ea_i / eb_j above).  The norms and the window are spelled out here, not ms_norms + ms_window: the one block is
// loaded once, and the window keeps the literal MS_C (msw_c(1) is 1.49976e-5: it would move the windows and the statistics words)
template <int SIDE>
__device__ inline float ms_fragments(const float *__restrict__ f, int ld, int row, bool valid, int g, int dim, bool vec, uint4 out[4], float &window) {
    float v[2][8];
    ms_load_block(f + (size_t)row * ld, valid, g, 0, dim, vec, v);
    double nsq = 0.0, n1 = 0.0;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 8; ++i) { nsq += (double)v[ks][i] * (double)v[ks][i]; n1 += fabs((double)v[ks][i]); }
    nsq += __shfl_xor(nsq, 16);
    nsq += __shfl_xor(nsq, 32);
    n1 += __shfl_xor(n1, 16);
    n1 += __shfl_xor(n1, 32);
    // rows past the frame's count are all-zero fragments and are masked by index in k_match_screen (no sentinel norm: a real
    // |a|^2 between 3e4 and 6.5e4 would have passed one)
    const float nf = valid ? (float)nsq : 0.0f;
    const bool in_range = nf <= MS_NORM_MAX;   // false for NaN too
    window = !in_range ? __builtin_inff()
                       : (SIDE ? fmaf(MS_C, nf, 2.0f * MS_A * (float)n1) : fmaf(2.0f * MS_C, nf, MS_A * ((float)n1 + 1.0f)));
    ms_convert_block<SIDE>(v, g, 0, dim, in_range, nf, out);
    return nf;
}

// frame 0 of every pair as A fragments: one wavefront per 16-row tile (frame 1's 16 columns are converted by the wavefronts that
// own them, in k_match_screen)
static __device__ __forceinline__ void match_prep_body(const caelo_pair_set &ps, int ld0, int64_t k0_max, int dim, int64_t kpad, int vec) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    const int k0 = P.n0 ? min(max(*P.n0, 0), (int)k0_max) : (int)k0_max;
    const MsWs W = ms_ws(P.ws_match, kpad, 1);
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 16 >= ms_pad16(k0_max)) return;
    const int row = tile * 16 + m;
    uint4 fr[4];
    float ea;
    ms_fragments<0>(P.f0, ld0, row, row < k0, g, dim, vec != 0, fr, ea);
    if (g == 0) W.ea[row] = ea;
    uint4 *o = W.img + (size_t)tile * MS_FRAG_U4 + lane;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u * 64] = fr[u];
}
__global__ void __launch_bounds__(256) k_match_prep(const caelo_pair_set ps, int ld0, int64_t k0_max, int dim, int64_t kpad, int vec) {
    match_prep_body(ps, ld0, k0_max, dim, kpad, vec);
}

// cdist's distance of two frame-0 rows to one frame-1 row, exactly as exact_dist computes it (sequential f64 sum of squared
// differences, sqrt) -- but with the three rows fetched 16 channels at a time, all loads of a chunk in flight together: exact_dist's
// 2 x 60 dependent L2 round trips made every workgroup with one undecided column 25 us long.
__device__ inline void ms_exact_pair(const float *__restrict__ a1, const float *__restrict__ a2, const float *__restrict__ b, int dim, bool vec,
                                     double &d1, double &d2) {
    double s1 = 0.0, s2 = 0.0;
    for (int c0 = 0; c0 < dim; c0 += 16) {
        float va[16], vb[16], vc[16];
        if (vec) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x, z = x;
                if (c0 + 4 * q < dim) { x = *(const float4 *)(a1 + c0 + 4 * q); y = *(const float4 *)(a2 + c0 + 4 * q); z = *(const float4 *)(b + c0 + 4 * q); }
                va[4 * q] = x.x; va[4 * q + 1] = x.y; va[4 * q + 2] = x.z; va[4 * q + 3] = x.w;
                vb[4 * q] = y.x; vb[4 * q + 1] = y.y; vb[4 * q + 2] = y.z; vb[4 * q + 3] = y.w;
                vc[4 * q] = z.x; vc[4 * q + 1] = z.y; vc[4 * q + 2] = z.z; vc[4 * q + 3] = z.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool in = c0 + i < dim;
                va[i] = in ? a1[c0 + i] : 0.0f; vb[i] = in ? a2[c0 + i] : 0.0f; vc[i] = in ? b[c0 + i] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (c0 + i < dim) {
                const double e1 = __dsub_rn((double)va[i], (double)vc[i]), e2 = __dsub_rn((double)vb[i], (double)vc[i]);
                s1 = __dadd_rn(s1, __dmul_rn(e1, e1));
                s2 = __dadd_rn(s2, __dmul_rn(e2, e2));
            }
        }
    }
    d1 = sqrt(s1);
    d2 = sqrt(s2);
}

#ifndef MS_CT
#define MS_CT 2      // column tiles per workgroup: every wavefront multiplies its row tiles with both
#endif
#define MS_NW 4      // wavefronts per workgroup: wavefront w owns the row tiles w, w + 4, w + 8, ...
#ifndef MS_RT
#define MS_RT 2
#endif
// MS_RT: row tiles a wavefront has in flight (one "round": tiles w + 4 (2 r + q), q < 2).  Four in flight took 228 registers: no
                     // room beside two of stage 1's 168-register workgroups; two take 128
#define MS_CAND 8    // candidate rows remembered per column (the float64 argmin is one of them); a column with more is re-scanned exactly
// Round 4 re-tile (VERDICT r3 item 4).  Round 3's kernel was ONE load phase per wavefront with all 32 results per lane kept in
// registers: 1 024-thread workgroups of 16 wavefronts x 128 registers -- a whole CU's register file, so inside the pipeline a
// workgroup could only start on a CU that the encoder's persistent grids had left completely alone (13-25 us alone, 212 us on
// average in the pipeline).  Now: 256-thread workgroups (one wavefront per SIMD, < 170 registers, 9 KB of LDS) that fit beside
// one stage-1 workgroup, each wavefront walking its 16 row tiles in rounds of four with the next round's fragments requested as
// soon as a tile's MFMAs are issued -- twice: sweep 1 leaves each column's smallest upper bound, sweep 2 RECOMPUTES the
// products (the matrix pipe is idle anyway: 393 k MFMAs per 8 pairs = 3 us of it) and compares the lower bounds.  Any k0.
// Measured on the way in round 3 (8 pairs per launch): single-sweep forms that keep a sorted top-3 per lane cost 10-13 VALU
// instructions per element (18-20 us); the index in the low mantissa bits of an f32 key widens the window by 2^-12 |s| and sends
// 1 % of the columns to the exact re-scan (36 us).
struct MsRound {
    uint4 fr[MS_RT][4];
    float4 ea[MS_RT];
};
__device__ inline void ms_load_tile(const MsWs &W, int t, int ntiles, int lane, int g, uint4 fr[4], float4 &ea) {
    const int tc = t < ntiles ? t : ntiles - 1;   // past the end: the last tile again, its rows are masked by index
    const uint4 *ap = W.img + (size_t)tc * MS_FRAG_U4 + lane;
#pragma unroll
    for (int u = 0; u < 4; ++u) fr[u] = ap[u * 64];
    ea = *(const float4 *)(W.ea + tc * 16 + 4 * g);
}
// s_ij of one row tile against the workgroup's two column tiles: smallest terms first, the two column tiles' chains alternate
__device__ inline void ms_tile_products(const uint4 fr[4], const ms_h8 bh[MS_CT][2], const ms_h8 bl[MS_CT][2], ms_f4 acc[MS_CT]) {
    ms_h8 ah[2], al[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        ah[ks] = __builtin_bit_cast(ms_h8, fr[2 * ks]);
        al[ks] = __builtin_bit_cast(ms_h8, fr[2 * ks + 1]);
    }
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) acc[ct] = (ms_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int ct = 0; ct < MS_CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[ks], bh[ct][ks], acc[ct], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int ct = 0; ct < MS_CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks], bl[ct][ks], acc[ct], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int ct = 0; ct < MS_CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks], bh[ct][ks], acc[ct], 0, 0, 0);
}

// The tail of both screens (k_match_screen, k_match_screen_wide): what decides pair_idx once sweep 2 has left each column's candidate
// rows in s_cand / s_cnt -- the out-of-range rule, the first-minimum tie rule, the MS_CAND overflow.  Called by the whole workgroup
// after the barrier that ends sweep 2; the shared arrays are the calling kernel's own.  (__forceinline__: a device function that is
// CALLED costs its callers the register budget, DESIGN.md 6; the instruction streams with and without this function were compared,
// profiles/match_shared_tail_asm_diff.txt.)
template <int NW>
static __device__ __forceinline__ void ms_certify_tail(const float *__restrict__ f0, int ld0, int k0, const float *__restrict__ f1, int ld1, int k1, int dim,
                                                       int vec, int64_t *__restrict__ pair_idx, int32_t *stats, int jb, int (&s_cnt)[MS_CT][16],
                                                       int (&s_cand)[MS_CT][16][MS_CAND], double (&s_cd)[MS_CT][16][MS_CAND], float (&sEb)[MS_CT][16],
                                                       int &s_bad_row, int (&s_rescan)[16 * MS_CT], double (&s_rd)[NW], int (&s_ri)[NW]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float BIGF = 3.0e38f;
    const double BIG = 1.0e300;
    // ---- certify.  One candidate: it IS the float64 argmin.  Two to MS_CAND (near ties, repeated descriptors -- equal patches give
    // equal descriptors): the exact cdist distances of the candidates, two per thread (four threads per column), then the first
    // minimum.  Only a column with more candidates than the list holds is re-scanned over all of frame 0.
    if (tid < 16 * MS_CT * (MS_CAND / 2)) {
        const int c32 = tid & (16 * MS_CT - 1), slot = tid / (16 * MS_CT);
        const int ct = c32 >> 4, col = c32 & 15, j = jb + c32;
        const int cnt = s_cnt[ct][col];
        if (j < k1 && cnt >= 2 && cnt <= MS_CAND && 2 * slot < cnt) {
            const int i1 = s_cand[ct][col][2 * slot], i2 = 2 * slot + 1 < cnt ? s_cand[ct][col][2 * slot + 1] : i1;
            double d1, d2;
            ms_exact_pair(f0 + (size_t)i1 * ld0, f0 + (size_t)i2 * ld0, f1 + (size_t)j * ld1, dim, vec != 0, d1, d2);
            s_cd[ct][col][2 * slot] = d1;
            s_cd[ct][col][2 * slot + 1] = d2;
        }
    }
    __syncthreads();
    if (tid < 16 * MS_CT) {
        const int ct = tid >> 4, col = tid & 15;
        const int j = jb + tid;
        int rescan = 0;
        if (j < k1) {
            const int cnt = s_cnt[ct][col];
            // a frame-0 row or this column outside the f16 range: nothing the screen computed about the column means anything
            const bool out_of_range = s_bad_row != 0 || !(sEb[ct][col] < BIGF);
            if (cnt > MS_CAND || cnt < 1 || out_of_range) {
                rescan = 1;
                if (stats) atomicAdd(&stats[0], 1);
            } else if (cnt >= 2) {
                if (stats) atomicAdd(&stats[1], 1);
                double best = s_cd[ct][col][0];
                int besti = s_cand[ct][col][0];
                for (int c = 1; c < cnt; ++c) {
                    const double d = s_cd[ct][col][c];
                    const int i = s_cand[ct][col][c];
                    if (d < best || (d == best && i < besti)) { best = d; besti = i; }
                }
                pair_idx[j] = besti;
            } else {
                pair_idx[j] = s_cand[ct][col][0];  // certified by the screen alone
            }
        }
        s_rescan[tid] = rescan;
    }
    __syncthreads();
    // ---- exact re-scan of a column whose window holds three or more rows (whole workgroup)
    for (int cidx = 0; cidx < 16 * MS_CT; ++cidx) {
        if (!s_rescan[cidx]) continue;  // uniform
        const float *bj = f1 + (size_t)(jb + cidx) * ld1;
        double best = BIG;
        int besti = 0x7FFFFFFF;
        for (int i = tid; i < k0; i += 2 * 64 * NW) {   // rows i and i + 256: ascending per thread, ties resolved by index below
            const int i2 = i + 64 * NW < k0 ? i + 64 * NW : i;
            double da, db;
            ms_exact_pair(f0 + (size_t)i * ld0, f0 + (size_t)i2 * ld0, bj, dim, vec != 0, da, db);
            if (da < best) { best = da; besti = i; }
            if (i2 != i && db < best) { best = db; besti = i2; }
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
            for (int w = 1; w < NW; ++w)
                if (s_rd[w] < best || (s_rd[w] == best && s_ri[w] < besti)) { best = s_rd[w]; besti = s_ri[w]; }
            pair_idx[jb + cidx] = besti;
        }
    }
}

#ifndef MS_OCC
#define MS_OCC 4
#endif
static __device__ __forceinline__ void match_screen_body(const caelo_pair_set &ps, int ld0, int64_t k0_max, int ld1, int64_t k1_max, int dim, int64_t kpad, int vec) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    const float *__restrict__ f0 = P.f0, *__restrict__ f1 = P.f1;
    int64_t *__restrict__ pair_idx = P.pair_idx;
    const MsWs W = ms_ws(P.ws_match, kpad, 1);
    int32_t *stats = W.stats;
    constexpr int NW = MS_NW;
    __shared__ uint4 sB[MS_CT][4][64];
    __shared__ float sEb[MS_CT][16];
    __shared__ float sU[NW][MS_CT][16];
    __shared__ int s_cnt[MS_CT][16];
    __shared__ int s_cand[MS_CT][16][MS_CAND];
    __shared__ double s_cd[MS_CT][16][MS_CAND];
    __shared__ int s_rescan[16 * MS_CT];
    __shared__ int s_bad_row;
    __shared__ double s_rd[NW];
    __shared__ int s_ri[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, x = lane & 15;
    const int k0 = P.n0 ? min(max(*P.n0, 0), (int)k0_max) : (int)k0_max;
    const int k1 = P.n1 ? min(max(*P.n1, 0), (int)k1_max) : (int)k1_max;
    const int jb = blockIdx.x * 16 * MS_CT;
    if (jb >= k1) return;
    if (k0 == 0) {  // no frame-0 descriptor at all (the reference's argmin would raise): index 0, the pose fails
        if (tid < 16 * MS_CT && jb + tid < k1) pair_idx[jb + tid] = 0;
        return;
    }
    const float BIGF = 3.0e38f;
    const int ntiles = (k0 + 15) >> 4;
    const int nrounds = (ntiles + NW * MS_RT - 1) / (NW * MS_RT);
    // ---- round 0 of this wavefront's row tiles is requested before anything else
    MsRound R;
#pragma unroll
    for (int q = 0; q < MS_RT; ++q) ms_load_tile(W, wave + NW * q, ntiles, lane, g, R.fr[q], R.ea[q]);
    // ---- the workgroup's 2 x 16 columns as B fragments, converted once (wavefronts 0, 1) and shared through LDS (a column past
    // k1 computes on zeros: same instruction stream, never read)
    if (tid < 16 * MS_CT) s_cnt[tid >> 4][tid & 15] = 0;
    if (tid == 0) s_bad_row = 0;
    if (wave < MS_CT) {
        const int jcol = jb + wave * 16 + x;
        uint4 bfr[4];
        float ebv;
        ms_fragments<1>(f1, ld1, jcol < k1 ? jcol : 0, jcol < k1, g, dim, vec != 0, bfr, ebv);
#pragma unroll
        for (int u = 0; u < 4; ++u) sB[wave][u][lane] = bfr[u];
        if (g == 0) sEb[wave][x] = ebv;
    }
    __syncthreads();
    ms_h8 bh[MS_CT][2], bl[MS_CT][2];
    float eb[MS_CT];
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bh[ct][ks] = __builtin_bit_cast(ms_h8, sB[ct][2 * ks][lane]);
            bl[ct][ks] = __builtin_bit_cast(ms_h8, sB[ct][2 * ks + 1][lane]);
        }
        eb[ct] = sEb[ct][x];
    }
    // ---- sweep 1: each column's smallest upper bound s + ea_i (eb_j is added once at the end).  C row 4g + r of tile t is frame-0
    // descriptor 16 t + 4g + r; rows >= k0 are masked by index
    float Umin[MS_CT];
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) Umin[ct] = BIGF;
    bool bad_row = false;
    for (int r = 0; r < nrounds; ++r) {
#pragma unroll
        for (int q = 0; q < MS_RT; ++q) {
            const int t = wave + NW * (MS_RT * r + q);
            ms_f4 acc[MS_CT];
            ms_tile_products(R.fr[q], bh, bl, acc);
            const float eav[4] = {R.ea[q].x, R.ea[q].y, R.ea[q].z, R.ea[q].w};
            // the slot's next tile: sweep 1's next round, or sweep 2's first
            ms_load_tile(W, r + 1 < nrounds ? t + NW * MS_RT : wave + NW * q, ntiles, lane, g, R.fr[q], R.ea[q]);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const bool rv = 16 * t + 4 * g + rr < k0;
                bad_row |= rv && !(eav[rr] < BIGF);
#pragma unroll
                for (int ct = 0; ct < MS_CT; ++ct)
                    if (rv) Umin[ct] = fminf(Umin[ct], acc[ct][rr] + eav[rr]);
            }
        }
    }
    // ---- the columns' smallest upper bounds: the 4 lane groups by shuffles, the wavefronts through LDS
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) {
        Umin[ct] = fminf(Umin[ct], __shfl_xor(Umin[ct], 16));
        Umin[ct] = fminf(Umin[ct], __shfl_xor(Umin[ct], 32));
        if (g == 0) sU[wave][ct][x] = Umin[ct];
    }
    if (__ballot(bad_row) != 0ull && lane == 0) s_bad_row = 1;
    __syncthreads();
    // ---- sweep 2: the rows whose lower bound s - ea_i - eb_j does not exceed the column's smallest upper bound (about one per column)
    float thr[MS_CT];
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) {
        float u = BIGF;
#pragma unroll
        for (int h = 0; h < NW; ++h) u = fminf(u, sU[h][ct][x]);
        thr[ct] = u + 2.0f * eb[ct];
    }
    for (int r = 0; r < nrounds; ++r) {
#pragma unroll
        for (int q = 0; q < MS_RT; ++q) {
            const int t = wave + NW * (MS_RT * r + q);
            ms_f4 acc[MS_CT];
            ms_tile_products(R.fr[q], bh, bl, acc);
            const float eav[4] = {R.ea[q].x, R.ea[q].y, R.ea[q].z, R.ea[q].w};
            if (r + 1 < nrounds) ms_load_tile(W, t + NW * MS_RT, ntiles, lane, g, R.fr[q], R.ea[q]);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const bool rv = 16 * t + 4 * g + rr < k0;
#pragma unroll
                for (int ct = 0; ct < MS_CT; ++ct)
                    if (rv && acc[ct][rr] - eav[rr] <= thr[ct]) {
                        const int p = atomicAdd(&s_cnt[ct][x], 1);
                        if (p < MS_CAND) s_cand[ct][x][p] = 16 * t + 4 * g + rr;
                    }
            }
        }
    }
    __syncthreads();
    ms_certify_tail<NW>(f0, ld0, k0, f1, ld1, k1, dim, vec, pair_idx, stats, jb, s_cnt, s_cand, s_cd, sEb, s_bad_row, s_rescan, s_rd, s_ri);
}
__global__ void __launch_bounds__(64 * MS_NW, MS_OCC) k_match_screen(const caelo_pair_set ps, int ld0, int64_t k0_max, int ld1, int64_t k1_max,
                                                             int dim, int64_t kpad, int vec) {
    match_screen_body(ps, ld0, k0_max, ld1, k1_max, dim, kpad, vec);
}
