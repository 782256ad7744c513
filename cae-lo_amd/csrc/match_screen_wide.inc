// match_screen_wide.inc -- the f16 screen of match_screen.inc over several K = 64 blocks: descriptors 65 .. 256 wide (the published
// comparison's 128-d USIP descriptors, Scripts/GenerateTrajactory.m:193-203).  Part of match.hip, after match_screen.inc.
//
// Same method, same certificates: 2-way f16 splits, A rows [a, |a|^2 hi, |a|^2 lo], B columns [-2 b, 1, 1], two sweeps of frame 0,
// one survivor certified, two to MS_CAND decided by cdist's sequential float64 sum over all `dim` channels (ms_exact_pair), more
// re-scanned exactly by the workgroup.  What changes is the depth of the chain: nb = ceil((dim + 2) / 64) blocks of K = 64, the two
// norm slots at channels dim, dim + 1 of the LAST block (255 and 256 need a fifth block for them), channels past them zero:
// 6 nb v_mfma_f32_16x16x32_f16 per 16 x 16 tile, all lo x hi terms first, then hi x lo, then hi x hi.
//
// The window, re-derived for nb blocks as match_screen.inc:16-20 does for one:  e_ij = ea_i + eb_j
//     = msw_c(nb) (2 |a_i|^2 + |b_j|^2) + MS_A (|a_i|_1 + 1 + 2 |b_j|_1).
//   * Split residuals and dropped lo lo products: per product |a_k| |2 b_k| (2^-22 + 2^-22 + 2^-22), summed with Cauchy-Schwarz and
//     2 |a||b| <= |a|^2 + |b|^2, plus 2^-22 |a|^2 for the norm slot: < 4 2^-22 (|a|^2 + |b|^2).  A sum over channels: it does not
//     depend on how many blocks the channels are spread over.
//   * The chain is now 6 nb MFMAs of K = 32: 192 nb f32 additions, each assumed (as there) to round a partial sum that is at most
//     |a|^2 + 2 sum |a_k b_k| <= 2 |a|^2 + |b|^2: 192 nb 2^-24 (2 |a|^2 + |b|^2).
//   * Together (4 2^-22 + 192 nb 2^-24) = 1.24e-5 at nb = 1, where MS_C = 1.5e-5: msw_c(nb) keeps that ratio,
//     (1.5 / 1.24) (4 2^-22 + 192 nb 2^-24) = 2.88e-5, 4.27e-5, 5.65e-5, 7.04e-5 for nb = 2 .. 5.
//   * The absolute part (f16 subnormal low halves, MS_A): 2^-25 per ELEMENT, so each product carries at most
//     2^-25 (|a_k| + |2 b_k|) of it and the |a|^2 slot 2^-25 more -- a sum over the channels again: MS_A (|a|_1 + 1) + 2 MS_A |b|_1
//     with MS_A = 2^-24 holds as it stands, the 1-norms simply run over all `dim` channels.
//   * MS_NORM_MAX is a property of the f16 format, not of the width: unchanged (elements <= 174, -2 b <= 347, partial sums < 1e5).
//
// Frame 1's fragments stay in registers as in the narrow kernel: 16 VGPRs per block and column tile, 32 nb for the workgroup's two
// column tiles.  Every wavefront converts them for itself (lane (g, x) of a B fragment holds column x, channels 8 g .. 8 g + 7 of
// each 32-deep step -- exactly what the lane would hold of an A tile), so nothing but eb_j goes through LDS.  One row tile in
// flight per wavefront (16 nb VGPRs) instead of two; the launch bounds trade occupancy for registers as nb grows
// (DESIGN.md 5.2a has the compiled figures).  k_match_prep_wide takes nb at run time (it is a conversion pass); the screen is
// compiled per nb so that the fragment arrays index statically.
// The tail (certify / exact pairs / re-scan) repeats match_screen_body's on purpose: sharing it would mean re-inlining a new
// function into k_match_screen, whose instructions are pinned (DESIGN.md 6).
// Workspace (caelo_match_ws_bytes_dim): 256 B of statistics | frame 0 as A fragments, nb images per 16-row tile | ea_i.
#define MSW_MAXDIM 256
__host__ __device__ inline int msw_nb(int dim) { return (dim + 2 + 63) / 64; }
__host__ __device__ constexpr float msw_c(int nb) {
    return (1.5f / 1.24f) * (4.0f * 2.384185791015625e-7f + 192.0f * (float)nb * 5.9604644775390625e-8f);
}

struct MswWs {
    int32_t *stats;
    uint4 *img;     // frame 0: [tile][block nb][k step 2][term 2][lane 64]
    float *ea;      // ea_i = 2 msw_c |a_i|^2 + MS_A (|a_i|_1 + 1), +inf when |a_i|^2 is out of range
};
__host__ __device__ inline MswWs msw_ws(void *ws, int64_t kpad, int nb) {
    MswWs w;
    char *p = (char *)ws;
    w.stats = (int32_t *)p;
    w.img = (uint4 *)(p + 256);
    w.ea = (float *)(w.img + (size_t)(kpad / 16) * nb * MS_FRAG_U4);
    return w;
}
static inline int64_t msw_ws_bytes(int64_t kmax, int nb) {
    const int64_t kp = ms_pad16(kmax);
    return 256 + (kp / 16) * nb * MS_FRAG_U4 * 16 + kp * 4;
}

// channels 64 b + 32 ks + 8 g .. + 7 (ks = 0, 1) of one row; zero past dim and for an invalid row
static __device__ __forceinline__ void msw_load_block(const float *__restrict__ rowp, bool valid, int g, int b, int dim, bool vec, float v[2][8]) {
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
static __device__ __forceinline__ void msw_norms(const float *__restrict__ rowp, bool valid, int g, int nb, int dim, bool vec, float &nf, float &n1f) {
    double nsq = 0.0, n1 = 0.0;
    for (int b = 0; b < nb; ++b) {
        float v[2][8];
        msw_load_block(rowp, valid, g, b, dim, vec, v);
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
// the row's (SIDE 0) / column's (SIDE 1) share of the window; +inf when the norm is out of the f16 range (or NaN)
template <int SIDE>
static __device__ __forceinline__ float msw_window(float nf, float n1f, int nb) {
    if (!(nf <= MS_NORM_MAX)) return __builtin_inff();
    const float c = msw_c(nb);
    return SIDE ? fmaf(c, nf, 2.0f * MS_A * n1f) : fmaf(2.0f * c, nf, MS_A * (n1f + 1.0f));
}
// one block of a row as this lane's fragment slots: out[2 ks] the high halves, out[2 ks + 1] the low halves of k step ks
template <int SIDE>
static __device__ __forceinline__ void msw_convert_block(const float v[2][8], int g, int b, int dim, bool in_range, float nf, uint4 out[4]) {
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

// frame 0 of every pair as A fragments: one wavefront per 16-row tile, a first pass over the row for its norms, a second for the blocks
__global__ void __launch_bounds__(256) k_match_prep_wide(const caelo_pair_set ps, int ld0, int64_t k0_max, int dim, int nb, int64_t kpad, int vec) {
    const auto &P = pair_of(ps, blockIdx.z);
    const int k0 = P.n0 ? min(max(*P.n0, 0), (int)k0_max) : (int)k0_max;
    const MswWs W = msw_ws(P.ws_match, kpad, nb);
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 16 >= ms_pad16(k0_max)) return;
    const int row = tile * 16 + m;
    const bool valid = row < k0;
    const float *rowp = P.f0 + (size_t)(valid ? row : 0) * ld0;
    float nf, n1f;
    msw_norms(rowp, valid, g, nb, dim, vec != 0, nf, n1f);
    const float ea = msw_window<0>(nf, n1f, nb);
    if (g == 0) W.ea[row] = ea;
    uint4 *o = W.img + (size_t)tile * nb * MS_FRAG_U4 + lane;
    for (int b = 0; b < nb; ++b) {
        float v[2][8];
        uint4 fr[4];
        msw_load_block(rowp, valid, g, b, dim, vec != 0, v);
        msw_convert_block<0>(v, g, b, dim, nf <= MS_NORM_MAX, nf, fr);
#pragma unroll
        for (int u = 0; u < 4; ++u) o[(b * 4 + u) * 64] = fr[u];
    }
}

template <int NB>
static __device__ __forceinline__ void msw_load_tile(const MswWs &W, int t, int ntiles, int lane, int g, uint4 (&fr)[NB * 4], float4 &ea) {
    const int tc = t < ntiles ? t : ntiles - 1;   // past the end: the last tile again, its rows are masked by index
    const uint4 *ap = W.img + (size_t)tc * NB * MS_FRAG_U4 + lane;
#pragma unroll
    for (int u = 0; u < NB * 4; ++u) fr[u] = ap[u * 64];
    ea = *(const float4 *)(W.ea + tc * 16 + 4 * g);
}
// s_ij of one row tile against the workgroup's two column tiles: smallest terms first, the two column tiles' chains alternate
template <int NB>
static __device__ __forceinline__ void msw_tile_products(const uint4 (&fr)[NB * 4], const ms_h8 (&bh)[MS_CT][NB * 2], const ms_h8 (&bl)[MS_CT][NB * 2],
                                                         ms_f4 acc[MS_CT]) {
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) acc[ct] = (ms_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NB * 2; ++ks)
#pragma unroll
        for (int ct = 0; ct < MS_CT; ++ct)
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ms_h8, fr[2 * ks + 1]), bh[ct][ks], acc[ct], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < NB * 2; ++ks)
#pragma unroll
        for (int ct = 0; ct < MS_CT; ++ct)
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ms_h8, fr[2 * ks]), bl[ct][ks], acc[ct], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < NB * 2; ++ks)
#pragma unroll
        for (int ct = 0; ct < MS_CT; ++ct)
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ms_h8, fr[2 * ks]), bh[ct][ks], acc[ct], 0, 0, 0);
}

// workgroups per CU the screen is compiled for: 256 / 512 registers per lane (three at nb = 2 and two at nb = 4 spilled)
#define MSW_OCC(NB) ((NB) <= 3 ? 2 : 1)
template <int NB>
__global__ void __launch_bounds__(64 * MS_NW, MSW_OCC(NB)) k_match_screen_wide(const caelo_pair_set ps, int ld0, int64_t k0_max, int ld1, int64_t k1_max,
                                                                                int dim, int64_t kpad, int vec) {
    const auto &P = pair_of(ps, blockIdx.z);
    const float *__restrict__ f0 = P.f0, *__restrict__ f1 = P.f1;
    int64_t *__restrict__ pair_idx = P.pair_idx;
    const MswWs W = msw_ws(P.ws_match, kpad, NB);
    int32_t *stats = W.stats;
    constexpr int NW = MS_NW;
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
    const double BIG = 1.0e300;
    const int ntiles = (k0 + 15) >> 4;
    const int nrounds = (ntiles + NW - 1) / NW;
    // ---- this wavefront's first row tile is requested before anything else
    uint4 fr[NB * 4];
    float4 ea;
    msw_load_tile<NB>(W, wave, ntiles, lane, g, fr, ea);
    // ---- the workgroup's 2 x 16 columns as B fragments, converted by every wavefront for itself (a column past k1 computes on
    // zeros: same instruction stream, never read)
    if (tid < 16 * MS_CT) s_cnt[tid >> 4][tid & 15] = 0;
    if (tid == 0) s_bad_row = 0;
    ms_h8 bh[MS_CT][NB * 2], bl[MS_CT][NB * 2];
    float eb[MS_CT];
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) {
        const int jcol = jb + ct * 16 + x;
        const bool valid = jcol < k1;
        const float *colp = f1 + (size_t)(valid ? jcol : 0) * ld1;
        float nf, n1f;
        msw_norms(colp, valid, g, NB, dim, vec != 0, nf, n1f);
        eb[ct] = msw_window<1>(nf, n1f, NB);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float v[2][8];
            uint4 o[4];
            msw_load_block(colp, valid, g, b, dim, vec != 0, v);
            msw_convert_block<1>(v, g, b, dim, nf <= MS_NORM_MAX, nf, o);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bh[ct][2 * b + ks] = __builtin_bit_cast(ms_h8, o[2 * ks]);
                bl[ct][2 * b + ks] = __builtin_bit_cast(ms_h8, o[2 * ks + 1]);
            }
        }
        if (wave == 0 && g == 0) sEb[ct][x] = eb[ct];
    }
    __syncthreads();
    // ---- sweep 1: each column's smallest upper bound s + ea_i (eb_j is added once at the end).  C row 4g + r of tile t is frame-0
    // descriptor 16 t + 4g + r; rows >= k0 are masked by index
    float Umin[MS_CT];
#pragma unroll
    for (int ct = 0; ct < MS_CT; ++ct) Umin[ct] = BIGF;
    bool bad_row = false;
    for (int r = 0; r < nrounds; ++r) {
        const int t = wave + NW * r;
        ms_f4 acc[MS_CT];
        msw_tile_products<NB>(fr, bh, bl, acc);
        const float eav[4] = {ea.x, ea.y, ea.z, ea.w};
        // the next tile: sweep 1's next round, or sweep 2's first
        msw_load_tile<NB>(W, r + 1 < nrounds ? t + NW : wave, ntiles, lane, g, fr, ea);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const bool rv = 16 * t + 4 * g + rr < k0;
            bad_row |= rv && !(eav[rr] < BIGF);
#pragma unroll
            for (int ct = 0; ct < MS_CT; ++ct)
                if (rv) Umin[ct] = fminf(Umin[ct], acc[ct][rr] + eav[rr]);
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
        const int t = wave + NW * r;
        ms_f4 acc[MS_CT];
        msw_tile_products<NB>(fr, bh, bl, acc);
        const float eav[4] = {ea.x, ea.y, ea.z, ea.w};
        if (r + 1 < nrounds) msw_load_tile<NB>(W, t + NW, ntiles, lane, g, fr, ea);
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
    __syncthreads();
    // ---- certify, as match_screen_body does.  One candidate: it IS the float64 argmin.  Two to MS_CAND: the exact cdist distances of
    // the candidates, two per thread (four threads per column), then the first minimum.  More: the column is re-scanned.
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
    // ---- exact re-scan of a column whose window holds more rows than the list (whole workgroup)
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

static int match_set_wide(const caelo_pair_set &ps, int ld0, int64_t k0_max, int ld1, int64_t k1_max, int dim, hipStream_t s) {
    const int nb = msw_nb(dim);
    const int64_t kpad = ms_pad16(k0_max > k1_max ? k0_max : k1_max);
    bool v4 = (dim % 4 == 0) && (ld0 % 4 == 0) && (ld1 % 4 == 0);
    for (int i = 0; i < ps.n; ++i) v4 = v4 && (((uintptr_t)ps.p[i].f0 | (uintptr_t)ps.p[i].f1) & 15u) == 0;
    k_match_prep_wide<<<dim3((unsigned)((kpad / 16 + 3) / 4), 1, ps.n), 256, 0, s>>>(ps, ld0, k0_max, dim, nb, kpad, v4 ? 1 : 0);
    CAELO_LAUNCH_CHECK();
    const dim3 grid((unsigned)((k1_max + 16 * MS_CT - 1) / (16 * MS_CT)), 1, ps.n);
    switch (nb) {
    case 2: k_match_screen_wide<2><<<grid, 64 * MS_NW, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim, kpad, v4 ? 1 : 0); break;
    case 3: k_match_screen_wide<3><<<grid, 64 * MS_NW, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim, kpad, v4 ? 1 : 0); break;
    case 4: k_match_screen_wide<4><<<grid, 64 * MS_NW, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim, kpad, v4 ? 1 : 0); break;
    default: k_match_screen_wide<5><<<grid, 64 * MS_NW, 0, s>>>(ps, ld0, k0_max, ld1, k1_max, dim, kpad, v4 ? 1 : 0); break;
    }
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
