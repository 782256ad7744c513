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
// Shared with the narrow screen, all in match_screen.inc: the operand path (ms_load_block / ms_norms / ms_window / ms_convert_block,
// msw_c), the workspace (ms_ws with nb images per tile) and the tail that decides pair_idx (ms_certify_tail).  They are
// `static __device__ __forceinline__`: what DESIGN.md 6 warns of is a function hipcc stops inlining, and a forced inline cannot
// become a call.  The kernels with and without the shared functions were compared instruction by instruction
// (profiles/match_shared_tail_asm_diff.txt): the same floating-point instructions everywhere, no register or LDS figure above the
// separate copies'.
// Workspace (caelo_match_ws_bytes_dim): 256 B of statistics | frame 0 as A fragments, nb images per 16-row tile | ea_i.
#define MSW_MAXDIM 256
__host__ __device__ inline int msw_nb(int dim) { return (dim + 2 + 63) / 64; }

// frame 0 of every pair as A fragments: one wavefront per 16-row tile, a first pass over the row for its norms, a second for the blocks
__global__ void __launch_bounds__(256) k_match_prep_wide(const caelo_pair_set ps, int ld0, int64_t k0_max, int dim, int nb, int64_t kpad, int vec) {
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    const int k0 = P.n0 ? min(max(*P.n0, 0), (int)k0_max) : (int)k0_max;
    const MsWs W = ms_ws(P.ws_match, kpad, nb);
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 16 >= ms_pad16(k0_max)) return;
    const int row = tile * 16 + m;
    const bool valid = row < k0;
    const float *rowp = P.f0 + (size_t)(valid ? row : 0) * ld0;
    float nf, n1f;
    ms_norms(rowp, valid, g, nb, dim, vec != 0, nf, n1f);
    const float ea = ms_window<0>(nf, n1f, nb);
    if (g == 0) W.ea[row] = ea;
    uint4 *o = W.img + (size_t)tile * nb * MS_FRAG_U4 + lane;
    for (int b = 0; b < nb; ++b) {
        float v[2][8];
        uint4 fr[4];
        ms_load_block(rowp, valid, g, b, dim, vec != 0, v);
        ms_convert_block<0>(v, g, b, dim, nf <= MS_NORM_MAX, nf, fr);
#pragma unroll
        for (int u = 0; u < 4; ++u) o[(b * 4 + u) * 64] = fr[u];
    }
}

template <int NB>
static __device__ __forceinline__ void msw_load_tile(const MsWs &W, int t, int ntiles, int lane, int g, uint4 (&fr)[NB * 4], float4 &ea) {
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
    const caelo_pair_dev &P = ps.p[blockIdx.z];
    const float *__restrict__ f0 = P.f0, *__restrict__ f1 = P.f1;
    int64_t *__restrict__ pair_idx = P.pair_idx;
    const MsWs W = ms_ws(P.ws_match, kpad, NB);
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
        ms_norms(colp, valid, g, NB, dim, vec != 0, nf, n1f);
        eb[ct] = ms_window<1>(nf, n1f, NB);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float v[2][8];
            uint4 o[4];
            ms_load_block(colp, valid, g, b, dim, vec != 0, v);
            ms_convert_block<1>(v, g, b, dim, nf <= MS_NORM_MAX, nf, o);
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
    ms_certify_tail<NW>(f0, ld0, k0, f1, ld1, k1, dim, vec, pair_idx, stats, jb, s_cnt, s_cand, s_cd, sEb, s_bad_row, s_rescan, s_rd, s_ri);
}
